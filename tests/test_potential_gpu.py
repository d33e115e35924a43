"""GPU: the per-body potential of the Hermite sweeps (option "potential"), murbhip_download_potential and
murbhip_potential_energy, through the C ABI and the plugin.

Yardstick: tests/helpers/potential_ref.py (numpy fp64, written from include/murbhip.h, pinned by tests/test_potential_host.py).
The bound everywhere is the project's force bound TOL_F64_MAX = 2e-6 relative to the fp64 phi_i (all terms are positive, so the
sum of the term magnitudes is phi_i itself), and the same 2e-6 for potential_energy against -1/2 sum m_i phi_i of the fp64 sum."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_block_ref as B      # noqa: E402
import hermite_ref as H            # noqa: E402
import nearest_ref as N            # noqa: E402
import potential_ref as PR         # noqa: E402
from active_sets import active_sets   # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
TOL = PR.TOL_F64_MAX
Q, V = PR.Q, PR.V
ETA, ETA_START = 0.02, 0.01
JSPLITS = (1, 3, 8)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hermite_sim(gpu, s, soft, potential=1, **opts):
    sim = gpu.Simulation(len(s["qx"]), soft=soft)
    sim.set_option("integrator", 2)
    sim.set_option("potential", potential)
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.upload(s)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def assert_phi(got, want, what, rows=None):
    rows = np.arange(len(want)) if rows is None else np.asarray(rows)
    assert np.isfinite(got[rows]).all() and not np.signbit(got[rows]).any(), what
    e = PR.rel_err(got[rows], want[rows])
    w = int(np.argmax(e)) if len(e) else 0
    print(f"{what}: phi off by at most {e.max(initial=0.0):.2e} of the fp64 value (bound {TOL:.0e}), body {rows[w] if len(e) else '-'}")
    assert e.max(initial=0.0) <= TOL, f"{what}: phi of body {rows[w]} (tile {rows[w] // PR.TILE}, offset {rows[w] % PR.TILE}) off by {e[w]:.3e}; {(e > TOL).sum()} bodies over"


def assert_energy(got, s, want_phi, what):
    want = PR.energy_of(s, want_phi)
    err = abs(got - want) / abs(want) if want != 0.0 else abs(got)
    print(f"{what}: potential energy {got:.9e}, fp64 {want:.9e}, off by {err:.2e} (bound {TOL:.0e})")
    assert err <= TOL, what


# --------------------------------------------------------------------------------------------------------------------- 1. dense
@pytest.mark.parametrize("n", [1, 2, 513, 1024, 2049])
def test_dense(gpu, n):
    """Every body massive (the lattice of the "nearest" tests, with its coincident pair and its massless body): phi and the
    energy within the bound for "jsplit" 1, 3 and 8, accelerations and jerks those of "potential" 0 bit for bit, and a step of
    dt = 0 — whose predicted state is the current one — leaves phi as it is, bit for bit."""
    s, soft = N.lattice(n)
    want = PR.phi_of(s, soft)
    for jsplit in JSPLITS:
        with hermite_sim(gpu, s, soft, potential=0, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            plain = (np.stack(sim.acc()), np.stack(sim.jerk()))
            assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.potential_energy) == E_STATE
        with hermite_sim(gpu, s, soft, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            phi = sim.potential()
            w = sim.potential_energy()
            a, j = np.stack(sim.acc()), np.stack(sim.jerk())
            sim.step(0.0)
            phi1 = sim.potential()
        assert np.array_equal(bits(a), bits(plain[0])) and np.array_equal(bits(j), bits(plain[1])), \
            f"n={n} jsplit {jsplit}: the forces changed with the option"
        if n == 1:
            assert phi[0] == 0.0 and not np.signbit(phi[0]) and w == 0.0
        assert_phi(phi, want, f"n={n} jsplit {jsplit}")
        assert_energy(w, s, want, f"n={n} jsplit {jsplit}")
        assert np.array_equal(bits(phi1), bits(phi)), f"n={n} jsplit {jsplit}: a step of dt = 0 changed phi"


# -------------------------------------------------------------------------------------------------------------- 2. the own term
@pytest.mark.parametrize("n", [2, 514])
def test_own_term_never_enters_the_sum(gpu, n):
    """Two bodies of 1e30 kg, 1e10 m apart, soft 1e6 m: the own term is 1e4 x the pair term, and a sum that held it once misses
    the bound by a factor of 50 and more (tests/test_potential_host.py).  n = 514: the two in slots 5 and 513, in two tiles, the
    rest massless and far away — their phi are checked too."""
    s, soft, (a, b) = PR.own_term_pair(n)
    want = PR.phi_of(s, soft)
    for jsplit in (1, 3):
        with hermite_sim(gpu, s, soft, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            phi = sim.potential()
            w = sim.potential_energy()
        assert_phi(phi, want, f"own term n={n} jsplit {jsplit}: the two", rows=[a, b])
        assert_phi(phi, want, f"own term n={n} jsplit {jsplit}: all")
        assert_energy(w, s, want, f"own term n={n} jsplit {jsplit}")


# ------------------------------------------------------------------------------------------------------- 3. coincident bodies
@pytest.mark.parametrize("pair", PR.COINCIDENT_PAIRS)
def test_coincident_bodies_count(gpu, pair):
    """Two massive bodies at one position — in the two slots of a pair, in two lanes, in two tiles: the exclusion is by slot, so
    each has the other's G m / soft in its phi."""
    s, soft = PR.coincident(pair)
    want = PR.phi_of(s, soft)
    gm = H._gm(s)
    a, b = pair
    for jsplit in (1, 2):
        with hermite_sim(gpu, s, soft, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            phi = sim.potential()
        assert_phi(phi, want, f"coincident {pair} jsplit {jsplit}")
        assert phi[a] > 0.999 * gm[b] / float(soft) and phi[b] > 0.999 * gm[a] / float(soft)


# ---------------------------------------------------------------------------------------------------------- 4. sparse sources
@lru_cache(maxsize=None)
def sparse_truth():
    s, soft, src = PR.sparse()
    return s, soft, src, PR.phi_of(s, soft)


@pytest.mark.parametrize("jsplit", JSPLITS)
def test_sparse_sources(gpu, jsplit):
    """n = 2049, 16 sources over all tiles (first and last slot of a tile included), everything else massless: one lost or
    doubled term is far above the bound on every body (the power condition is asserted in tests/test_potential_host.py)."""
    s, soft, src, want = sparse_truth()
    with hermite_sim(gpu, s, soft, jsplit=jsplit) as sim:
        sim.compute_acc_jerk()
        phi = sim.potential()
        w = sim.potential_energy()
    assert_phi(phi, want, f"sparse jsplit {jsplit}")
    assert_energy(w, s, want, f"sparse jsplit {jsplit}")


# -------------------------------------------------------------------------------------------------------------- 5. block steps
@lru_cache(maxsize=None)
def cluster(n):
    return B.cluster(n)


def snapshot(sim):
    st = sim.state()
    return {"q": np.stack([st[k] for k in Q]), "v": np.stack([st[k] for k in V]), "a": np.stack(sim.acc()),
            "j": np.stack(sim.jerk()), "ticks": sim.block_state()[0], "levels": sim.block_state()[1], "phi": sim.potential()}


def test_block_step_replay(gpu):
    """cluster(256), one block step per call with "block_units" fixed: the active bodies' phi are the fp64 sums at the predicted
    state of all bodies, the inactive bodies' phi do not change by a bit; potential_energy answers while the block is open,
    energy does not; state, (a, j), ticks and levels are those of "potential" 0 bit for bit."""
    s, period = cluster(256)
    dt_max, kmax = float(np.float32(period / 2.0)), 12
    gm = H._gm(s)
    sims = [hermite_sim(gpu, s, B.SOFT, potential=p, block_units=16) for p in (1, 0)]
    try:
        for sim in sims:
            sim.compute_acc_jerk()
        assert_phi(sims[0].potential(), PR.phi_of(s, B.SOFT), "starting evaluation")
        partial, opened, before = 0, 0, None      # a snapshot needs ticks and levels: they exist behind the first call
        for step in range(24):
            outs = [sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=1) for sim in sims]
            assert outs[0] == outs[1], f"step {step}: the counts differ with the option"
            now = snapshot(sims[0])
            st0 = sims[1].state()
            other = {"q": np.stack([st0[k] for k in Q]), "v": np.stack([st0[k] for k in V]), "a": np.stack(sims[1].acc()),
                     "j": np.stack(sims[1].jerk())}
            for k in ("q", "v", "a", "j"):
                assert np.array_equal(bits(now[k]), bits(other[k])), f"step {step}: {k} changed with the option"
            assert np.array_equal(now["ticks"], sims[1].block_state()[0]) and np.array_equal(now["levels"], sims[1].block_state()[1])
            if not outs[0]["synchronised"]:
                opened += 1
                w = sims[0].potential_energy()      # allowed while the block is open ...
                assert np.isfinite(w) and w < 0.0
                assert abs(w - PR.energy_of(s, now["phi"])) <= 1e-12 * abs(w)      # ... and it is the fp64 sum of what potential() returns
                assert code_of(gpu, sims[0].energy) == E_STATE      # ... where energy refuses
                assert code_of(gpu, lambda: sims[0].set_option("potential", 0)) == E_STATE
            if before is not None:
                t_next, act = B.next_time(before["ticks"], before["levels"], kmax)
                qp, _ = B.predict_all(before["q"], before["v"], before["a"], before["j"], before["ticks"], t_next, dt_max, kmax)
                assert act.sum() == outs[0]["max_active"]
                partial += int(act.sum() < 256)
                want = PR.phi_f64(H._r32(qp), gm, B.SOFT, rows=np.flatnonzero(act))
                full = np.zeros(256)
                full[act] = want
                assert_phi(now["phi"], full, f"step {step} ({act.sum()} active)", rows=np.flatnonzero(act))
                assert np.array_equal(bits(now["phi"][~act]), bits(before["phi"][~act])), f"step {step}: an inactive body's phi changed"
            before = now
        assert partial >= 10 and opened >= 10, "the replay saw too few partial active sets"
    finally:
        for sim in sims:
            sim.close()


def test_block_run_is_bit_identical_with_and_without(gpu):
    """A full evolve_block run: state, (a, j), ticks, levels and counts do not depend on the option, under the same "block_units";
    at the synchronised end every phi belongs to the last block step, in which all bodies were active."""
    s, period = cluster(256)
    dt_max = float(np.float32(period / 2.0))
    got = []
    for p in (0, 1):
        with hermite_sim(gpu, s, B.SOFT, potential=p, block_units=64) as sim:
            out = sim.evolve_block(dt_max, blocks=2, eta=ETA, eta_start=ETA_START, kmax=12)
            st = sim.state()
            got.append((out, np.stack([st[k] for k in Q + V] + list(sim.acc()) + list(sim.jerk())), sim.block_state()))
            if p:
                phi, w = sim.potential(), sim.potential_energy()
    assert got[0][0] == got[1][0] and got[0][0]["synchronised"]
    assert np.array_equal(bits(got[0][1]), bits(got[1][1]))
    assert np.array_equal(got[0][2][0], got[1][2][0]) and np.array_equal(got[0][2][1], got[1][2][1])
    assert np.isfinite(phi).all() and (phi > 0).all() and w < 0.0


SHAPE_KMAX = 4
SHAPE_DT_MAX = np.float32(2.0 ** -6)      # one step of 2^-10 s: the sources' neighbours move by 1e-3 of their distances at most


@pytest.mark.parametrize("chunks", [1, 3])
def test_active_set_shapes(gpu, chunks):
    """One block step per active set of the sparse probe (levels set by hand), among them 1, 15, 16 and 17 bodies — the group
    cut of the active sweep — and bodies of one wave in different tiles: the active bodies' phi against the fp64 sum at the
    predicted state, the others' unchanged, with the sweep's j range in 1 and in 3 chunks."""
    s, soft, src = PR.sparse(velocities=True)
    n, gm = len(s["m"]), H._gm(s)
    sets = [a for a in active_sets(n) if len(a) in (1, 2, 15, 16, 17)] + [np.array([0, 512, 1024, 1536]), np.array([511, 512, 2047, 2048])]
    assert {1, 15, 16, 17} <= {len(a) for a in sets}
    with hermite_sim(gpu, s, soft) as sim:
        for act in sets:
            groups = (len(act) + 15) // 16
            sim.set_option("block_units", groups * chunks)
            sim.upload(s)
            sim.compute_acc_jerk()
            a0, j0, phi0 = np.stack(sim.acc()), np.stack(sim.jerk()), sim.potential()
            levels = np.zeros(n, np.int32)
            levels[act] = SHAPE_KMAX
            sim.set_block_levels(levels, SHAPE_KMAX)
            out = sim.evolve_block(float(SHAPE_DT_MAX), kmax=SHAPE_KMAX, max_steps=1)
            assert out["body_steps"] == len(act) and not out["synchronised"]
            phi1 = sim.potential()
            mask = np.zeros(n, bool)
            mask[act] = True
            qp, _ = B.predict_all(H._stack(s, Q), H._stack(s, V), a0, j0, np.zeros(n, np.int64), 1, SHAPE_DT_MAX, SHAPE_KMAX)
            full = np.zeros(n)
            full[act] = PR.phi_f64(H._r32(qp), gm, soft, rows=act)
            assert_phi(phi1, full, f"{chunks} chunks, active set of {len(act)} ({act[:4]}...)", rows=act)
            assert np.array_equal(bits(phi1[~mask]), bits(phi0[~mask])), f"active set of {len(act)}: an inactive body's phi changed"


# --------------------------------------------------------------------------------------------------------------------- 6. evolve
def test_evolve_is_bit_identical_with_and_without(gpu):
    """A short adaptive run: out5 and the state do not depend on the option; phi afterwards is finite and positive."""
    s, period = cluster(256)
    got = []
    for p in (0, 1):
        with hermite_sim(gpu, s, B.SOFT, potential=p) as sim:
            out = sim.evolve(period / 64.0, eta=ETA, eta_start=ETA_START, max_steps=40)
            st = sim.state()
            got.append((out, np.stack([st[k] for k in Q + V] + list(sim.acc()) + list(sim.jerk()))))
            if p:
                phi, w = sim.potential(), sim.potential_energy()
    assert got[0][0] == got[1][0] and got[0][0]["steps"] > 2
    assert np.array_equal(bits(got[0][1]), bits(got[1][1]))
    assert np.isfinite(phi).all() and (phi > 0).all() and np.isfinite(w) and w < 0.0


# ---------------------------------------------------------------------------------------------------------------------- 7. rules
def test_state_rules(gpu):
    s, soft = N.lattice(513)
    with gpu.Simulation(513, soft=soft) as sim:
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            assert code_of(gpu, lambda: sim.set_option("potential", 1)) == E_STATE
        sim.set_option("integrator", 2)
        for bad in (2, -1):
            assert code_of(gpu, lambda: sim.set_option("potential", bad)) == E_INVALID
        assert sim.info("potential") == 0
        for other, value in (("nearest", 1), ("contact", 1), ("contact", 2)):      # set first ...
            sim.set_option(other, value)
            assert code_of(gpu, lambda: sim.set_option("potential", 1)) == E_STATE
            sim.set_option("potential", 0)      # 0 is always accepted
            sim.set_option(other, 0)
        bytes0 = sim.info("device_bytes")
        sim.set_option("potential", 1)
        assert sim.info("potential") == 1
        for other, value in (("nearest", 1), ("contact", 1), ("contact", 2)):      # ... and set afterwards
            assert code_of(gpu, lambda: sim.set_option(other, value)) == E_STATE
        assert code_of(gpu, lambda: sim.set_option("integrator", 0)) == E_STATE      # it belongs to the Hermite sweeps
        assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.potential_energy) == E_STATE      # nothing uploaded
        sim.upload(s)
        assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.potential_energy) == E_STATE      # no evaluation yet
        sim.compute_acc_jerk()
        phi = sim.potential()
        assert sim.info("device_bytes") > bytes0      # the buffer is counted
        sim.upload(s)
        assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.potential_energy) == E_STATE      # the bodies changed
        sim.step(1.0)
        assert (sim.potential() > 0).all()      # a step keeps them
        sim.set_option("potential", 0)      # drops the remembered evaluation
        assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.jerk) == E_STATE
        sim.compute_acc_jerk()
        assert code_of(gpu, sim.potential) == E_STATE
        sim.set_option("potential", 1)
        assert code_of(gpu, sim.potential) == E_STATE and code_of(gpu, sim.jerk) == E_STATE
        sim.upload(s)
        sim.compute_acc_jerk()
        assert np.array_equal(bits(sim.potential()), bits(phi))      # bit-reproducible
        import ctypes as C
        assert gpu.lib().murbhip_download_potential(sim._h, None) == E_INVALID
        assert gpu.lib().murbhip_potential_energy(sim._h, None) == E_INVALID
    with gpu.Simulation(4096, soft=np.float32(2e8), devices=[0, 0], exchange="copy") as two:     # two shards on one device
        assert code_of(gpu, lambda: two.set_option("potential", 1)) == E_STATE


def test_switching_is_refused_while_a_block_is_open(gpu):
    s, period = cluster(256)
    dt_max = float(np.float32(period / 2.0))
    for p in (0, 1):
        with hermite_sim(gpu, s, B.SOFT, potential=p) as sim:
            out = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=12, max_steps=3)
            assert not out["synchronised"]
            assert code_of(gpu, lambda: sim.set_option("potential", 1 - p)) == E_STATE
            sim.set_option("potential", p)      # no switch: accepted, the block stays open
            rest = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=12)
            assert rest["synchronised"]
            sim.set_option("potential", 1 - p)


def test_plugin_end_to_end(gpu):
    """HostSim(potential=True) on hip+hermite+block, two iterations.  This checks that potential() is finite, positive and of
    length n at the synchronised boundary, NOT a comparison with an fp64 sum: the values belong to the predicted end state of the
    iteration's last block step, which the plugin does not hand out."""
    n, soft, dt = 1024, np.float32(2e8), np.float32(3600.0)
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=4, potential=True) as host:
        assert host.potential() is None      # no sweep yet
        host.step(2)
        phi = host.potential()
    assert phi is not None and phi.shape == (n,) and phi.dtype == np.float32
    assert np.isfinite(phi).all() and (phi > 0).all()
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=4) as plain:
        plain.step(1)
        assert plain.potential() is None
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=1) as leap:
        assert leap.H.murbhost_sim_set_potential(leap.h, 1) == -1 and leap.potential() is None


# ------------------------------------------------------------------------------- 8. phi and the company a body keeps in its wave
@lru_cache(maxsize=None)
def dense_system():
    return PR.dense()


@pytest.mark.parametrize("cut", ["one chunk", "one tile per chunk"])
def test_phi_does_not_depend_on_the_wave_mates(gpu, cut):
    """The active sweep's wave takes four bodies of the active list, whose order is unspecified: they can lie in four layout
    tiles.  A body's phi, like its (a1, j1), must not change by a bit with the bodies that share its wave (include/murbhip.h).
    Dense system, n = 2 049.  Reference bits: a block step of all 512 bodies of tile 0, where every wave has tile 0 as its only
    own tile.  Against them, for 64 bodies b of tile 0: a step of {b, one body each of tiles 1, 2, 3} — exactly one wave, four
    own tiles —, a step of b alone, and the step of all n bodies.  With one tile per chunk a partial sum holds one tile and no
    order can matter: the control."""
    s, soft = dense_system()
    n, gm = len(s["m"]), H._gm(s)
    probes = PR.dense_probes(64)
    with hermite_sim(gpu, s, soft) as sim:
        tiles = int(sim.info("slots")) // PR.TILE
        chunks = 1 if cut == "one chunk" else tiles

        def step(act):
            act = np.asarray(act, np.int64)
            sim.set_option("block_units", ((len(act) + 15) // 16) * chunks)
            sim.upload(s)
            sim.compute_acc_jerk()
            levels = np.zeros(n, np.int32)
            levels[act] = SHAPE_KMAX
            sim.set_block_levels(levels, SHAPE_KMAX)
            out = sim.evolve_block(float(SHAPE_DT_MAX), kmax=SHAPE_KMAX, max_steps=1)
            assert out["body_steps"] == len(act)
            return bits(sim.potential()), bits(np.stack(sim.acc() + sim.jerk()))

        sim.compute_acc_jerk()
        a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
        want_phi, want_aj = step(np.arange(PR.TILE))
        qp, _ = B.predict_all(H._stack(s, Q), H._stack(s, V), a0, j0, np.zeros(n, np.int64), 1, SHAPE_DT_MAX, SHAPE_KMAX)
        full = np.zeros(n)
        full[probes] = PR.phi_f64(H._r32(qp), gm, soft, rows=probes)
        assert_phi(want_phi.view(np.float32), full, f"{cut}: tile 0 active", rows=probes)
        all_phi, all_aj = step(np.arange(n))
        again_phi, again_aj = step(np.arange(n))
        assert np.array_equal(all_aj, again_aj), f"{cut}: (a1, j1) of two all-n steps differ"
        bad = {"four tiles": [], "alone": [], "all n": [int(b) for b in probes if all_phi[b] != want_phi[b]],
               "all n, run to run": np.flatnonzero(all_phi != again_phi).tolist()}
        assert np.array_equal(all_aj[:, probes], want_aj[:, probes]), f"{cut}: (a1, j1) differ between tile 0 and all n"
        for k, b in enumerate(probes):
            mates = [PR.TILE * t + (37 * k + 11 * t) % PR.TILE for t in (1, 2, 3)]
            for what, act in (("four tiles", [int(b)] + mates), ("alone", [int(b)])):
                phi, aj = step(act)
                assert np.array_equal(aj[:, b], want_aj[:, b]), f"{cut}: (a1, j1) of body {b} differ, {what}"
                if phi[b] != want_phi[b]:
                    bad[what].append(int(b))
        print(f"{cut} ({chunks} of {tiles} tiles): phi bits against the tile-0 step differ for "
              + ", ".join(f"{len(v)} of {n if 'run' in k else len(probes)} bodies ({k})" for k, v in bad.items()))
        assert not any(bad.values()), f"{cut}: phi depends on the bodies that share the wave: " + \
            ", ".join(f"{k}: {len(v)} bodies, first {v[:8]}" for k, v in bad.items() if v)

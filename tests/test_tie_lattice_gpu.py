"""GPU: the tie rule of the nearest-neighbour and contact sweeps ("lowest index among equal values"), the active sweeps'
refresh, and the hit lists beyond their cap, on the dense tie lattice.

Yardstick: tests/helpers/nearest_ref.py and contact_ref.py on dense_lattice (pinned by tests/test_nearest_host.py and
tests/test_contact_host.py): a full cubic grid in a random order, so that nearly every body has several candidates at the very
same fp32 value, in several layout tiles.  Every value is exact in fp32, so every comparison here is exact: indices equal,
values equal as bits, no tolerance anywhere.

The bodies move.  The lattice's velocities are k 2^30 with k = q2 - q, q2 the same points held by other bodies: one predictor
step of 2^-30 puts every body on q2 exactly (asserted from the device's own (a0, j0) before anything is compared), and the
sweep of that step sees a lattice whose winners differ in nearly every row.  A refresh that wrote nothing, or stale rows, shows."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import contact_ref as CR                 # noqa: E402
import hermite_block_ref as B            # noqa: E402
import hermite_ref as H                  # noqa: E402
import nearest_ref as N                  # noqa: E402
from active_sets import active_sets      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID = -2000
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
DT = 2.0 ** -30                 # the step that carries q to q2
BLOCK_KMAX = 2                  # the active bodies at level 2, the others at level 0 ...
BLOCK_DT_MAX = 2.0 ** -28       # ... so that the active bodies' step, and the block step, is DT
CAP = 4096                      # entries a hit list keeps


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@lru_cache(maxsize=None)
def lattice(n):
    """(state, soft, q, q2, radii) of the dense lattice: integer positions before and after the shift."""
    s, soft, q = N.dense_lattice(n)
    q2, _ = N.shifted(q)
    return s, soft, q, q2, CR.dense_radii(n)


@lru_cache(maxsize=None)
def reference(n, mode, moved, big=False):
    """(index, value) of the restatement on q (moved False) or q2, computed once.  big: every radius 8 (the hit-list test)."""
    s, soft, q, q2, radii = lattice(n)
    pos = q2 if moved else q
    if mode == "nearest":
        return N.nearest(pos, 0.25, exact=True)
    return CR.contact(pos, np.full(n, 8.0, np.float32) if big else radii, 0.25)


def make_sim(gpu, n, mode, on=1, radii=None, **opts):
    s, soft, q, q2, lattice_radii = lattice(n)
    sim = gpu.Simulation(n, soft=soft)
    sim.set_option("integrator", 2)
    sim.set_option(mode, on)
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.upload(s)
    if mode == "contact":
        sim.upload_radii(lattice_radii if radii is None else radii)
    return sim


def result(sim, mode):
    return sim.nearest() if mode == "nearest" else sim.contact()


def assert_rows(got, want, rows, what):
    """Indices equal and values equal as bits on `rows`; the message names the first rows that differ and where they lie."""
    rows = np.asarray(rows)
    bad = rows[(got[0][rows] != want[0][rows]) | (bits(got[1])[rows] != bits(want[1])[rows])]
    if len(bad):
        lines = [f"body {i} (tile {i // N.TILE}): got ({got[0][i]}, {got[1][i]!r}) in tile {got[0][i] // N.TILE}, want "
                 f"({want[0][i]}, {want[1][i]!r}) in tile {want[0][i] // N.TILE}" for i in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} rows differ\n  " + "\n  ".join(lines))


def state_of(n):
    s = lattice(n)[0]
    return np.stack([s[k] for k in Q]), np.stack([s[k] for k in V])


# ---------------------------------------------------------------------------------------------------------------- a. full sweeps
@pytest.mark.parametrize("jsplit", [0, 1, 3, 8, 32])
@pytest.mark.parametrize("mode", ["nearest", "contact"])
@pytest.mark.parametrize("n", [2049, 2561])
def test_full_sweeps(gpu, n, mode, jsplit):
    """murb_nn_sweep_kernel / murb_contact_sweep_kernel, 6 layout tiles (5 or 6 of them hold bodies, the last body alone in
    its tile) in 1, 3 or 6 chunks or the library's own cut: every row of the starting evaluation is the restatement's on q,
    every row after one step of 2^-30 is the restatement's on q2; the forces do not change with the option."""
    s, soft, q, q2, radii = lattice(n)
    everyone = np.arange(n)
    with make_sim(gpu, n, mode, on=0, jsplit=jsplit) as off:
        off.compute_acc_jerk()
        plain = np.stack(list(off.acc()) + list(off.jerk()))
    with make_sim(gpu, n, mode, jsplit=jsplit) as sim:
        parts = int(sim.info("hermite_parts"))
        sim.compute_acc_jerk()
        got = result(sim, mode)
        a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
        assert_rows(got, reference(n, mode, False), everyone, f"n={n} {mode} jsplit={jsplit} ({parts} chunks), starting evaluation")
        assert (got[1][got[0]] <= got[1]).all()
        assert np.array_equal(bits(np.concatenate([a0, j0])), bits(plain)), "the forces changed with the option"
        qs, vs = state_of(n)
        qp, _ = H.predict(qs, vs, a0, j0, DT)
        assert np.array_equal(bits(qp.astype(np.float32)), bits(q2.astype(np.float32))), "the predictor does not land on q2"
        sim.step(DT)
        moved = result(sim, mode)
        assert_rows(moved, reference(n, mode, True), everyone, f"n={n} {mode} jsplit={jsplit} ({parts} chunks), after the step")
        assert (moved[1][moved[0]] <= moved[1]).all()
        assert np.mean(moved[0] != got[0]) >= 0.9
    if jsplit == 3:      # the adaptive sweep's launch of the same kernel
        with make_sim(gpu, n, mode, jsplit=jsplit) as sim:
            out = sim.evolve(DT, dt_min=DT, dt_max=DT, max_steps=1)
            assert out["steps"] == 1 and out["time"] == DT and out["dt_min"] == out["dt_max"] == DT
            again = result(sim, mode)
        assert np.array_equal(again[0], moved[0]) and np.array_equal(bits(again[1]), bits(moved[1])), "evolve differs from step"


# -------------------------------------------------------------------------------------------------------------- b. active sweeps
def tie_sets(n):
    """active_sets(n) and three shapes of their own: one wave whose four bodies lie in four tiles, 16 bodies (four waves) of
    one tile, and the three bodies that share one point."""
    sets = active_sets(n) + [np.array([0, 512, 1024, 1536]), 1541 + 32 * np.arange(16), np.array(sorted(N.DENSE_TRIPLE))]
    assert len({int(b) // N.TILE for b in sets[-3]}) == 4 and len({int(b) // N.TILE for b in sets[-2]}) == 1
    return sets


_seen = {}      # (n, mode, set) -> the bits of the first chunk count that ran


@pytest.mark.parametrize("chunks", [1, 2, 4, 0])
@pytest.mark.parametrize("mode", ["nearest", "contact"])
@pytest.mark.parametrize("n", [2049, 2561])
def test_active_sweeps(gpu, n, mode, chunks):
    """murb_nn_active_sweep_kernel / murb_contact_active_sweep_kernel: one block step per active set with "block_units" forced
    to groups x chunks (tests/test_hermite_block_gpu.py), 6 layout tiles in 1, 2, 4 (1, 2, 1, 2 tiles) or 6 chunks.  All
    bodies are predicted onto q2; the active rows are the restatement's on q2, the inactive rows keep the bits of q."""
    s, soft, q, q2, radii = lattice(n)
    qs, vs = state_of(n)
    before, after = reference(n, mode, False), reference(n, mode, True)
    everyone = np.arange(n)
    with make_sim(gpu, n, mode) as sim:
        tiles = int(sim.info("slots")) // N.TILE
        want_chunks = chunks or tiles
        for k, act in enumerate(tie_sets(n)):
            what = f"n={n} {mode} chunks={want_chunks} of {tiles} tiles, active set {k} ({len(act)} bodies from {act[0]})"
            sim.set_option("block_units", ((len(act) + 15) // 16) * want_chunks)
            sim.upload(s)
            sim.compute_acc_jerk()
            assert_rows(result(sim, mode), before, everyone, what + ", starting evaluation")
            a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
            levels = np.zeros(n, np.int32)
            levels[act] = BLOCK_KMAX
            sim.set_block_levels(levels, BLOCK_KMAX)
            out = sim.evolve_block(BLOCK_DT_MAX, kmax=BLOCK_KMAX, max_steps=1)
            assert out["steps"] == 1 and out["body_steps"] == len(act) and out["dt_min"] == DT, (what, out)
            qp, _ = B.predict_all(qs, vs, a0, j0, np.zeros(n, np.uint32), 1, BLOCK_DT_MAX, BLOCK_KMAX)
            assert np.array_equal(bits(qp.astype(np.float32)), bits(q2.astype(np.float32))), what + ": the predictor does not land on q2"
            got = result(sim, mode)
            mask = np.zeros(n, bool)
            mask[act] = True
            assert_rows(got, after, everyone[mask], what + ", active rows")
            assert_rows(got, before, everyone[~mask], what + ", inactive rows")
            first = _seen.setdefault((n, mode, k), (got[0].copy(), bits(got[1]).copy(), want_chunks))
            assert np.array_equal(got[0], first[0]) and np.array_equal(bits(got[1]), first[1]), \
                what + f": the bits differ from those of {first[2]} chunks"


# ------------------------------------------------------------------------------------------------ c. the hit lists beyond their cap
def raw_list(gpu, sim, mode, i, j, v, capacity):
    """murbhip_encounters / murbhip_contacts through the C ABI: (return code, count, time)."""
    fn = gpu.lib().murbhip_encounters if mode == "nearest" else gpu.lib().murbhip_contacts
    count, time = C.c_ulong(), C.c_double()
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    ptr = [None if x is None else x.ctypes.data_as(t) for x, t in ((i, ip), (j, ip), (v, fp))]
    return fn(sim._h, ptr[0], ptr[1], ptr[2], capacity, C.byref(count), C.byref(time)), int(count.value), time.value


@pytest.mark.parametrize("how", ["evolve", "evolve_block"])
@pytest.mark.parametrize("mode", ["nearest", "contact"])
def test_hit_lists_beyond_the_cap(gpu, mode, how):
    """n = 4 609, every body a hit (an encounter radius far larger than the lattice; every radius 8 with "contact" 2): the count
    is n, 4 096 entries come back sorted, each with its body's own (partner, value).  Which 4 096 are kept is not specified."""
    n = 4609
    big = np.full(n, 8.0, np.float32)
    want = reference(n, mode, True, big=True)
    if mode == "contact":
        assert (want[1] <= 0).all()
    with make_sim(gpu, n, mode, on=1 if mode == "nearest" else 2, radii=big) as sim:
        if mode == "nearest":
            sim.set_encounter(1000.0)

        def run():
            if how == "evolve":
                return sim.evolve(DT, dt_min=DT, dt_max=DT, max_steps=1)
            return sim.evolve_block(BLOCK_DT_MAX, kmax=BLOCK_KMAX, max_steps=1)

        if how == "evolve_block":
            sim.set_block_levels(np.full(n, BLOCK_KMAX, np.int32), BLOCK_KMAX)
        out = run()
        assert out["steps"] == 1 and out["time"] == DT and (how == "evolve" or out["body_steps"] == n)
        hits = sim.encounters() if mode == "nearest" else sim.contacts()
        value = hits["r2" if mode == "nearest" else "gap2"]
        idx, val = result(sim, mode)
        assert_rows((idx, val), want, np.arange(n), f"{mode} {how}: the rows behind the hit list")
        assert hits["count"] == n == int(sim.info("encounter_count" if mode == "nearest" else "contact_count"))
        assert int(sim.info("contact_count" if mode == "nearest" else "encounter_count")) == 0
        assert len(hits["i"]) == CAP and (np.diff(hits["i"]) > 0).all() and hits["i"][0] >= 0 and hits["i"][-1] < n
        assert np.array_equal(hits["j"], idx[hits["i"]]) and np.array_equal(bits(value), bits(val[hits["i"]]))
        assert hits["time"] == out["time"]
        # the raw calls: a capacity below the 4 096 kept is refused, NULL arrays ask for the count alone
        i, j, v = np.zeros(CAP, np.int32), np.zeros(CAP, np.int32), np.zeros(CAP, np.float32)
        assert raw_list(gpu, sim, mode, i, j, v, CAP - 1)[0] == E_INVALID
        assert raw_list(gpu, sim, mode, None, None, None, 0) == (0, n, out["time"])
        assert raw_list(gpu, sim, mode, i, j, v, CAP) == (0, n, out["time"])
        assert np.array_equal(i, hits["i"]) and np.array_equal(j, hits["j"]) and np.array_equal(bits(v), bits(value))
        other = gpu.lib().murbhip_contacts if mode == "nearest" else gpu.lib().murbhip_encounters
        count, time = C.c_ulong(99), C.c_double()
        assert other(sim._h, None, None, None, 0, C.byref(count), C.byref(time)) == 0 and count.value == 0
        # the stop off: the next call clears the list
        if mode == "nearest":
            sim.set_encounter(0.0)
        else:
            sim.set_option("contact", 1)
        run()
        assert (sim.encounters() if mode == "nearest" else sim.contacts())["count"] == 0
        assert raw_list(gpu, sim, mode, None, None, None, 0)[:2] == (0, 0)

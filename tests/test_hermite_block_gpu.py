"""GPU: individual block time steps of the Hermite integrator (murbhip_evolve_block, `--im hip+hermite+block`) through the C ABI.

Yardsticks: tests/helpers/hermite_block_ref.py (numpy, written from include/murbhip.h, pinned by
tests/test_hermite_block_host.py) for the active sets, ticks, levels and counts; hermite_ref.correct for the state update,
bit for bit, from the device's own (a0, j0, a1, j1); hermite_ref's fp64 formulas at the restated prediction for the sweep's
(a1, j1), within the bounds of tests/test_hermite_gpu.py; the fixed-step path of the same library for kmax = 0."""
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_adaptive_ref as A   # noqa: E402
import hermite_block_ref as B      # noqa: E402
import hermite_probe as P          # noqa: E402
import hermite_ref as H            # noqa: E402
from active_sets import active_sets   # noqa: E402

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
E_INVALID, E_STATE = -2000, -2001
TOL_F64_MAX, JERK_MARGIN = 2e-6, 4.0      # tests/test_hermite_gpu.py
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
ETA, ETA_START = 0.02, 0.01


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hermite_sim(gpu, s, soft=SOFT, **opts):
    sim = gpu.Simulation(len(s["qx"]), soft=soft)
    sim.set_option("integrator", 2)
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.upload(s)
    return sim


class Snapshot:
    """q, v, a, j (3, n each, fp32) and ticks, levels of a context: every body at its own time."""

    def __init__(self, sim):
        st = sim.state()
        self.q, self.v = np.stack([st[k] for k in Q]), np.stack([st[k] for k in V])
        self.a, self.j = np.stack(sim.acc()), np.stack(sim.jerk())
        self.ticks, self.levels = sim.block_state()

    def arrays(self):
        return {"q": self.q, "v": self.v, "a": self.a, "j": self.j, "ticks": self.ticks, "levels": self.levels}


def assert_same(got, want, what=""):
    for k, w in want.arrays().items():
        g = got.arrays()[k]
        same = np.array_equal(bits(g), bits(w)) if w.dtype == np.float32 else np.array_equal(g, w)
        assert same, f"{what}: {k} differs"


@lru_cache(maxsize=None)
def cluster(n):
    return B.cluster(n)


# ---------------------------------------------------------------------------------------------------------------- 1. error codes
def test_error_codes(gpu):
    s, period = cluster(32)
    dt_max = float(np.float32(period / 2.0))
    with hermite_sim(gpu, s, B.SOFT) as sim:
        for kw in (dict(dt_max=0.0), dict(dt_max=-1.0), dict(dt_max=float("inf")), dict(dt_max=float("nan")), dict(blocks=0),
                   dict(eta=0.0), dict(eta_start=0.0), dict(eta=-1.0), dict(kmax=-1), dict(kmax=21), dict(max_steps=0),
                   dict(dt_max=1e-36, kmax=10)):      # 1e-36 2^-10 is no normal fp32 number
            args = dict(dt_max=dt_max)
            args.update(kw)
            with pytest.raises(gpu.MurbHipError) as e:
                sim.evolve_block(**args)
            assert e.value.code == E_INVALID, kw
        with pytest.raises(gpu.MurbHipError) as e:
            sim.set_block_levels(np.full(32, 5), 4)
        assert e.value.code == E_INVALID
        with pytest.raises(gpu.MurbHipError) as e:
            sim.set_block_levels(np.full(32, -1), 4)
        assert e.value.code == E_INVALID
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            with pytest.raises(gpu.MurbHipError) as e:
                sim.evolve_block(dt_max)
            assert e.value.code == E_STATE
        sim.set_option("integrator", 2)
        assert np.array_equal(bits(sim.state()["qx"]), bits(s["qx"]))     # none of them moved anything

        # a max_steps stop inside a block leaves it open
        out = sim.evolve_block(dt_max, max_steps=1)
        assert out["steps"] == 1 and not out["synchronised"] and 0.0 < out["time"] < dt_max
        for call in (lambda: sim.step(DT), lambda: sim.steps(DT, 2), lambda: sim.evolve(1000.0), sim.compute_acc,
                     sim.compute_acc_jerk, sim.energy, sim.moments, lambda: sim.warmup(1.0),
                     lambda: sim.set_block_levels(np.zeros(32), 12), lambda: sim.evolve_block(dt_max, kmax=11),
                     lambda: sim.evolve_block(dt_max * 2.0)):
            with pytest.raises(gpu.MurbHipError) as e:
                call()
            assert e.value.code == E_STATE
        snap = Snapshot(sim)     # the downloads work: every body at its own time
        assert snap.ticks.max() > 0 and (snap.ticks == 0).any() and np.isfinite(snap.j).all()
        more = sim.evolve_block(dt_max, max_steps=1)     # ... and so does going on with the same grid
        assert more["steps"] == 1 and not more["synchronised"]
        sim.upload(s)     # closes the block and drops the levels
        sim.step(DT)
        sim.compute_acc_jerk()
        assert sum(sim.energy()) < 0.0
        out = sim.evolve_block(dt_max)
        assert out["synchronised"] and out["time"] == dt_max
        sim.step(DT)      # after a synchronised return everything is allowed again
        sim.evolve(1000.0)
    with gpu.Simulation(4096, soft=SOFT, devices=[0, 0], exchange="copy") as two:     # two shards on one device
        two.upload(gpu.init_bodies(4096, "galaxy"))
        with pytest.raises(gpu.MurbHipError) as e:
            two.evolve_block(3600.0)
        assert e.value.code == E_STATE


# ------------------------------------------------------------------------------------------------------- 2. single-step replay
@lru_cache(maxsize=None)
def jerk_bound(name):
    """C of tests/test_hermite_gpu.py's jerk bound (units of 2^-24) for a system: 4 x what a numpy float32 evaluation attains
    against fp64, over all bodies of the INITIAL state — the block steps replayed below advance it by little more than one
    dt_max, the same bodies on the same orbits, so that one CPU evaluation serves every step."""
    s, soft = replay_system(name)[:2]
    _, j, abs_j = H.acc_jerk_f64(s, np.float32(soft), want_abs=True)
    _, j32 = H.acc_jerk_f32(s, np.float32(soft))
    return JERK_MARGIN * float(H.scaled_err(j32, j, abs_j).max()) * 2.0 ** 24


@lru_cache(maxsize=None)
def replay_system(name):
    """(state, softening, dt_max, kmax).  random: 2 049 bodies, blocks of 2^17 s in 64 ticks — the starting rule spreads the
    bodies over levels 0 ... 6 and the first 44 block steps have active sets of 1 ... 2 049 bodies (restatement, CPU).
    cluster: the specification's 256 bodies, blocks of half a binary period in 4 096 ticks — the binary starts at level 12 and
    the field bodies at levels 0 ... 2, so that the binary alone is active for the first 99 block steps; the field's levels
    come up (44, 20, 110, 68 bodies) from there to the block's end at the 128th, where all 256 are (restatement, CPU).
    wrap: 5 120 bodies of the same generator, blocks of 8 ticks of 3 600 s, levels set by hand (replay_levels) and one chunk per
    layout tile (replay_options): the system tests/test_block_wrap_gpu.py replays, whose steps walk more units than the grid."""
    import murbhip
    if name == "random":
        return murbhip.init_bodies(2049, "random"), float(SOFT), 2.0 ** 17, 6
    if name == "wrap":      # tests/test_block_wrap_gpu.py: 10 layout tiles, blocks of 8 ticks of 3 600 s, levels by hand
        return murbhip.init_bodies(5120, "random"), float(SOFT), 8.0 * float(DT), 3
    s, period = cluster(256)
    return s, B.SOFT, float(np.float32(period / 2.0)), 12


def replay_levels(name):
    """The levels a replay starts from where they are set by hand (set_block_levels), None where the starting rule gives them.
    wrap: i mod 4 with kmax 3, so that the first active sets hold about 1 280, 2 560, 1 280, 3 840 ... 5 120 bodies."""
    return (np.arange(5120) % 4).astype(np.int32) if name == "wrap" else None


def replay_options(name):
    return {"block_units": 65536} if name == "wrap" else {}      # wrap: one chunk per layout tile in every step


@pytest.mark.parametrize("name,steps", [("random", 44), ("cluster", 136)])
def test_single_step_replay(gpu, O, name, steps):
    sizes, _ = replay(gpu, O, name, steps)
    assert steps >= 40 and len(sizes) == steps and min(sizes) < 16 < max(sizes)


def replay(gpu, O, name, steps):
    """`steps` block steps of replay_system(name), one per call, or fewer where a synchronised boundary comes first and the
    levels were set by hand.  Returns (the restatement's active-set sizes, the device's body-steps) per step."""
    s, soft, dt_max, kmax = replay_system(name)
    hand = replay_levels(name)
    n, gm, c_jerk = len(s["m"]), H._gm(s), jerk_bound(name)
    T = 1 << kmax
    worst_a = worst_j = 0.0
    sizes, body_steps = [], []
    with hermite_sim(gpu, s, soft, **replay_options(name)) as sim:
        sim.compute_acc_jerk()
        a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
        want_start = B.start_levels(a0, j0, ETA_START, dt_max, kmax) if hand is None else hand
        if hand is not None:
            sim.set_block_levels(hand, kmax)
        pre = None
        for k in range(steps):
            out = sim.evolve_block(dt_max, blocks=1000, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=1)
            post = Snapshot(sim)
            if pre is None:     # what the first call started from: the state as uploaded, the starting rule's levels
                pre = Snapshot.__new__(Snapshot)
                pre.q, pre.v = np.stack([s[f] for f in Q]), np.stack([s[f] for f in V])
                pre.a, pre.j, pre.ticks, pre.levels = a0, j0, np.zeros(n, np.uint32), want_start
            t_next, act = B.next_time(pre.ticks, pre.levels, kmax)
            idx = np.flatnonzero(act)
            sizes.append(len(idx))
            body_steps.append(out["body_steps"])
            # the active set is exactly the argmin set: its size, and nobody else moved in any array, bit for bit
            assert out["steps"] == 1 and out["body_steps"] == len(idx) == out["max_active"], (k, out, len(idx))
            assert out["synchronised"] == (t_next == T)
            for key, w in pre.arrays().items():
                g = post.arrays()[key]
                g, w = (g[..., ~act], w[..., ~act])
                assert np.array_equal(bits(g), bits(w)) if w.dtype == np.float32 else np.array_equal(g, w), (k, key)
            # ticks and levels of the active bodies: the restatement's from the device's own evaluations
            want_levels, clamped = B.levels_after(pre.a, pre.j, post.a, post.j, pre.levels, act, t_next, ETA, dt_max, kmax)
            assert np.array_equal(post.levels, want_levels), (k, np.flatnonzero(post.levels != want_levels)[:8])
            assert (post.ticks[act] == (0 if t_next == T else t_next)).all() and out["clamped"] == clamped
            used = pre.levels[act]
            assert out["dt_min"] == float(B.level_dt(dt_max, used.max())) and out["dt_max"] == float(B.level_dt(dt_max, used.min()))
            assert out["time"] == (t_next - int(pre.ticks.max())) * B.tick_seconds(dt_max, kmax)
            # active q, v: hermite_ref.correct on the device's own (a0, j0, a1, j1) with the body's own dt_i, bit for bit
            for lv in np.unique(used):
                sel = act & (pre.levels == lv)
                q1, v1 = H.correct(pre.q[:, sel], pre.v[:, sel], pre.a[:, sel], pre.j[:, sel], post.a[:, sel], post.j[:, sel],
                                   B.level_dt(dt_max, lv), True)
                assert np.array_equal(bits(post.v[:, sel]), bits(v1)), (k, "v", int(lv))
                assert np.array_equal(bits(post.q[:, sel]), bits(q1)), (k, "q", int(lv))
            # active (a1, j1) against fp64 at the restatement's prediction (at most 256 of them a step: the cost is the CPU's)
            qp, vp = B.predict_all(pre.q, pre.v, pre.a, pre.j, pre.ticks, t_next, dt_max, kmax)
            rows = idx[np.unique(np.linspace(0, len(idx) - 1, min(len(idx), 256)).astype(np.int64))]
            ta, tj, abs_j = B.evaluate_rows(H._r32(qp), H._r32(vp), gm, rows, soft)
            worst_a = max(worst_a, float(O.rel_err(post.a[:, rows], ta).max()))
            worst_j = max(worst_j, float(H.scaled_err(post.j[:, rows], tj, abs_j).max()) * 2.0 ** 24)
            pre = post
            if hand is not None and out["synchronised"]:
                break
    print(f"{name}: {len(sizes)} block steps, active sets {sizes}; acc max rel {worst_a:.3e} (bound {TOL_F64_MAX:.1e}); "
          f"jerk max scaled {worst_j:.2f} x 2^-24 (bound C = {c_jerk:.2f})")
    assert worst_a <= TOL_F64_MAX and worst_j <= c_jerk
    return sizes, body_steps


# ------------------------------------------------------------------------------------------------------- 3. active-set shapes
SHAPE_KMAX = 2                         # the active bodies at level 2 (steps of one tick), the others at level 0
SHAPE_DT_MAX = np.float32(4.0) * DT    # ... so that the step is DT for the active ones


@lru_cache(maxsize=None)
def shape_probe(n):
    """(probe state, sources): masses on at most 256 bodies (oracle.probe_sources' choice, the first probe), so that a missed or
    doubled range of j shows in every active body's sums."""
    import murbhip
    import oracle
    first, count = murbhip.partition(n, 1, 0)
    src = [x for x in oracle.probe_sources(n, [first], [count], murbhip.slice_slots(n, 1), probes=1, k_max=256, per_block=8) if len(x)][0]
    return oracle.probe_state(oracle.init_bodies(n, "random"), src, seed=n, zero_velocities=False), src


_shape_truth = {}


def shape_truth(n, a0, j0):
    """The probe's truth at the restated prediction of one step of DT from the device's (a0, j0): computed once per size."""
    if n not in _shape_truth:
        ps, src = shape_probe(n)
        _shape_truth[n] = (bits(np.stack(a0)).copy(), P.Truth(P.predicted(ps, a0, j0, DT), src, SOFT))
    seen, truth = _shape_truth[n]
    assert np.array_equal(seen, bits(np.stack(a0))), "the device's (a0, j0) of one probe differ from run to run"
    return truth


@pytest.mark.parametrize("chunks", [1, 2, 4, 0])
@pytest.mark.parametrize("n", [2049, 2561])
def test_active_set_shapes(gpu, n, chunks):
    """One block step per active set, with "block_units" forced to groups x chunks so that the sweep's j range is cut into
    1, 2, 4 chunks or one per tile (chunks = 0).  Both sizes have 6 layout tiles (slots come in multiples of 1 024): 4 chunks
    cut them unevenly (1, 2, 1, 2 tiles)."""
    ps, src = shape_probe(n)
    lines = []
    with hermite_sim(gpu, ps) as sim:
        tiles = int(sim.info("slots")) // P.TILE
        want_chunks = chunks or tiles
        for act in active_sets(n):
            groups = (len(act) + 15) // 16
            sim.set_option("block_units", groups * want_chunks)
            sim.upload(ps)
            sim.compute_acc_jerk()
            a0, j0 = sim.acc(), sim.jerk()
            truth = shape_truth(n, a0, j0)
            levels = np.zeros(n, np.int32)
            levels[act] = SHAPE_KMAX
            if len(act) == n:
                levels[:] = SHAPE_KMAX
            sim.set_block_levels(levels, SHAPE_KMAX)
            out = sim.evolve_block(float(SHAPE_DT_MAX), kmax=SHAPE_KMAX, max_steps=1)
            assert out["body_steps"] == len(act) and out["dt_min"] == out["dt_max"] == float(DT), (len(act), out)
            a1, j1 = np.stack(sim.acc()), np.stack(sim.jerk())
            ticks, _ = sim.block_state()
            mask = np.zeros(n, bool)
            mask[act] = True
            assert (ticks[mask] == 1).all() and (ticks[~mask] == 0).all()
            assert np.array_equal(bits(a1[:, ~mask]), bits(np.stack(a0)[:, ~mask])) and np.array_equal(bits(j1[:, ~mask]), bits(np.stack(j0)[:, ~mask]))
            ea = P.probe_err(a1[:, act], truth.a[:, act], truth.abs_a[act])
            ej = H.scaled_err(j1[:, act], truth.j[:, act], truth.abs_j[act]) * 2.0 ** 24
            wa, wj = int(np.argmax(ea)), int(np.argmax(ej))
            lines.append(f"{len(act)}: {ea[wa]:.1e} / {ej[wj]:.2f}")
            assert ea[wa] <= P.TOL_F64_MAX, f"n={n} chunks={want_chunks} active={len(act)}: acceleration of {P.where(act[wa])} off by {ea[wa]:.3e}"
            assert ej[wj] <= truth.c, f"n={n} chunks={want_chunks} active={len(act)}: jerk of {P.where(act[wj])} off by {ej[wj]:.2f} x 2^-24, bound {truth.c:.2f}"
    print(f"n={n}, {want_chunks} chunks of {tiles} tiles; active bodies: acc of the source terms / jerk x 2^-24 (bounds "
          f"{P.TOL_F64_MAX:.0e} / {truth.c:.2f}): " + "; ".join(lines))


# --------------------------------------------------------------------------------------------------------------- 4. split runs
def test_split_runs_and_batches(gpu):
    """4 blocks in one call == 2 + 2 == step by step == any batch length, bit for bit in state, a, j, ticks and levels; two
    identical runs give identical bits, whatever order the active lists came in."""
    s, period = cluster(256)
    dt_max = float(np.float32(period / 2.0))

    def run(how, **opts):
        with hermite_sim(gpu, s, B.SOFT, **opts) as sim:
            counts = how(sim)
            return Snapshot(sim), counts

    def whole(sim):
        out = sim.evolve_block(dt_max, blocks=4)
        assert out["synchronised"] and out["time"] == 4.0 * dt_max and out["clamped"] == 0
        return out["steps"], out["body_steps"]

    def halves(sim):
        a, b = sim.evolve_block(dt_max, blocks=2), sim.evolve_block(dt_max, blocks=2)
        assert a["synchronised"] and b["synchronised"]
        return a["steps"] + b["steps"], a["body_steps"] + b["body_steps"]

    def one_by_one(sim):
        steps = bodies = done = 0
        while done < 4:
            out = sim.evolve_block(dt_max, blocks=4 - done, max_steps=1)
            steps, bodies, done = steps + out["steps"], bodies + out["body_steps"], done + int(out["synchronised"])
        return steps, bodies

    want, counts = run(whole)
    print(f"4 blocks: {counts[0]} block steps, {counts[1]} body-steps")
    assert_same(run(whole)[0], want, "second identical run")
    for how, opts in ((halves, {}), (one_by_one, {}), (whole, {"evolve_batch": 1}), (whole, {"evolve_batch": 3}),
                      (whole, {"evolve_batch": 64})):
        got, c = run(how, **opts)
        assert c == counts, (how.__name__, opts)
        assert_same(got, want, f"{how.__name__} {opts}")


# ------------------------------------------------------------------------------------------------------------------ 5. kmax = 0
def test_kmax_zero_is_the_fixed_step(gpu):
    """kmax = 0: every body at level 0, a block step is a Hermite step of all bodies.  The state after 3 blocks against
    murbhip_steps(dt_max, 3): the two differ only by the chunk cut of the fp32 row sums, so the bound is 4 x the largest
    relative difference that murbhip_steps itself shows between "jsplit" 1 and 8 on the same input, per component of the
    state (max |x - y| over the bodies / max |y|), measured here."""
    n = 2049
    s = gpu.init_bodies(n, "random")

    def fixed(jsplit):
        with hermite_sim(gpu, s, jsplit=jsplit) as sim:
            sim.steps(DT, 3)
            return sim.state()

    def rel(x, y):
        return {k: float(np.abs(x[k].astype(np.float64) - y[k]).max() / np.abs(y[k].astype(np.float64)).max()) for k in Q + V}

    f1, f8 = fixed(1), fixed(8)
    yard = rel(f1, f8)
    with hermite_sim(gpu, s) as sim:
        out = sim.evolve_block(float(DT), blocks=3, kmax=0)
        got = sim.state()
        ticks, levels = sim.block_state()
    assert out["steps"] == 3 and out["body_steps"] == 3 * n and out["synchronised"] and out["time"] == 3.0 * float(DT)
    assert out["dt_min"] == out["dt_max"] == float(DT) and out["max_active"] == n
    assert (levels == 0).all() and (ticks == 0).all()
    diff = rel(got, f8)
    bound = 4.0 * max(yard.values())
    print("jsplit 1 against 8:", {k: f"{v:.2e}" for k, v in yard.items()}, "-> bound", f"{bound:.2e};",
          "block against jsplit 8:", {k: f"{v:.2e}" for k, v in diff.items()})
    assert max(yard.values()) > 0.0
    assert max(diff.values()) <= bound


# ------------------------------------------------------------------------------------------------------ 6. physics on the device
def test_cluster_on_the_device(gpu):
    """The n = 256 system of tests/test_hermite_block_host.py, 4 blocks, kmax 12: block steps and body-steps equal the
    restatement's, nothing is clamped, and the energy error read with murbhip_energy at the synchronised end is within 2 x
    the restatement's (the factor is for the fp32 sweep)."""
    s, period = cluster(256)
    dt_max = float(np.float32(period / 2.0))
    e0_ref = A.energy(s, B.SOFT)
    ref = B.Run(s, B.SOFT, dt_max, kmax=12, eta=ETA, eta_start=ETA_START).run(4)
    ref_err = abs(A.energy(ref.state(), B.SOFT) - e0_ref) / abs(e0_ref)
    with hermite_sim(gpu, s, B.SOFT) as sim:
        e0 = sum(sim.energy())
        out = sim.evolve_block(dt_max, blocks=4, eta=ETA, eta_start=ETA_START, kmax=12)
        e1 = sum(sim.energy())
        end = dict(sim.state(), m=s["m"])
    err = abs(e1 - e0) / abs(e0)
    err64 = abs(A.energy(end, B.SOFT) - e0_ref) / abs(e0_ref)
    print(f"device: {out['steps']} block steps, {out['body_steps']} body-steps, dt {out['dt_min']:.4g} ... {out['dt_max']:.4g} s, "
          f"{out['clamped']} clamped, relative energy error {err:.3e} (murbhip_energy; {err64:.3e} from the downloaded state in "
          f"fp64); restatement: {ref.steps} block steps, {ref.body_steps} body-steps, {ref_err:.3e}")
    assert out["synchronised"] and out["time"] == 4.0 * dt_max and out["clamped"] == 0
    assert out["steps"] == ref.steps and out["body_steps"] == ref.body_steps
    assert err <= 2.0 * ref_err


# ------------------------------------------------------------------------------------------------------------- 7. upper layers
def test_plugin_matches_the_c_abi(gpu):
    """HostSim(integrator=4): five iterations are five evolve_block(dt, blocks=1) calls, bit for bit; one history row each."""
    n, iters, kmax = 2048, 5, 6
    with gpu.HostSim(n, "galaxy", SOFT, DT, tracking=True, integrator=4, eta=ETA, kmax=kmax) as sim:
        sim.step(iters)
        got, hist, sub, counts = sim.state(), sim.history(), sim.substeps(), sim.block_counts()
    assert len(hist["energy"]) == iters
    s = gpu.init_bodies(n, "galaxy")
    steps = bodies = clamped = 0
    lo, hi = np.inf, 0.0
    with hermite_sim(gpu, s) as ref:
        for _ in range(iters):
            out = ref.evolve_block(float(DT), blocks=1, eta=ETA, eta_start=ETA_START, kmax=kmax)
            assert out["synchronised"]
            steps, bodies, clamped = steps + out["steps"], bodies + out["body_steps"], clamped + out["clamped"]
            lo, hi = min(lo, out["dt_min"]), max(hi, out["dt_max"])
        want = ref.state()
    for k in Q + V:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert sub == (float(steps), lo, hi) and counts == (steps, bodies, clamped) and steps >= iters
    with gpu.HostSim(n, "galaxy", SOFT, DT, tracking=True, integrator=3) as shared:
        assert shared.block_counts() is None


def test_murb_hip_cli_block(gpu, tmp_path):
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    csv = tmp_path / "m.csv"
    r = subprocess.run([exe, "-n", "2048", "-i", "5", "--nv", "--im", "hip+hermite+block", "--eta", "0.01", "--kmax", "8", "--gf",
                        "--csv", str(csv)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "  -> implementation    (--im  ): hip+hermite+block" in r.stdout
    m = re.search(r"Block steps: (\d+) block steps, (\d+) body-steps, dt from ([0-9.e+]+) to ([0-9.e+]+) sec, (\d+) clamped "
                  r"\(eta 0\.01, kmax 8\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 5 and int(m.group(2)) >= 5 * 2048 and 0.0 < float(m.group(3)) <= float(m.group(4)) <= 3600.0
    assert len(csv.read_text().splitlines()) == 6
    bad = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", "hip+hermite+block", "--kmax", "21"], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode != 0 and "--kmax" in bad.stdout
    h = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert "hip+hermite+block" in h.stdout + h.stderr and "--kmax" in h.stdout + h.stderr

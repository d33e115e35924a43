"""GPU: the active sweep of a block step (murb_force_jerk_block_sweep: plain, nearest, contact and potential form) beyond one
pass of its fixed grid.  A workgroup walks units u = blockIdx.x, += grid; everything that is made again inside that loop (the
control block, the thread's index, the stride of the three option forms, the LDS tiles behind the stage's barrier) matters
from a workgroup's second unit on, and no other file has enough units for one: tests/helpers/block_wrap.py lists the shapes,
tests/test_hermite_block_host.py pins their arithmetic (rows written against rows allocated, passes on 256 CUs).

Yardsticks: hermite_ref's fp64 formulas at the restated prediction for (a1, j1) within the project's bounds; potential_ref's
fp64 phi; nearest_ref / contact_ref on the dense tie lattice, exact; and bits against bits: across the four forms (their grids
differ, 5 against 4 workgroups per CU, so a wrong stride shows), across pass depth (a body's sums in the all-n step against a
step of a few groups that ends in the first pass), and from run to run.

Rows are not cleared between steps.  Before every measured step the same context takes the same step on a state whose
positions are doubled (accelerations about 4 times smaller, lattice values 4 times larger): a unit left out leaves those."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_wrap as W             # noqa: E402
import contact_ref as CR           # noqa: E402
import hermite_block_ref as B      # noqa: E402
import hermite_ref as H            # noqa: E402
import nearest_ref as N            # noqa: E402
import potential_ref as PR         # noqa: E402
import test_hermite_block_gpu as T   # noqa: E402  (Snapshot, assert_same, the replay)

pytestmark = pytest.mark.gpu

SOFT, DT = T.SOFT, T.DT
KMAX, DT_MAX = T.SHAPE_KMAX, T.SHAPE_DT_MAX      # the active bodies at level 2 take one tick = DT, the others rest at level 0
TOL_F64_MAX, JERK_MARGIN = T.TOL_F64_MAX, T.JERK_MARGIN
Q, V = T.Q, T.V
bits = T.bits
OPTION = {"plain": None, "potential": "potential", "nearest": "nearest", "contact0": "contact", "contact": "contact"}
CASES = [(n, c) for n, cs in W.CUTS.items() for c in cs] + [(W.MAIN, "tight")]


def doubled(s):
    return {k: (np.float32(2.0) * v if k in Q else v.copy()) for k, v in s.items()}


def open_sim(gpu, s, soft, form, radii=None):
    sim = gpu.Simulation(len(s["m"]), soft=soft)
    sim.set_option("integrator", 2)
    if OPTION[form]:
        sim.set_option(OPTION[form], 1)
    sim.upload(s)
    if OPTION[form] == "contact":
        sim.upload_radii(np.zeros(len(s["m"]), np.float32) if radii is None else radii)
    return sim


def grid_of(sim, form):
    grid = int(sim.info("block_grid"))
    return grid if form == "plain" else grid // 5 * 4


def side_result(sim, form):
    if form == "potential":
        return (bits(sim.potential()),)
    if form == "plain":
        return ()
    idx, val = sim.nearest() if form == "nearest" else sim.contact()
    return (idx, bits(val))


def block_step(sim, form, s, stale, act, units, dt_max, kmax):
    """One block step of the bodies `act` from the state s, behind the same step from `stale` on the same rows.
    Returns (out8, (a0, j0), side result before, Snapshot after, side result after)."""
    n = len(s["m"])
    sim.set_option("block_units", units)
    levels = np.zeros(n, np.int32)
    levels[act] = kmax
    for state in (stale, s):
        sim.upload(state)
        sim.compute_acc_jerk()
        start = (np.stack(sim.acc()), np.stack(sim.jerk()))
        before = side_result(sim, form)
        sim.set_block_levels(levels, kmax)
        out = sim.evolve_block(float(dt_max), kmax=kmax, max_steps=1)
        assert out["steps"] == 1 and out["body_steps"] == len(act) == out["max_active"], (form, len(act), out)
    return out, start, before, T.Snapshot(sim), side_result(sim, form)


def check_untouched(s, act, start, before, post, after, kmax, what):
    """Inactive rows keep every bit; the active bodies' ticks and levels say that they stepped."""
    n = len(s["m"])
    mask = np.zeros(n, bool)
    mask[act] = True
    assert (post.ticks[~mask] == 0).all() and (post.ticks[mask] == 1).all(), what + ": ticks"
    rest = ~mask
    assert np.array_equal(bits(post.a[:, rest]), bits(start[0][:, rest])) and np.array_equal(bits(post.j[:, rest]), bits(start[1][:, rest])), \
        what + ": an inactive body's (a, j) changed"
    assert np.array_equal(bits(post.q[:, rest]), bits(H._stack(s, Q, np.float32)[:, rest])) and \
        np.array_equal(bits(post.v[:, rest]), bits(H._stack(s, V, np.float32)[:, rest])), what + ": an inactive body moved"
    for b, x in zip(before, after):
        assert np.array_equal(x[rest], b[rest]), what + ": an inactive body's neighbour / phi row changed"
    return mask


# ------------------------------------------------------------------------------------------------------------- 0. pass counts
def test_pass_counts(gpu):
    """The device's own grid: units and passes of every case's all-n step, and the largest case of the main size makes at
    least 3 passes in every form, so that this file cannot go blind on another chip."""
    with gpu.Simulation(W.MAIN, soft=SOFT) as sim:
        sim.set_option("integrator", 2)
        plain, option, tiles = grid_of(sim, "plain"), grid_of(sim, "nearest"), int(sim.info("slots")) // W.TILE
    assert tiles == W.slots_of(W.MAIN) // W.TILE == 10
    worst = None
    for n, c in CASES:
        t = W.slots_of(n) // W.TILE
        groups, chunks, units = W.plan(n, W.units_of(n, c)(-(-n // W.GROUP)), t)
        print(f"n={n} cut {c}: {groups} groups x {chunks} chunks {W.cut(t, chunks)} = {units} units; {W.passes(units, plain)} passes "
              f"of {plain} workgroups (plain), {W.passes(units, option)} of {option} (nearest, contact, potential)")
        if n == W.MAIN:
            worst = max(worst or 0, units)
    assert W.passes(worst, plain) >= 3 and W.passes(worst, option) >= 3, (worst, plain, option)


# -------------------------------------------------------------------------------------------------- 1. random system, all forms
@lru_cache(maxsize=None)
def random_system(n):
    import oracle
    s = oracle.init_bodies(n, "random")
    assert (s["m"] > 0).all() and min(np.abs(s[k]).max() for k in V) > 0.0      # dense, all massive, moving
    return s, doubled(s)


_truth = {}


def truth(n, start):
    """fp64 (a, j, sum |jerk terms|) of the rows W.fp64_rows at the restated prediction of one step of DT from the device's
    (a0, j0); the jerk bound C = JERK_MARGIN x what numpy float32 (128 partial sums a body, tests/test_hermite_gpu.py) attains
    against it on those rows; fp64 phi of the same rows (all rows up to the main size: the energy needs them).  Once a size."""
    if n not in _truth:
        s = random_system(n)[0]
        gm = H._gm(s)
        rows = W.fp64_rows(n, limit=W.MAIN if n <= W.MAIN else 1024)
        qp, vp = B.predict_all(H._stack(s, Q), H._stack(s, V), start[0], start[1], np.zeros(n, np.int64), 1, DT_MAX, KMAX)
        qp, vp = H._r32(qp), H._r32(vp)
        a, j, abs_j = B.evaluate_rows(qp, vp, gm, rows, SOFT)
        _, j32, _ = H._evaluate(qp.astype(np.float32), vp.astype(np.float32), H._gm(s, np.float32), SOFT, dtype=np.float32, nsplit=128)
        c = JERK_MARGIN * float(H.scaled_err(j32[:, rows], j, abs_j).max()) * 2.0 ** 24
        stale_a = B.evaluate_rows(H._stack(random_system(n)[1], Q), vp, gm, rows[:64], SOFT)[0]      # about what a skipped unit leaves
        assert (rel(stale_a, a[:, :64]) > 1e3 * TOL_F64_MAX).all(), "stale rows would pass the bound"
        _truth[n] = dict(rows=rows, a=a, j=j, abs_j=abs_j, c=c, phi=PR.phi_f64(qp, gm, SOFT, rows=rows), qp=qp,
                         seen=bits(np.stack(start)).copy())
    t = _truth[n]
    assert np.array_equal(t["seen"], bits(np.stack(start))), "the device's starting (a0, j0) differ from run to run"
    return t


def rel(x, y):
    return np.sqrt(((np.asarray(x, np.float64) - y) ** 2).sum(0)) / np.sqrt((np.asarray(y, np.float64) ** 2).sum(0))


@pytest.mark.parametrize("n,c", CASES)
def test_every_form_past_one_pass(gpu, O, n, c):
    """One block step per active set and form on the dense random system.  plain: the active (a1, j1) against fp64 at the
    restated prediction.  potential, nearest, contact (all radii 0): every bit of q, v, a, j, ticks and levels equals plain's.
    potential: phi of the active rows against fp64; the energy of the all-n step.  Every smaller set's (a1, j1) — and phi — carry
    the bits of the all-n step (the cut is the same, the pass is not); the all-n step twice gives the same bits."""
    s, stale = random_system(n)
    sets = W.wrap_sets(n) + [W.depth_set(n)]
    units_for = W.units_of(n, c)
    plain, lines = {}, []
    for form in ("plain", "potential", "nearest", "contact0"):
        with open_sim(gpu, s, SOFT, form) as sim:
            tiles, grid = int(sim.info("slots")) // W.TILE, grid_of(sim, form)
            first = None
            for k, act in enumerate(sets):
                groups = -(-len(act) // W.GROUP)
                units = units_for(groups)
                _, chunks, walked = W.plan(len(act), units, tiles)
                what = f"n={n} cut {c} {form}: {len(act)} active, {groups} groups x {chunks} chunks = {walked} units, {W.passes(walked, grid)} passes of {grid}"
                out, start, before, post, after = block_step(sim, form, s, stale, act, units, DT_MAX, KMAX)
                assert out["dt_min"] == out["dt_max"] == float(DT), what
                mask = check_untouched(s, act, start, before, post, after, KMAX, what)
                t = truth(n, start)
                if k == 0:
                    lines.append(what)
                    first = (post, after)
                    _, _, _, post2, after2 = block_step(sim, form, s, stale, act, units, DT_MAX, KMAX)
                    T.assert_same(post2, post, what + ", the same step again")
                    assert all(np.array_equal(x, y) for x, y in zip(after2, after)), what + ": phi / neighbours differ from run to run"
                else:      # pass depth: the same cut, other units
                    assert np.array_equal(bits(post.a[:, act]), bits(first[0].a[:, act])) and \
                        np.array_equal(bits(post.j[:, act]), bits(first[0].j[:, act])), what + ": (a1, j1) differ from the all-n step's"
                    for x, y in zip(after, first[1]):
                        assert np.array_equal(x[act], y[act]), what + ": phi / neighbours differ from the all-n step's"
                if form == "plain":
                    plain[k] = post
                    sel = mask[t["rows"]]
                    rows = t["rows"][sel]
                    ea = O.rel_err(post.a[:, rows], t["a"][:, sel])
                    ej = H.scaled_err(post.j[:, rows], t["j"][:, sel], t["abs_j"][sel]) * 2.0 ** 24
                    if k == 0:
                        lines.append(f"  acc max rel {ea.max():.2e} (bound {TOL_F64_MAX:.0e}), jerk {ej.max():.2f} x 2^-24 (bound C = {t['c']:.2f}) on {len(rows)} rows")
                    assert ea.max() <= TOL_F64_MAX, what + f": acceleration of body {rows[int(np.argmax(ea))]} off by {ea.max():.3e}"
                    assert ej.max() <= t["c"], what + f": jerk of body {rows[int(np.argmax(ej))]} off by {ej.max():.2f} x 2^-24, bound {t['c']:.2f}"
                else:
                    T.assert_same(post, plain[k], what + " against the plain form")
                if form == "potential":
                    sel = mask[t["rows"]]
                    rows = t["rows"][sel]
                    phi = after[0].view(np.float32)
                    assert np.isfinite(phi[rows]).all()
                    e = PR.rel_err(phi[rows], t["phi"][sel])
                    assert e.max() <= PR.TOL_F64_MAX, what + f": phi of body {rows[int(np.argmax(e))]} off by {e.max():.3e}"
                    if k == 0 and len(t["rows"]) == n:      # every phi belongs to this step: the energy, as test_potential_gpu checks it
                        want = PR.energy_of(s, t["phi"])
                        got = sim.potential_energy()
                        lines.append(f"  phi max rel {e.max():.2e}; potential energy off by {abs(got - want) / abs(want):.2e} (bound {PR.TOL_F64_MAX:.0e})")
                        assert abs(got - want) <= PR.TOL_F64_MAX * abs(want), what
    print("\n".join(lines))


# ------------------------------------------------------------------------------------------------- 2. the lattice, all forms
LATTICE_DT, LATTICE_KMAX, LATTICE_DT_MAX = 2.0 ** -30, 2, 2.0 ** -28      # tests/test_tie_lattice_gpu.py
LATTICE_CASES = [(W.MAIN, 1), (W.MAIN, 7), (W.MAIN, 10), (W.DEEP, 20)]


@lru_cache(maxsize=None)
def lattice(n):
    s, soft, q = N.dense_lattice(n)
    q2, _ = N.shifted(q)
    stale = doubled(s)
    return s, soft, q, q2, CR.dense_radii(n), stale


@lru_cache(maxsize=None)
def lattice_reference(n, form, moved):
    """(index, value bits) of nearest_ref / contact_ref on q or q2, folded tile by tile (the fold keeps the lowest index among
    equal values, like the brute force; a tile at a time needs no n x n matrix)."""
    s, soft, q, q2, radii, _ = lattice(n)
    pos, tiles = (q2 if moved else q), W.slots_of(n) // W.TILE
    idx, val = N.chunked(pos, 0.25, n, tiles, tiles) if form == "nearest" else CR.chunked(pos, radii, 0.25, n, tiles, tiles)
    return idx, bits(val)


@pytest.mark.parametrize("n,c", LATTICE_CASES)
def test_lattice_past_one_pass(gpu, n, c):
    """The dense tie lattice (tests/test_tie_lattice_gpu.py) at 10 and 20 layout tiles: (partner, value) of the active rows are
    the restatement's on q2, bit for bit, the inactive rows the restatement's on q; and q, v, a, j, ticks and levels carry the
    same bits under "nearest", "contact" (the lattice's radii, and all radii 0), "potential" and all three off."""
    s, soft, q, q2, radii, stale = lattice(n)
    sets = W.wrap_sets(n)[:3] + [W.depth_set(n), np.array([0, 512, 1024, 1536]), np.array(sorted(N.DENSE_TRIPLE))]
    base, lines = {}, []
    for form in ("nearest", "contact", "contact0", "potential", "plain"):
        with open_sim(gpu, s, soft, form, radii=radii if form == "contact" else None) as sim:
            tiles, grid = int(sim.info("slots")) // W.TILE, grid_of(sim, form)
            first = None
            for k, act in enumerate(sets):
                groups = -(-len(act) // W.GROUP)
                _, chunks, walked = W.plan(len(act), groups * c, tiles)
                what = f"n={n} cut {c} {form}: {len(act)} active, {walked} units, {W.passes(walked, grid)} passes of {grid}"
                out, start, before, post, after = block_step(sim, form, s, stale, act, groups * c, LATTICE_DT_MAX, LATTICE_KMAX)
                assert out["dt_min"] == LATTICE_DT, what
                mask = check_untouched(s, act, start, before, post, after, LATTICE_KMAX, what)
                if k == 0:
                    lines.append(what)
                    first = (post, after)
                    qp, _ = B.predict_all(H._stack(s, Q), H._stack(s, V), start[0], start[1], np.zeros(n, np.uint32), 1, LATTICE_DT_MAX, LATTICE_KMAX)
                    assert np.array_equal(bits(qp.astype(np.float32)), bits(q2.astype(np.float32))), what + ": the predictor does not land on q2"
                else:
                    assert np.array_equal(bits(post.a[:, act]), bits(first[0].a[:, act])) and \
                        np.array_equal(bits(post.j[:, act]), bits(first[0].j[:, act])), what + ": (a1, j1) differ from the all-n step's"
                    for x, y in zip(after, first[1]):
                        assert np.array_equal(x[act], y[act]), what + ": phi / neighbours differ from the all-n step's"
                if form in ("nearest", "contact"):
                    for rows, ref, name in ((mask, lattice_reference(n, form, True), "active"), (~mask, lattice_reference(n, form, False), "inactive")):
                        bad = np.flatnonzero(rows & ((after[0] != ref[0]) | (after[1] != ref[1])))
                        assert len(bad) == 0, what + f": {len(bad)} {name} rows differ from the restatement, first {bad[:6]} (tiles {bad[:6] // W.TILE})"
                if form == "nearest":
                    base[k] = post
                else:
                    T.assert_same(post, base[k], what + " against the nearest form")
    print("\n".join(lines))


# ----------------------------------------------------------------------------------------------------------- 3. a run, replayed
def test_replay_of_a_run_past_one_pass(gpu, O):
    """tests/test_hermite_block_gpu.py's single-step replay on its third system: n = 5 120, "block_units" 65 536 (10 chunks in
    every step), levels i mod 4 set by hand, to the first synchronised boundary.  At least 3 of the replayed steps walk more
    units than the grid holds workgroups."""
    with gpu.Simulation(W.MAIN, soft=SOFT) as sim:
        grid = int(sim.info("block_grid"))
    sizes, body_steps = T.replay(gpu, O, "wrap", 64)
    assert sizes == body_steps and len(sizes) <= 8 and sizes[-1] == W.MAIN
    deep = [x for x in body_steps if -(-x // W.GROUP) * 10 > grid]
    print(f"wrap: {len(deep)} of {len(sizes)} steps walk more than {grid} units")
    assert len(deep) >= 3


# ----------------------------------------------------------------------------------------------- 4. one run, five configurations
def test_one_run_in_five_configurations(gpu):
    """The run of the replay (one block of 8 ticks) under "block_units" 3 200, 65 536, 3 200 raised to 65 536 while the block is
    open (the row buffer is reallocated between two calls), "evolve_batch" 1, and once more: the same bits in q, v, a, j, ticks
    and levels and the same counts.  3 200 units are 10 chunks for every active set of up to 5 120 bodies, like 65 536."""
    s, soft, dt_max, kmax = T.replay_system("wrap")
    hand = T.replay_levels("wrap")
    for active in (1, 16, 1280, 5120):
        assert W.plan(active, 3200, 10)[1] == W.plan(active, 65536, 10)[1] == 10

    def run(raise_at=None, **opts):
        with T.hermite_sim(gpu, s, soft, **opts) as sim:
            sim.compute_acc_jerk()
            sim.set_block_levels(hand, kmax)
            steps = bodies = 0
            if raise_at:
                out = sim.evolve_block(dt_max, kmax=kmax, eta=T.ETA, eta_start=T.ETA_START, max_steps=raise_at)
                assert not out["synchronised"]
                steps, bodies = out["steps"], out["body_steps"]
                sim.set_option("block_units", 65536)
            out = sim.evolve_block(dt_max, kmax=kmax, eta=T.ETA, eta_start=T.ETA_START)
            assert out["synchronised"]
            return T.Snapshot(sim), (steps + out["steps"], bodies + out["body_steps"])

    want, counts = run(block_units=3200)
    print(f"one block: {counts[0]} block steps, {counts[1]} body-steps")
    assert counts[0] >= 4 and counts[1] > 2 * W.MAIN
    for what, kw in (("65 536 units", dict(block_units=65536)), ("3 200 raised to 65 536", dict(block_units=3200, raise_at=3)),
                     ("evolve_batch 1", dict(block_units=3200, evolve_batch=1)), ("the same again", dict(block_units=3200))):
        got, c = run(**kw)
        assert c == counts, what
        T.assert_same(got, want, what)

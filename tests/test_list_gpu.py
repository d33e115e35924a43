"""MI355X: the field of listed bodies and the neighbour split (include/murblist.h) through the C ABI, the Python interface and the
plugin.  Gather addressing bit for bit against the field read-out of a single massive body, values against fp64 within
tests/helpers/list_ref.py's bound for neighbour lists and hand-made lists, soft = 0, bit-identical results whatever the call looks
like, the split against the lists it stands for, the calls as observers, and the refused calls."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import field_ref as F         # noqa: E402
import knn_ref as K           # noqa: E402
import list_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
SHAPES = (1025, 2049)   # tiles of 512, 512 and 1; four tiles and 1
_fp, _ip, _up = (C.POINTER(t) for t in (C.c_float, C.c_int, C.c_ulong))


def make_sim(gpu, s, soft=R.SOFT, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft)
    for k, v in opts.items():
        if k in gpu.FIELD_OPTIONS:
            sim.set_field_option(k, v)
        elif k in gpu.NBR_OPTIONS:
            sim.set_neighbour_option(k, v)
        else:
            sim.set_option(k, v)
    sim.upload(s)
    return sim


def same(x, y):
    return F.same_bits(x, y)


def pick(d, rows):
    return {k: d[k][rows] for k in R.KEYS}


@lru_cache(maxsize=None)
def system(n):
    """field_ref.system(n).  Do not modify."""
    return R.system(n)


@lru_cache(maxsize=None)
def cpu_neighbours(n):
    """(offsets, idx) of the radii cycling through 0, 0.05, 0.1, 0.2, 0.45 over the bodies, restated on the CPU.  Do not modify."""
    return R.neighbours_f32(system(n), R.radii(n), R.SOFT)


def pool(n):
    """(bodies, lists): (body, list) pairs of every kind the tests use: empty, the lengths on both sides of a lane step, two
    and three lane steps, n - 1, the body in its own list, a duplicate, ascending neighbour lists."""
    perm = R.permutation(n)
    last = int(perm[n - 1])                                   # in no prefix shorter than n
    bodies, lists = [last], [np.zeros(0, np.int32)]
    for mine in R.prefix_lists(n):
        bodies.append(last)
        lists.append(mine)
    bodies += [int(perm[5]), 3]
    lists += [perm[:40], np.concatenate([perm[100:130], perm[110:112]])]
    o, j = cpu_neighbours(n)
    by_len = {}
    for b, mine in enumerate(R.lists_of(o, j)):
        by_len.setdefault(min(len(mine), 300) // 25, (b, mine))
    for b, mine in by_len.values():
        bodies.append(b)
        lists.append(mine.astype(np.int32))
    return np.array(bodies, np.int32), lists


# ------------------------------------------------------------------------------------------------ 1. gather addressing, bit-exact
def test_gather_addressing_is_bit_exact(gpu):
    """Single-entry lists [j] and two-entry lists [2k, 2k + 1] at 17 midpoints: bit for bit field_at of the same points on a
    context in which the listed bodies alone have mass.  Every other term there is +-0, so the sums are exact: the list sweep
    reads the records of exactly the listed bodies, at both ends of a tile and of the body range, and adds the two halves of a
    lane as the field sweep adds them."""
    n = 1025
    s = system(n)
    p, v, _ = F.midpoints(s, 17)
    with make_sim(gpu, s) as full, gpu.Simulation(n, soft=R.SOFT) as one:
        for src in [[j] for j in (0, 1, 510, 511, 512, 513, 1023, 1024)] + [[2 * k, 2 * k + 1] for k in (0, 255, 256, 511)]:
            t = {k: x.copy() for k, x in s.items()}
            t["m"][:] = 0
            t["m"][src] = s["m"][src]
            one.upload(t)
            want = one.field_at(p, v)
            o, j = R.csr([src] * 17)
            got = full.list_field_at(p, v, o, j)
            assert same(got, want), src
            assert np.all(got["phi"] > 0) and np.all(np.isfinite(got["jx"])), src
            if len(src) == 2:
                swapped = full.list_field_at(p, v, *R.csr([src[::-1]] * 17))
                assert same(swapped, want), "x + y of one lane's halves commutes"


# ------------------------------------------------------------------------------------------------------------------ 2. values
@pytest.mark.parametrize("n", SHAPES)
def test_neighbour_lists_against_fp64(gpu, n):
    """Lists from neighbours_of with radii cycling through 0, 0.05, 0.1, 0.2 and 0.45 over the bodies: every class of length is
    there (asserted on the CPU before the device is used), and a, j and phi of every body are within the bound."""
    s = system(n)
    length = np.diff(cpu_neighbours(n)[0].astype(np.int64))
    classes = (length == 0, (length >= 1) & (length <= 2), (length > 2) & (length <= 128), (length > 128) & (length <= 256), length > 256)
    if n == 1025:
        assert [int(c.sum()) for c in (classes[0], classes[1], length > 128, length > 256)] == [338, 127, 186, 70]
    for c in classes[1:]:
        assert (length[c] % 2 == 0).any() and (length[c] % 2 == 1).any(), "odd and even lengths in every class"
    with make_sim(gpu, s) as sim:
        o, j, _ = sim.neighbours_of(h=R.radii(n))
        got_len = np.diff(o.astype(np.int64))
        assert np.abs(got_len - length).max() <= 1 and (got_len != length).sum() <= 4, "the fp32 restatement, up to pairs on the sphere"
        got = sim.list_field_of(None, o, j)
    p, v, _ = R.body_points(s, np.arange(n))
    ref, c = R.bound_of(p, v, o, j, s, R.SOFT)
    R.check(got, ref, c, f"n={n}: neighbour lists, {int(o[-1])} entries")
    empty = got_len == 0
    assert empty.sum() >= 300 and all(np.all(F.bits(got[k][empty]) == 0) for k in R.KEYS), "+0.0f seven times"


@pytest.mark.parametrize("n", SHAPES)
def test_hand_made_lists_against_fp64(gpu, n):
    """Lists of exactly 1, 2, 3, 127, 128, 129, 255, 256, 257 and n - 1 entries, prefixes of a fixed permutation (not ascending),
    a list that holds the body itself, a list with a duplicate and an empty one: within the bound for the bodies and, with the
    same lists, for points of the caller's."""
    s = system(n)
    bodies, lists = pool(n)
    o, j = R.csr(lists)
    lens = [len(x) for x in lists]
    assert set(R.LENGTHS + (n - 1, 0)) <= set(lens) and bodies[11] in lists[11] and len(set(lists[12])) < len(lists[12])
    assert any(np.any(np.diff(x) < 0) for x in lists), "not ascending"
    p, v, _ = R.body_points(s, bodies)
    mp, mv, _ = F.midpoints(s, len(bodies))
    with make_sim(gpu, s) as sim:
        got = sim.list_field_of(bodies, o, j)
        got_at = sim.list_field_at(mp, mv, o, j)
        rest = sim.list_field_at(mp, None, o, j)
    ref, c = R.bound_of(p, v, o, j, s, R.SOFT)
    R.check(got, ref, c, f"n={n}: hand-made lists, bodies")
    own = float(H_G() * s["m"][bodies[11]]) / float(R.SOFT)
    assert got["phi"][11] > own, "the body in its own list adds G m / soft to phi"
    ref_at, c_at = R.bound_of(mp, mv, o, j, s, R.SOFT)
    R.check(got_at, ref_at, c_at, f"n={n}: hand-made lists, midpoints")
    ref_rest, c_rest = R.bound_of(mp, None, o, j, s, R.SOFT)
    R.check(rest, ref_rest, c_rest, f"n={n}: hand-made lists, midpoints at rest")
    assert all(F.bits(got[k])[0] == 0 for k in R.KEYS), "the empty list"


def H_G():
    import hermite_ref
    return hermite_ref.G


# ------------------------------------------------------------------------------------------------------------------ 3. soft = 0
def test_soft_zero(gpu):
    """soft = 0, odd lengths and lengths that are no multiple of 128, no coincident pair: finite and within the bound, so the slots
    past the end add +0 (a slot that counted, or added 0 x inf, would show).  One coincident entry gives NaN, by the forces' rule."""
    n = 1025
    s = system(n)
    perm = R.permutation(n)
    last = int(perm[n - 1])
    lists = [perm[:k] for k in (1, 3, 127, 129, 255, 257, 383, n - 1)]
    bodies = np.full(len(lists), last, np.int32)
    o, j = R.csr(lists)
    p, v, _ = R.body_points(s, bodies)
    zero = np.float32(0.0)
    with make_sim(gpu, s, soft=zero) as sim:
        got = sim.list_field_of(bodies, o, j)
        assert all(np.all(np.isfinite(got[k])) for k in R.KEYS)
        ref, c = R.bound_of(p, v, o, j, s, zero)
        R.check(got, ref, c, "soft = 0: lengths " + ", ".join(str(len(x)) for x in lists))
        for mine in ([last], np.concatenate([perm[:2], [last]]), np.concatenate([[last], perm[:200]])):
            bad = sim.list_field_of([last, last], *R.csr([mine, perm[:3]]))
            assert all(np.isnan(bad[k][0]) for k in R.KEYS[:6]) and not np.isfinite(bad["phi"][0]), len(mine)
            assert all(F.bits(bad[k])[1] == F.bits(got[k])[1] for k in R.KEYS), "the next point is untouched by it"


# ----------------------------------------------------------------------------------------------------------- 4. reproducibility
def alone(sim, bodies, lists):
    """Every (body, list) pair in a call of its own."""
    out = [sim.list_field_of([b], *R.csr([mine])) for b, mine in zip(bodies, lists)]
    return {k: np.concatenate([x[k] for x in out]) for k in R.KEYS}


@pytest.mark.parametrize("opts", [{}, {"field_batch": 16}, {"list_entries": 16}, {"field_batch": 16, "list_entries": 16}],
                         ids=["default", "field_batch=16", "list_entries=16", "both=16"])
def test_results_do_not_depend_on_the_call(gpu, opts):
    """The same point and list give the same bits alone, among 15, 17 and n + 5 points with repeats, at different places in the
    call with different other lists, under "field_batch" 16 (several launches) and "list_entries" 16 (ranges of a few points, and
    lists longer than the buffer), and through murblist_at given the body's own q and v."""
    n = 1025
    s = system(n)
    bodies, lists = pool(n)
    with make_sim(gpu, s) as plain:
        want = alone(plain, bodies, lists)
    rng = np.random.default_rng(8)
    with make_sim(gpu, s, **opts) as sim:
        if "list_entries" in opts:
            assert sim.neighbour_option("list_entries") == 16
        for count in (1, 15, 17, n + 5):
            rows = rng.integers(0, len(bodies), count) if count > 1 else np.array([10])
            if count == n + 5:
                rows[:len(bodies)] = np.arange(len(bodies))[::-1]   # every pair at least once
            o, j = R.csr([lists[r] for r in rows])
            got = sim.list_field_of(bodies[rows], o, j)
            assert same(got, pick(want, rows)), (opts, count)
            if count <= 17:
                p, v, _ = R.body_points(s, bodies[rows])
                assert same(sim.list_field_at(p, v, o, j), got), (opts, count, "at")
        again = sim.list_field_of(bodies, *R.csr(lists))
        assert same(again, want), opts


# ---------------------------------------------------------------------------------------------------------------------- 5. split
@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("opts", [{}, {"list_entries": 16}, {"field_batch": 16}], ids=["default", "list_entries=16", "field_batch=16"])
def test_split_is_the_list_sweep_on_the_neighbour_lists(gpu, n, opts):
    """murbsplit_of is bit for bit murblist_of on the lists murbnbr_of returns, with counts == diff(offsets): for all bodies and
    for a list of bodies with repeats, with one radius for all and with one per body."""
    s = system(n)
    some = np.concatenate([np.arange(0, n, 7), [n - 1, 0, 0, 512]]).astype(np.int32)
    with make_sim(gpu, s, **opts) as sim, make_sim(gpu, s) as plain:
        for bodies, h in ((None, np.float32(0.1)), (None, R.radii(n)), (some, np.float32(0.2)), (some, R.radii(n)[some])):
            counts, got = sim.irregular_field_of(bodies, h)
            o, j, _ = plain.neighbours_of(bodies, h)
            assert counts.dtype == np.uint64 and np.array_equal(counts, np.diff(o)), (opts, np.ndim(h))
            want = plain.list_field_of(bodies, o, j)
            assert same(got, want), (opts, bodies is None, np.ndim(h))
            assert int(o[-1]) > 0


def test_irregular_and_regular_make_the_whole(gpu):
    """For every eighth body at mixed radii: irregular + list_field_of(complement_lists(...)) is field_of's fp64 reference within
    the sum of the two parts' bounds, each scaled by its own part's magnitudes; force_split's regular is the fp64 field of the
    complement within the bounds of the two results it is formed from (each scaled by its own magnitudes) plus half an ulp of the
    result for the one rounding of the difference."""
    n = 1025
    s = system(n)
    bodies = np.arange(0, n, 8).astype(np.int32)
    h = R.radii(n)[bodies]
    with make_sim(gpu, s) as sim:
        split = sim.force_split(h, bodies)
        o, j, _ = sim.neighbours_of(bodies, h)
        co, cj = gpu.complement_lists(n, bodies, o, j)
        rest = sim.list_field_of(bodies, co, cj)
        again = sim.field_of(bodies)
    assert np.array_equal(split["counts"], np.diff(o)) and same(split["total"], again)
    assert np.array_equal(np.diff(co.astype(np.int64)) + np.diff(o.astype(np.int64)), np.full(len(bodies), n - 1))
    p, v, skip = R.body_points(s, bodies)
    ref_i, c_i = R.bound_of(p, v, o, j, s, R.SOFT)
    ref_r, c_r = R.bound_of(p, v, co, cj, s, R.SOFT)
    ref_t, c_t = F.bound_of(p, v, skip, s, R.SOFT)
    R.check(split["irregular"], ref_i, c_i, "irregular")
    R.check(rest, ref_r, c_r, "complement lists")
    F.check(split["total"], ref_t, c_t, "field_of")
    irr, reg, tot, fs = R.as_tuple(split["irregular"]), R.as_tuple(rest), R.as_tuple(split["total"]), R.as_tuple(split["regular"])
    norm = lambda x: np.sqrt((np.atleast_2d(x) ** 2).sum(0))    # noqa: E731
    for at, name in enumerate(("a", "j", "phi")):
        whole = norm(irr[at] + reg[at] - ref_t[at])
        allowed = R.U24 * (c_i[name] * ref_i[3][name] + c_r[name] * ref_r[3][name])
        print(name, "irregular + complement against the whole: largest share of the allowed error", float((whole / allowed).max()))
        assert np.all(whole <= allowed), name
        off = norm(fs[at] - ref_r[at])
        allowed = R.U24 * (c_t[name] * ref_t[3][name] + c_i[name] * ref_i[3][name] + norm(ref_r[at]))
        print(name, "regular against the fp64 complement: largest share of the allowed error", float((off / allowed).max()))
        assert np.all(off <= allowed), name
    want = gpu.split_regular(split["total"], split["irregular"])
    assert same(split["regular"], want)


# --------------------------------------------------------------------------------------------------- 6. observers, 7. refusals
def raw(gpu, sim, name, *args):
    return getattr(gpu.lib(), name)(sim._h, *args)


def ptr(x, t):
    return None if x is None else np.ascontiguousarray(x).ctypes.data_as(t)


def fresh_out(count):
    return [np.full(count, -7.0, np.float32) for _ in range(7)]


def call_of(gpu, sim, bodies, o, j, out, count=None):
    b = None if bodies is None else np.ascontiguousarray(bodies, np.int32)
    o = None if o is None else np.ascontiguousarray(o, np.uint64)
    j = None if j is None else np.ascontiguousarray(j, np.int32)
    count = len(b) if count is None else count
    return raw(gpu, sim, "murblist_of", count, ptr(b, _ip), ptr(o, _up), ptr(j, _ip), *[ptr(x, _fp) for x in out])


def call_at(gpu, sim, pos, vel, o, j, out, count):
    o = None if o is None else np.ascontiguousarray(o, np.uint64)
    j = None if j is None else np.ascontiguousarray(j, np.int32)
    return raw(gpu, sim, "murblist_at", count, *[ptr(x, _fp) for x in pos], *[ptr(x, _fp) for x in vel], ptr(o, _up), ptr(j, _ip),
               *[ptr(x, _fp) for x in out])


def call_split(gpu, sim, bodies, h, h_all, counts, out, count=None):
    b = None if bodies is None else np.ascontiguousarray(bodies, np.int32)
    count = len(b) if count is None else count
    return raw(gpu, sim, "murbsplit_of", count, ptr(b, _ip), ptr(h, _fp), float(h_all), ptr(counts, _up), *[ptr(x, _fp) for x in out])


def refused_forms(gpu, sim, n):
    """One refused form of each call; each returns MURBHIP_E_INVALID and writes nothing."""
    out = fresh_out(2)
    pos = [np.zeros(2, np.float32)] * 3
    assert call_of(gpu, sim, [0, 1], [0, 1, 2], [1, n], out) == E_INVALID
    assert call_at(gpu, sim, pos, [None] * 3, [0, 1, 2], [1, -1], out, 2) == E_INVALID
    assert call_split(gpu, sim, [0, 1], None, -1.0, None, out) == E_INVALID
    assert all(np.all(x == -7.0) for x in out)


@pytest.mark.parametrize("nearest", (0, 1))
def test_observers_leave_the_run_alone(gpu, nearest):
    """step; the three calls and their refused forms; step, under "integrator" 2: every later bit (state, acc, nearest(), field_of,
    neighbours_of) is what it is without them, and each call returns the bits it returns as the only observer."""
    n = 1025
    s, soft = K.plummer(n)
    bodies = np.arange(0, n, 5).astype(np.int32)
    pts = np.stack([s[k][:40] + np.float32(0.25) for k in ("qx", "qy", "qz")])
    o, j = R.csr([np.arange(k % 300, dtype=np.int32)[::-1] for k in range(7, 7 + 13 * len(bodies), 13)])
    po, pj = R.csr([np.arange(3 * k, dtype=np.int32) for k in range(40)])
    seen = {}

    def run(probe):
        with gpu.Simulation(n, soft=soft, g=1.0) as sim:
            sim.set_option("integrator", 2)
            sim.set_option("nearest", nearest)
            sim.upload(s)
            sim.steps(2.0 ** -10, 1)
            if probe in ("all", "of"):
                seen[probe, "of"] = sim.list_field_of(bodies, o, j)
            if probe in ("all", "refused"):
                refused_forms(gpu, sim, n)
            if probe in ("all", "at"):
                seen[probe, "at"] = sim.list_field_at(pts, None, po, pj)
            if probe in ("all", "split"):
                seen[probe, "split"] = sim.irregular_field_of(h=0.3)[1]
            sim.steps(2.0 ** -10, 1)
            sim.sync()
            st = sim.state()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.neighbours_of(h=0.2))
            rec += [sim.field_of(bodies)[k] for k in R.KEYS]
            if nearest:
                rec += list(sim.nearest())
            return [np.ascontiguousarray(x).view(np.uint8) for x in rec]

    plain = run(None)
    for probe in ("all", "of", "at", "split", "refused"):
        assert all(np.array_equal(x, y) for x, y in zip(plain, run(probe))), probe
    for kind in ("of", "at", "split"):
        assert same(seen["all", kind], seen[kind, kind]), kind
        assert np.any(seen[kind, kind]["phi"] > 0)


def test_refusals(gpu):
    """Every refusal the header lists: the code, nothing written, nothing launched that a later call could see."""
    n = 600
    s = system(1025)
    s = {k: np.ascontiguousarray(x[:n]) for k, x in s.items()}
    good_o, good_j = R.csr([[1, 2, 3], [], [0, 599]])
    bodies = np.array([5, 6, 7], np.int32)
    pos = [np.ascontiguousarray(s[k][:3] + np.float32(0.5)) for k in R.Q]
    vel = [np.ascontiguousarray(s[k][:3]) for k in R.V]
    out = fresh_out(3)
    counts = np.full(3, 77, np.uint64)

    def refused(code, rc, what):
        assert rc == code, (what, rc)
        assert all(np.all(x == -7.0) for x in out) and np.all(counts == 77), what
        assert same(sim.list_field_of(bodies, good_o, good_j), before), what

    with gpu.Simulation(n, soft=R.SOFT) as sim:
        assert call_of(gpu, sim, bodies, good_o, good_j, out) == E_STATE, "before the first upload"
        assert call_at(gpu, sim, pos, vel, good_o, good_j, out, 3) == E_STATE and call_split(gpu, sim, bodies, None, 0.1, counts, out) == E_STATE
        assert call_of(gpu, sim, bodies, None, None, out, count=0) == 0 and call_at(gpu, sim, [None] * 3, [None] * 3, None, None, out, 0) == 0
        assert call_split(gpu, sim, None, None, -1.0, None, out, count=0) == 0, "count 0 does nothing, in every state"
        sim.upload(s)
        before = sim.list_field_of(bodies, good_o, good_j)
        lists_before = sim.neighbours_of(bodies, 0.2)
        for name, call in (("of", lambda o, j: call_of(gpu, sim, bodies, o, j, out)),
                           ("at", lambda o, j: call_at(gpu, sim, pos, vel, o, j, out, 3))):
            refused(E_INVALID, call(None, good_j), name + ": NULL offsets")
            refused(E_INVALID, call(good_o, None), name + ": NULL idx with a non-zero total")
            refused(E_INVALID, call([1, 3, 3, 5], good_j), name + ": offsets[0] != 0")
            refused(E_INVALID, call([0, 3, 2, 5], good_j), name + ": offsets decrease")
            for bad in (-1, n, 2 ** 31 - 1, -2 ** 31):
                for place in (0, 4):
                    j = good_j.copy()
                    j[place] = bad
                    refused(E_INVALID, call(good_o, j), name + f": entry {bad} at {place}")
            assert call([0, 0, 0, 0], None) == 0 and all(np.all(F.bits(x) == 0) for x in out), name + ": empty lists need no idx"
            for x in out:
                x[:] = -7.0
        refused(E_INVALID, call_of(gpu, sim, None, good_o, good_j, out, count=3), "all bodies, but count != n")
        for bad in (-1, n, 2 ** 31 - 1):
            refused(E_INVALID, call_of(gpu, sim, [5, bad, 7], good_o, good_j, out), f"body index {bad}")
            refused(E_INVALID, call_split(gpu, sim, [5, bad, 7], None, 0.1, counts, out), f"split: body index {bad}")
        refused(E_INVALID, call_split(gpu, sim, None, None, 0.1, counts, out, count=3), "split: all bodies, but count != n")
        for bad in (-0.5, np.nan, np.inf):
            refused(E_INVALID, call_split(gpu, sim, bodies, None, bad, counts, out), f"split: radius {bad}")
            refused(E_INVALID, call_split(gpu, sim, bodies, np.array([0.1, bad, 0.1], np.float32), 0.1, counts, out), f"split: radius {bad} of one body")
        for k in range(3):
            args = list(pos)
            args[k] = None
            refused(E_INVALID, call_at(gpu, sim, args, vel, good_o, good_j, out, 3), "a NULL position array")
            part = list(vel)
            part[k] = None
            refused(E_INVALID, call_at(gpu, sim, pos, part, good_o, good_j, out, 3), "velocities set in part")
            for bad in (np.nan, np.inf, -np.inf):
                args = [x.copy() for x in pos]
                args[k][1] = bad
                refused(E_INVALID, call_at(gpu, sim, args, vel, good_o, good_j, out, 3), f"coordinate {bad}")
                args = [x.copy() for x in vel]
                args[k][2] = bad
                refused(E_INVALID, call_at(gpu, sim, pos, args, good_o, good_j, out, 3), f"velocity {bad}")
        for hole in ((0,), (0, 1), (3, 4), (5,)):   # ax ay az, jx jy jz set in part
            part = [None if k in hole else x for k, x in enumerate(out)]
            refused(E_INVALID, call_of(gpu, sim, bodies, good_o, good_j, part), f"outputs {hole} missing")
            refused(E_INVALID, call_split(gpu, sim, bodies, None, 0.1, counts, part), f"split: outputs {hole} missing")
        assert gpu.lib().murblist_of(None, 3, *[None] * 10) == E_INVALID, "no context"
        # whole groups may be left out, counts too
        only_phi = [None] * 6 + [out[6]]
        assert call_of(gpu, sim, bodies, good_o, good_j, only_phi) == 0 and np.array_equal(F.bits(out[6]), F.bits(before["phi"]))
        assert all(np.all(x == -7.0) for x in out[:6])
        assert call_split(gpu, sim, bodies, None, 0.2, None, only_phi) == 0 and call_split(gpu, sim, bodies, None, 0.2, counts, [None] * 7) == 0
        assert np.array_equal(counts, np.diff(lists_before[0]))
        assert all(np.array_equal(x, y) for x, y in zip(sim.neighbours_of(bodies, 0.2), lists_before))
        with pytest.raises(ValueError):
            sim.list_field_of(bodies, good_o[:-1], good_j)
        with pytest.raises(gpu.MurbHipError) as e:
            sim.list_field_of(bodies, good_o, [1, 2, 3, 0, n])
        assert e.value.code == E_INVALID


def test_open_block_and_two_shards_are_refused(gpu):
    n = 600
    s, soft = K.plummer(n)
    o, j = R.csr([[1, 2], [0]])
    pts = np.zeros((3, 2), np.float32)

    def codes(sim):
        found = []
        for call in (lambda: sim.list_field_of([0, 1], o, j), lambda: sim.list_field_at(pts, None, o, j),
                     lambda: sim.irregular_field_of([0, 1], 0.1), lambda: sim.force_split(0.1)):
            with pytest.raises(gpu.MurbHipError) as e:
                call()
            found.append(e.value.code)
        return found

    def run(probe):
        with gpu.Simulation(n, soft=soft, g=1.0) as sim:
            sim.set_option("integrator", 2)
            sim.upload(s)
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert codes(sim) == [E_STATE] * 4
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [np.ascontiguousarray(st[k]).view(np.uint8) for k in sorted(st)] + [F.bits(sim.list_field_of([0, 1], o, j)["phi"])]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    with gpu.Simulation(n, soft=soft, g=1.0, devices=[0, 0]) as sim:
        sim.upload(s)
        assert codes(sim) == [E_STATE] * 4


def test_span_kind(gpu):
    """"profile" 2 records the list sweep's launches as spans of the kind "list": one per range of points that holds an entry (40
    bodies under "field_batch" 16: three launches; the split of 40 bodies: three more), outside the force_* figures, while the
    split's count and fill sweeps stay "nbr" spans."""
    n = 600
    s = system(1025)
    s = {k: np.ascontiguousarray(x[:n]) for k, x in s.items()}
    o, j = R.csr([[(k + 1) % n, (k + 2) % n] for k in range(40)])

    def run(level, on):
        with make_sim(gpu, s, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if on:
                sim.list_field_of(np.arange(40), o, j)
                sim.irregular_field_of(np.arange(40), 0.3)
            sim.knn_of([0, 1], k=1)
            return {k: sim.info(k) for k in ("span_list_count", "span_list_ms_avg", "span_nbr_count", "span_knn_count", "span_field_count",
                                             "force_launches")}

    with_it, without = run(2, True), run(2, False)
    assert with_it["span_list_count"] == 3 + 3 and with_it["span_list_ms_avg"] > 0
    assert with_it["span_nbr_count"] == 3 + 3 and without["span_nbr_count"] == 0
    assert without["span_list_count"] == 0 == without["span_list_ms_avg"] and with_it["span_field_count"] == 0
    assert with_it["span_knn_count"] == without["span_knn_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)["span_list_count"] == 0


# ------------------------------------------------------------------------------------------------------------------ 8. plugin
def test_plugin_force_split(gpu):
    """HostSim.force_split(h) (SimulationNBodyHIP::forceSplit) equals Simulation.force_split(h) of the same bodies bit for bit,
    after an iteration too; some bodies have neighbours and some have none."""
    n, soft, dt = 2049, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt) as host:
        for _ in range(2):
            st = host.state()
            extent = float(np.ptp(st["qx"]))
            got = host.force_split(0.02 * extent)
            with gpu.Simulation(n, soft=soft) as sim:
                sim.upload(st)
                want = sim.force_split(0.02 * extent)
            assert np.array_equal(got["counts"], want["counts"]) and got["counts"].max() > 2
            for part in ("irregular", "total", "regular"):
                assert same(got[part], want[part]), part
            print(f"galaxy n={n}: neighbours within 2 % of the extent: mean {got['counts'].mean():.1f}, max {int(got['counts'].max())}")
            host.step(1)

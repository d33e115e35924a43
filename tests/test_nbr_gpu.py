"""MI355X: the neighbours-within-a-radius read-out (include/murbnbr.h) through the C ABI, the Python interface and the plugin.
Lattices have exact r2, so every comparison there is equality of bits with tests/helpers/nbr_ref.py, under every chunk count,
launch cut and list-buffer cut.  Floats (a Plummer sphere): the exact sets once no pair lies near the threshold.  Cross-checks
with the k-nearest-neighbour read-out and the Hermite sweeps' nearest neighbour.  The calls as observers, and the refused calls."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import knn_ref as K           # noqa: E402
import nbr_ref as NB          # noqa: E402
import nearest_ref as NR      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
Q = ("qx", "qy", "qz")
_fp, _ip, _up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ulong)
N = 2500
TOTALS = {0: 12, 1: 12678, 2: 62386, 3: 213992}      # dense_lattice(2500), soft 0.5: entries of all bodies' lists at h
MAXIMA = {0: 2, 1: 7, 2: 33, 3: 118}                 # ... and the longest list


def make_sim(gpu, s, soft, g=None, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft) if g is None else gpu.Simulation(len(s["m"]), soft=soft, g=g)
    for k, v in opts.items():
        (sim.set_field_option if k in gpu.FIELD_OPTIONS else sim.set_neighbour_option if k in gpu.NBR_OPTIONS else sim.set_option)(k, v)
    sim.upload(s)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def bits(x):
    return np.ascontiguousarray(x).view(np.int32 if x.dtype.itemsize == 4 else np.int64)


def row(res, p):
    """(idx, r2) of point p of an (offsets, idx, r2) result."""
    a, b = int(res[0][p]), int(res[0][p + 1])
    return res[1][a:b], res[2][a:b]


def take(res, points):
    """The (offsets, idx, r2) result of the listed points, from a result that holds them as rows."""
    rows = [row(res, p) for p in points]
    offsets = np.zeros(len(rows) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r[0]) for r in rows])
    return offsets, np.concatenate([r[0] for r in rows] or [np.zeros(0, np.int32)]), np.concatenate([r[1] for r in rows] or [np.zeros(0, np.float32)])


@lru_cache(maxsize=None)
def dense():
    """(state, soft, q_int, soft2) of nearest_ref.dense_lattice(2500): 5 layout tiles, 452 bodies in the ragged last one."""
    s, soft, q = NR.dense_lattice(N)
    return s, soft, q, np.float32(soft) * np.float32(soft)


@lru_cache(maxsize=None)
def dense_ref(h):
    _, _, q, soft2 = dense()
    return NB.neighbours(q, soft2, h)


@lru_cache(maxsize=None)
def plummer():
    return K.plummer(3000)


# ------------------------------------------------------------------------------------------------------------------ 1. lattices
@pytest.mark.parametrize("h", (0, 1, 2, 3))
def test_dense_lattice_every_cut(gpu, h):
    """All bodies of dense_lattice(2500) at h: "field_chunks" 1 to 5, "field_batch" 0 and 496 (six launches, the last a group of
    4 real points), "list_entries" 0 and 1000: every combination gives the restatement's arrays, hence each other's; the totals and
    the longest list are the known answers; the count-only call gives the same offsets."""
    s, soft, _, _ = dense()
    want = dense_ref(h)
    assert int(want[0][-1]) == TOTALS[h] and np.diff(want[0].astype(np.int64)).max() == MAXIMA[h]
    with make_sim(gpu, s, soft) as sim:
        for chunks in (1, 2, 3, 4, 5):
            for batch in (0, 496):
                for entries in (0, 1000):
                    sim.set_field_option("field_chunks", chunks)
                    sim.set_field_option("field_batch", batch)
                    sim.set_neighbour_option("list_entries", entries)
                    assert sim.field_option("field_chunks") == chunks and sim.neighbour_option("list_entries") == (entries or 1 << 26)
                    assert batch == 0 or gpu.field_layout(N, chunks, batch, N)["batches"] == 6
                    got = sim.neighbours_of(h=h)
                    assert NB.same(got, want), (chunks, batch, entries)
                    assert int(got[0][-1]) == TOTALS[h] and np.diff(got[0].astype(np.int64)).max() == MAXIMA[h]
            count_only = sim.neighbours_of(h=float(h), lists=False)
            assert count_only[1] is None and count_only[2] is None and np.array_equal(count_only[0], want[0])


def test_lists_longer_than_the_list_buffer(gpu):
    """64 bodies at h = 40: each lists all 2 499 others, so every list is longer than "list_entries" 1000 (a range of one point, and
    the buffer grows to it); with 16 and with the default the same arrays."""
    s, soft, q, soft2 = dense()
    who = np.arange(0, N, 40, dtype=np.int32)[:63].tolist() + [N - 1]
    want = NB.neighbours(q, soft2, 40, bodies=who)
    assert (np.diff(want[0].astype(np.int64)) == N - 1).all() and len(who) == 64
    for entries in (1000, 16, 0):
        with make_sim(gpu, s, soft, list_entries=entries, field_chunks=3) as sim:
            assert NB.same(sim.neighbours_of(who, h=40), want), entries


# ------------------------------------------------------------------------------------------------------------------- 2. small n
@pytest.mark.parametrize("n", (1, 2, 3, 7, 16, 17))
def test_small_n_lists_everyone_else(gpu, n):
    rng = np.random.default_rng(n)
    q = rng.permutation(40)[:n][None, :] * np.array([[1], [3], [7]]) + 2      # distinct integer points
    s = {"qx": q[0].astype(np.float32), "qy": q[1].astype(np.float32), "qz": q[2].astype(np.float32),
         "vx": np.zeros(n, np.float32), "vy": np.zeros(n, np.float32), "vz": np.zeros(n, np.float32), "m": np.ones(n, np.float32)}
    want = NB.neighbours(q, np.float32(0.25), 1e6)
    with make_sim(gpu, s, np.float32(0.5)) as sim:
        got = sim.neighbours_of(h=1e6)
        huge = sim.neighbours_of(h=3e19)      # thr rounds to +inf
    assert NB.same(got, want) and NB.same(huge, want)
    for p in range(n):
        assert row(got, p)[0].tolist() == [j for j in range(n) if j != p]
    assert int(got[0][-1]) == n * (n - 1)


# ------------------------------------------------------------------------------------------------------- 3. padding, the origin
def test_padding_and_the_origin(gpu):
    """nearest_ref.lattice(1500): body 0 sits at the origin, where the padding slots of the ragged last tile lie; bodies 5 and 400
    share a point.  A point at the origin with a large h lists the n bodies without a skip and n - 1 with skip = 0, never a slot
    >= n; h = 0 at body 5 lists exactly body 400, and at the origin body 0 alone."""
    n = 1500
    s, soft = NR.lattice(n)
    q = np.stack([s[c] for c in Q]).astype(np.int64)
    soft2 = np.float32(soft) * np.float32(soft)
    origin = np.zeros((3, 3), np.float32)
    with make_sim(gpu, s, soft) as sim:
        got = sim.neighbours_at(origin, 1e5, skip=[-1, 0, 7])
        zero = sim.neighbours_at(origin, 0.0, skip=[-1, 0, 7])
        five = sim.neighbours_of([5, 400, 0], h=0.0)
        everyone = sim.neighbours_of(h=1e5)
    assert NB.same(got, NB.neighbours_at(q, soft2, 1e5, origin.astype(np.int64), skip=[-1, 0, 7]))
    assert row(got, 0)[0].tolist() == list(range(n)) and row(got, 1)[0].tolist() == list(range(1, n))
    assert row(got, 2)[0].tolist() == [j for j in range(n) if j != 7]
    assert np.diff(zero[0].astype(np.int64)).tolist() == [1, 0, 1] and zero[1].tolist() == [0, 0] and (zero[2] == soft2).all()
    assert row(five, 0)[0].tolist() == [400] and row(five, 1)[0].tolist() == [5] and row(five, 2)[0].tolist() == []
    assert row(five, 0)[1][0] == soft2
    assert int(everyone[0][-1]) == n * (n - 1) and everyone[1].max() == n - 1 and everyone[1].min() == 0


# --------------------------------------------------------------------------------------------------- 4. radii, subsets and skip
def test_per_point_radii_subsets_and_skip(gpu):
    s, soft, q, soft2 = dense()
    rng = np.random.default_rng(4)
    sub = rng.integers(0, N, 333).astype(np.int32)
    sub[:6] = (7, 7, N - 1, 0, 14, 7)      # a body listed twice, the last, the first, one of the triple
    h = rng.choice(np.array([0, 1, 40], np.float32), 333)
    h[:6] = (1, 40, 40, 1, 0, 0)
    p = np.stack([s[c] for c in Q])
    other = np.where(sub == 3, 4, 3).astype(np.int32)      # a skipped body that is not the one on the point
    with make_sim(gpu, s, soft, field_batch=112, list_entries=5000) as sim:
        got = sim.neighbours_of(sub, h=h)
        at_self = sim.neighbours_at(p[:, sub], h, skip=sub)
        at_other = sim.neighbours_at(p[:, sub], h, skip=other)
        at_none = sim.neighbours_at(p[:, sub], h, skip=np.full(333, -1, np.int32))
        at_null = sim.neighbours_at(p[:, sub], h)
        everyone = {hh: sim.neighbours_of(h=hh) for hh in (0, 1)}
        all_at = sim.neighbours_at(p, 1.0, skip=np.arange(N, dtype=np.int32))
    assert NB.same(got, NB.neighbours(q, soft2, h, bodies=sub))
    assert NB.same(at_self, got), "points on the bodies with skip = i are the bodies' lists"
    assert NB.same(at_other, NB.neighbours_at(q, soft2, h, q[:, sub], skip=other))
    assert NB.same(at_none, NB.neighbours_at(q, soft2, h, q[:, sub])) and NB.same(at_null, at_none)
    assert all(b in row(at_none, e)[0] for e, b in enumerate(sub)), "without a skip the body on the point is listed"
    assert NB.same(all_at, everyone[1]) and NB.same(everyone[1], dense_ref(1))
    for hh in (0, 1):      # a point's list does not depend on the other points of the call
        pick = np.nonzero(h == hh)[0]
        assert NB.same(take(got, pick), take(everyone[hh], sub[pick]))


# ---------------------------------------------------------------------------------------- 5. symmetry, knn, the sweeps' nearest
def test_symmetry_and_agreement_with_knn_and_nearest(gpu):
    """A common h gives a symmetric relation with equal r2 bits.  Every murbknn_of(k = 32) entry with r2 <= thr appears with the
    same r2 bits; a list of at most 32 entries, sorted by (r2, index), is the head of the knn list.  With "nearest" 1 after
    compute_acc_jerk, nn_i is listed if and only if its r2_i <= thr."""
    s, soft, _, soft2 = dense()
    with make_sim(gpu, s, soft, integrator=2, nearest=1) as sim:
        sim.compute_acc_jerk()
        nn, nn_r2 = sim.nearest()
        kidx, kr2 = sim.knn_of(k=32)
        for h in (1, 2):
            thr = NR.threshold(h, soft2)
            offsets, idx, r2 = sim.neighbours_of(h=h)
            counts = np.diff(offsets.astype(np.int64))
            own = np.repeat(np.arange(N), counts)
            pairs = {}
            for i, j, r in zip(own.tolist(), idx.tolist(), bits(r2).tolist()):
                pairs[(i, j)] = r
            assert all(pairs.get((j, i)) == r for (i, j), r in pairs.items()), "not symmetric, or r2(i, j) != r2(j, i)"
            for i in range(N):
                mine, mine_r2 = row((offsets, idx, r2), i)
                near = kr2[i] <= thr
                assert all(pairs.get((i, int(j))) == int(b) for j, b in zip(kidx[i][near], bits(kr2[i][near]))), i
                if len(mine) <= 32:
                    order = np.lexsort((mine, mine_r2))
                    assert np.array_equal(mine[order], kidx[i][:len(mine)]) and np.array_equal(bits(mine_r2[order]), bits(kr2[i][:len(mine)])), i
                    assert len(mine) == 32 or not near[len(mine):].any()
                assert ((i, int(nn[i])) in pairs) == bool(nn_r2[i] <= thr), i
            assert (counts <= 32).sum() > N // 2 and (nn_r2 <= thr).sum() > N // 2


# --------------------------------------------------------------------------------------------------------------------- 6. floats
@pytest.mark.parametrize("h,entries", ((0.05, 212), (0.2, 13930), (1.0, 1180004)))
def test_plummer_exact_sets(gpu, h, entries):
    """knn_ref.plummer(3000): the fp64 reference has no pair within 4 fp32 ulps of thr (asserted first), so the sets are decided
    and must be exact; each r2 within 4 ulps of its pair's fp64 value (three fma roundings and the rounding of the differences)."""
    s, soft = plummer()
    inside, ref, thr, near = NB.neighbours_f64(s, soft, h)
    assert near == 0, f"{near} pairs within 4 ulps of the threshold: the reference cannot decide them"
    want = NB.csr(inside, ref)
    assert int(want[0][-1]) == entries and thr == gpu.neighbour_threshold(h, soft)
    with make_sim(gpu, s, soft, g=1.0) as sim:
        offsets, idx, r2 = sim.neighbours_of(h=h)
    assert np.array_equal(offsets, want[0]) and np.array_equal(idx, want[1])
    exact = ref[inside]      # row-major: the lists' order
    ulps = np.abs(r2.astype(np.float64) - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
    print(f"h={h}: {entries} entries, r2 off its fp64 value by at most {ulps.max():.2f} ulps")
    assert ulps.max() <= 4 and (r2 <= thr).all()


def test_lists_read_the_current_state(gpu):
    """After Hermite steps the lists are those of the downloaded positions: every pair whose fp64 r2 is further than 4 fp32 ulps
    from thr is in or out as the reference says (none is nearer here), and the state has moved."""
    s, soft = plummer()
    h = 0.2
    with make_sim(gpu, s, soft, g=1.0, integrator=2) as sim:
        before = sim.neighbours_of(h=h)
        sim.steps(2.0 ** -7, 4)
        now = dict(sim.state(), m=s["m"])
        offsets, idx, r2 = sim.neighbours_of(h=h)
    assert not np.array_equal(now["qx"], s["qx"])
    inside, ref, thr, near = NB.neighbours_f64(now, soft, h)
    got = np.zeros_like(inside)
    got[np.repeat(np.arange(3000), np.diff(offsets.astype(np.int64))), idx] = True
    decided = np.abs(ref - float(thr)) > 4 * float(np.spacing(thr))
    print(f"after 4 steps: {int(offsets[-1])} entries, {near} undecided pairs")
    assert np.array_equal(got[decided], inside[decided]) and int(got.sum()) == int(offsets[-1])
    assert not np.array_equal(offsets, before[0]) or not np.array_equal(idx, before[1]), "the lists did not follow the bodies"


# ------------------------------------------------------------------------------------------------------------------ 7. observers
def test_observers_leave_the_run_alone(gpu):
    s, soft = plummer()
    p = np.stack([s[c] for c in Q])[:, :50] + np.float32(0.01)

    def run(probe):
        def look(sim):
            if probe:
                sim.neighbours_of(h=0.2)
                sim.neighbours_of([3, 1, 2999], h=[0.0, 1.0, 5.0], lists=False)
                sim.neighbours_at(p, 0.3)
        with make_sim(gpu, s, soft, g=1.0, integrator=2, list_entries=4096) as sim:
            look(sim)
            for _ in range(3):
                sim.steps(2.0 ** -9, 2)
                look(sim)
            out = sim.evolve(2.0 ** -7, max_steps=10)
            look(sim)
            st = sim.state()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.jerk())
            return [bits(x) for x in rec], out

    (a, out_a), (b, out_b) = run(False), run(True)
    assert out_a == out_b
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_other_read_outs_survive_a_call(gpu):
    """field_of, tidal_of and knn_of share the point buffers: their bits are the same before and after neighbours calls."""
    s, soft = plummer()
    who = np.arange(0, 3000, 7, dtype=np.int32)
    with make_sim(gpu, s, soft, g=1.0) as sim:
        f0, t0, k0 = sim.field_of(who), sim.tidal_of(who), sim.knn_of(who, k=8)
        sim.neighbours_of(h=0.2)
        sim.neighbours_at(np.stack([s[c] for c in Q])[:, :100], 1.0)
        f1, t1, k1 = sim.field_of(who), sim.tidal_of(who), sim.knn_of(who, k=8)
    assert all(np.array_equal(bits(f0[k]), bits(f1[k])) for k in f0) and all(np.array_equal(bits(t0[k]), bits(t1[k])) for k in t0)
    assert np.array_equal(k0[0], k1[0]) and np.array_equal(bits(k0[1]), bits(k1[1]))


# -------------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(gpu):
    s, soft = NR.lattice(600)
    n = 600
    lib = gpu.lib()
    P = [np.ascontiguousarray(s[c][:20] + np.float32(0.5)) for c in Q]
    skip = np.full(20, -1, np.int32)
    radii = np.full(20, 400, np.float32)
    off = np.zeros(21, np.uint64)
    idx, r2 = np.full(20 * n, -7, np.int32), np.full(20 * n, -7, np.float32)
    fp = lambda x: x.ctypes.data_as(_fp)      # noqa: E731
    ip = lambda x: x.ctypes.data_as(_ip)      # noqa: E731

    def at(count=20, pos=None, sk=skip, h=radii, h_all=0.0, offsets=off, capacity=20 * n):
        pos = [fp(x) for x in P] if pos is None else pos
        return lib.murbnbr_at(sim._h, count, *pos, ip(sk) if sk is not None else None, fp(h) if h is not None else None, h_all,
                              offsets.ctypes.data_as(_up) if offsets is not None else None, ip(idx), fp(r2), capacity)

    def of(bodies, count=None, h=None, h_all=400.0, offsets=off, capacity=20 * n):
        b = np.ascontiguousarray(bodies, np.int32) if bodies is not None else None
        return lib.murbnbr_of(sim._h, len(b) if count is None else count, ip(b) if b is not None else None, fp(h) if h is not None else None,
                              h_all, offsets.ctypes.data_as(_up) if offsets is not None else None, ip(idx), fp(r2), capacity)

    def refused(code, rc, what):
        """The call returned its code, wrote no entry, and a following call returns what it returned before."""
        assert rc == code, (what, rc)
        assert (idx == -7).all() and (r2 == -7).all(), what
        assert NB.same(sim.neighbours_at(np.stack(P), radii, skip=skip), before) and NB.same(sim.neighbours_of(np.arange(16), h=400), bodies_before), what

    with gpu.Simulation(n, soft=soft) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE, "before the first upload"
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        assert lib.murbnbr_at(None, 20, *[fp(x) for x in P], None, None, 1.0, off.ctypes.data_as(_up), None, None, 0) == E_INVALID, "no context"
        assert (idx == -7).all() and (off == 0).all()
        sim.upload(s)
        before = sim.neighbours_at(np.stack(P), radii, skip=skip)
        bodies_before = sim.neighbours_of(np.arange(16), h=400)
        total = int(before[0][-1])
        assert 20 < total < 20 * n
        refused(E_INVALID, at(pos=[None, fp(P[1]), fp(P[2])]), "one position array missing")
        refused(E_INVALID, at(offsets=None), "no offsets")
        refused(E_INVALID, of([0, 1], offsets=None), "no offsets")
        refused(E_INVALID, of(None, count=3), "all bodies, but count != n")
        for bad in (np.nan, np.inf, -np.inf):
            for arr in P:
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate of {bad}")
        for bad in (-1.0, -np.float32(1e-30), np.nan, np.inf, -np.inf):
            hh = radii.copy()
            hh[1] = bad
            refused(E_INVALID, at(h=hh), f"a radius of {bad}")
            refused(E_INVALID, of([0, 1], h=hh), f"a radius of {bad} for a body")
            refused(E_INVALID, at(h=None, h_all=bad), f"h_all = {bad}")
            refused(E_INVALID, of([0, 1], h_all=bad), f"h_all = {bad} for bodies")
        for bad in (-2, n, 2 ** 31 - 1):
            sk = skip.copy()
            sk[19] = bad
            refused(E_INVALID, at(sk=sk), f"skip entry {bad}")
        for bad in (-1, n, -2 ** 31):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
        # capacity one short of the total: complete offsets, the arrays untouched
        off[:] = 0
        refused(E_INVALID, at(capacity=total - 1), "capacity one short")
        assert np.array_equal(off, before[0])
        for key, value in (("list_entries", 15), ("list_entries", -1), ("list_entries", (1 << 30) + 1), ("field_chunks", 2), ("nope", 0)):
            assert code_of(gpu, lambda: sim.set_neighbour_option(key, value)) == E_INVALID
        assert sim.neighbour_option("list_entries") == 1 << 26
        assert NB.same(sim.neighbours_at(np.stack(P), radii, skip=skip), before), "refused options"
        # and the calls that are allowed
        off[:] = 0
        assert at(capacity=total) == 0 and np.array_equal(off, before[0])
        assert np.array_equal(idx[:total], before[1]) and np.array_equal(bits(r2[:total]), bits(before[2])) and (idx[total:] == -7).all()
        assert at(sk=None, h=None, h_all=400.0) == 0 and np.array_equal(off, before[0]), "h NULL: h_all for every point"
        assert of([n - 1, 0]) == 0
        assert lib.murbnbr_at(sim._h, 20, *[fp(x) for x in P], None, fp(radii), 0.0, off.ctypes.data_as(_up), ip(idx), None, 20 * n) == 0, "r2 may be NULL alone"
        assert lib.murbnbr_at(sim._h, 20, *[fp(x) for x in P], None, fp(radii), np.nan, off.ctypes.data_as(_up), None, None, 0) == 0, "h given: h_all is not read"


def test_open_block_and_two_shards_are_refused(gpu):
    s, soft = plummer()

    def run(probe):
        with make_sim(gpu, s, soft, g=1.0, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, lambda: sim.neighbours_of(h=0.2)) == E_STATE
                assert code_of(gpu, lambda: sim.neighbours_at(np.zeros((3, 2), np.float32), 1.0, lists=False)) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(x) for x in sim.neighbours_of(h=0.2)]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    d, soft_d, _, _ = dense()
    with gpu.Simulation(N, soft=soft_d, devices=[0, 0]) as sim:
        sim.upload(d)
        assert code_of(gpu, lambda: sim.neighbours_of(h=1)) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the count and fill sweep launches as spans of the kind "nbr": 40 points under "field_batch" 16 are
    three launches, so the count-only call adds 3, and the call with lists 3 more for its own count pass and one per range of the
    fill pass (3 under the default "list_entries"; under 16, one per point with a list, every point having one at this h);
    outside the force_* figures and the field's and knn's spans."""
    s, soft = NR.lattice(600)

    def run(level, entries, calls):
        with make_sim(gpu, s, soft, field_batch=16, list_entries=entries) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if calls > 0:
                sim.neighbours_of(np.arange(40), h=1e4, lists=False)
            if calls > 1:
                sim.neighbours_of(np.arange(40), h=1e4)
            sim.field_of([0, 1])
            return {k: sim.info(k) for k in ("span_nbr_count", "span_nbr_ms_avg", "span_field_count", "span_knn_count", "force_launches")}

    none, counts, lists, cut = run(2, 0, 0), run(2, 0, 1), run(2, 0, 2), run(2, 16, 2)
    assert none["span_nbr_count"] == 0 == none["span_nbr_ms_avg"]
    assert counts["span_nbr_count"] == 3 and counts["span_nbr_ms_avg"] > 0
    assert lists["span_nbr_count"] == 3 + 3 + 3 + 3 and cut["span_nbr_count"] == 3 + 3 + 3 + 40
    for r in (counts, lists, cut):
        assert r["span_field_count"] == none["span_field_count"] == 1 and r["span_knn_count"] == 0
        assert r["force_launches"] == none["force_launches"] >= 1
    assert run(1, 0, 2)["span_nbr_count"] == 0


# ---------------------------------------------------------------------------------------------------------------------- 9. layers
def test_host_mirror(gpu):
    """HostSim.neighbours_of(h) (SimulationNBodyHIP::neighboursOf) equals Simulation.neighbours_of(h=h) on the same bodies, at a
    radius that gives a mean count of a few (from the median 6th-neighbour distance); and fof_groups takes its lists."""
    n, soft = 2049, 2e8
    with gpu.HostSim(n, "galaxy", soft, 3600.0) as host:
        s = host.state()
        with make_sim(gpu, s, np.float32(soft)) as sim:
            _, kr2 = sim.knn_of(k=6)
            h = float(np.sqrt(np.median(kr2[:, 5].astype(np.float64)) - soft * soft))
            want = sim.neighbours_of(h=h)
        offsets, idx = host.neighbours_of(h)
        empty = host.neighbours_of(0.0)
    assert np.array_equal(offsets, want[0]) and np.array_equal(idx, want[1])
    mean = int(offsets[-1]) / n
    print(f"galaxy n={n}: h = {h:.3e}, mean count {mean:.1f}")
    assert 2 < mean < 60
    assert int(empty[0][-1]) == 0 and empty[1].size == 0
    label = gpu.fof_groups(offsets, idx)
    assert (label[idx] == np.repeat(label, np.diff(offsets.astype(np.int64)))).all(), "linked bodies carry one label"

"""MI355X: pair separations (include/murbsep.h) through the C ABI, the Python interface and the plugin.  The histograms exactly
against tests/helpers/sep_ref.py on integer lattices and against the library's own r2 on a Plummer sphere, the sums against fp64
within the derived bound, both under every chunk count and two launch cuts, masks against a context of the members alone, the
mean separation and Q, the calls as observers, and the refused calls."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import knn_ref as K           # noqa: E402
import mst_ref as MR          # noqa: E402
import nearest_ref as NR      # noqa: E402
import sep_ref as R           # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
SHAPES = (1, 2, 127, 129, 511, 513, 2047, 2049)   # both sides of a lane step, a tile and four tiles
_fp, _ip, _dp, _bp, _qp = (C.POINTER(t) for t in (C.c_float, C.c_int, C.c_double, C.c_ubyte, C.c_ulonglong))
LATTICE_BINS = ((0, 0, 10), (0, 2, 80), (4, 6, 1022))      # edges at the powers of two, where the lattices' pairs sit
PLUMMER_BINS = ((-20, 4, 480), (-6, 0, 1), (-3, 6, 700))


def make_sim(gpu, s, soft, g=1.0, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft, g=g)
    for k, v in opts.items():
        (sim.set_field_option if k in gpu.FIELD_OPTIONS else sim.set_option)(k, v)
    sim.upload(s)
    return sim


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.int32, 8: np.int64}[x.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def tiles_of(n):
    return (n + 511) // 512


def settings(n):
    """Every "field_chunks" from 1 to the tile count, each with the default "field_batch" and with 16 (several launches)."""
    return [dict(field_chunks=c, **batch) for c in range(1, tiles_of(n) + 1) for batch in ({}, {"field_batch": 16})]


@lru_cache(maxsize=None)
def fixture(kind, n):
    """(state, soft, integer positions (3, n) or None for the Plummer sphere, which is used with soft = 0).  Do not modify."""
    if kind == "plummer":
        s, _ = K.plummer(n)
        return s, np.float32(0.0), None
    if kind == "lattice":
        s, soft = NR.lattice(n)
        return s, soft, np.stack([s[k].astype(np.int64) for k in ("qx", "qy", "qz")])
    return MR.tie_grid(n) if kind == "grid" else NR.dense_lattice(n)


@lru_cache(maxsize=None)
def lists(n):
    """{count: listed bodies}: 1, 15, 17 and n + 5 bodies, drawn with repeats.  Do not modify."""
    rng = np.random.default_rng(n)
    return {c: rng.integers(0, n, c).astype(np.int32) for c in sorted({1, 15, 17, n + 5})}


@lru_cache(maxsize=None)
def mask_of(n):
    m = np.random.default_rng(n + 1).random(n) < 0.4
    m[0] = True   # never empty
    return m


@lru_cache(maxsize=None)
def points_of(kind, n):
    """17 integer points of the caller's: random ones, and copies of three bodies' positions (r = 0, one "below" entry each)."""
    q = fixture(kind, n)[2]
    rng = np.random.default_rng(n + 2)
    p = rng.integers(int(q.min()), int(q.max()) + 2, size=(3, 17)).astype(np.int64)
    for col, body in zip((0, 5, 16), (0, n // 2, n - 1)):
        p[:, col] = q[:, body]
    return p


@lru_cache(maxsize=None)
def lattice_d2(kind, n):
    return R.d2_lattice(fixture(kind, n)[2])


@lru_cache(maxsize=None)
def lattice_reference(kind, n, what, params):
    """The restatement's (hist, out4) of one call on a lattice, computed once.  what: "all", "masked", a count of lists(n), or "at"."""
    q = fixture(kind, n)[2]
    if what == "at":
        return R.histogram(R.d2_lattice(q, points_of(kind, n)), *params, member=mask_of(n))
    d2 = lattice_d2(kind, n)
    if what == "all":
        return R.histogram(d2, *params, own=np.arange(n))
    if what == "masked":
        return R.histogram(d2, *params, member=mask_of(n), own=np.arange(n))
    who = lists(n)[what]
    return R.histogram(d2[who], *params, member=mask_of(n), own=who)


def check_counts(got, want, what):
    hist, out4 = got
    assert hist.dtype == np.uint64 and np.array_equal(hist, want[0]), (what, np.nonzero(hist != want[0])[0][:5])
    assert out4 == want[1], (what, out4, want[1])
    assert out4["below"] + int(hist.sum()) + out4["above"] == out4["pairs"], what


def check_sums(got, want, bound, what):
    """Within the derived relative bound of the fp64 sums; a sum of nothing is +0 exactly."""
    assert got.dtype == np.float64 and got.shape == want.shape
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), what
    err = np.abs(got[~zero] - want[~zero]) / want[~zero]
    if err.size:
        print(what, f"largest relative error {err.max():.3e} of {bound:.3e} allowed")
        assert err.max() <= bound, (what, err.max(), bound)


CASES = [(kind, n) for kind in ("lattice", "grid") for n in SHAPES] + [("dense", 2049)]


# ------------------------------------------------------------------------------------------------- 1. lattices: exact histograms
@pytest.mark.parametrize("kind,n", CASES)
def test_lattices_against_the_restatement(gpu, kind, n):
    """On integer lattices every d2 is exact, so the bins are decided exactly: all bodies, a mask of 40 %, lists of 1, 15, 17 and
    n + 5 bodies with repeats under the mask, and 17 points of the caller's (three on bodies), for three sets of bins, under every
    chunk count and both launch cuts.  The sums lie within the derived bound of fp64 and do not depend on the launch cut, the
    other points of the call, the histogram, or on whether the point is given by index or by position."""
    s, soft, q = fixture(kind, n)
    mask, pts = mask_of(n), points_of(kind, n)
    want_all, want_masked = R.sums64(R.positions(s)), R.sums64(R.positions(s), member=mask)
    want_at = R.sums64(R.positions(s), points=pts.astype(np.float32), member=mask)
    by_chunks = {}
    for opts in settings(n):
        bound = R.sum_bound(tiles_of(n), opts["field_chunks"])
        with make_sim(gpu, s, soft, **opts) as sim:
            plain = sim.separation_of()
            assert plain[1] is None and plain[2] is None
            check_sums(plain[0], want_all, bound, (opts, "all"))
            masked = sim.separation_of(member=mask)[0]
            check_sums(masked, want_masked, bound, (opts, "masked"))
            for params in LATTICE_BINS:
                total, hist, out4 = sim.separation_of(bins=params)
                check_counts((hist, out4), lattice_reference(kind, n, "all", params), (opts, params, "all"))
                assert same(total, plain[0]), "the sums with and without a histogram"
                assert np.all(hist % np.uint64(2) == 0) and out4["below"] % 2 == 0 and out4["above"] % 2 == 0, "every pair twice"
                total, hist, out4 = sim.separation_of(member=mask, bins=params)
                check_counts((hist, out4), lattice_reference(kind, n, "masked", params), (opts, params, "masked"))
                assert same(total, masked)
                for count, who in lists(n).items():
                    total, hist, out4 = sim.separation_of(who, member=mask, bins=params)
                    check_counts((hist, out4), lattice_reference(kind, n, count, params), (opts, params, count))
                    assert same(total, masked[who]), "a point's bits do not depend on the other points of the call"
                total, hist, out4 = sim.separation_at(pts.astype(np.float32), member=mask, bins=params)
                check_counts((hist, out4), lattice_reference(kind, n, "at", params), (opts, params, "at"))
            check_sums(total, want_at, bound, (opts, "at"))
            assert same(sim.separation_at(pts.astype(np.float32), member=mask)[0], total)
            assert same(sim.separation_at(R.positions(s))[0], plain[0]), "by position and by index"
        first = by_chunks.setdefault(opts["field_chunks"], (plain[0], masked, total))
        assert all(same(a, b) for a, b in zip(first, (plain[0], masked, total))), ("field_batch changes no bit", opts)


# --------------------------------------------------------------------------------------------- 2. Plummer sphere, soft = 0
def library_d2(sim, n):
    """Every ordered pair's r2 from neighbours_of with a radius that holds everything: with soft = 0 the same expression."""
    offsets, idx, r2 = sim.neighbours_of(h=1e6)
    assert len(idx) == n * (n - 1) and np.array_equal(np.diff(offsets.astype(np.int64)), np.full(n, n - 1))
    return idx.reshape(n, n - 1) if n > 1 else idx.reshape(n, 0), r2.reshape(n, n - 1) if n > 1 else r2.reshape(n, 0)


@pytest.mark.parametrize("n", SHAPES)
def test_plummer_against_the_librarys_own_r2(gpu, n):
    """In a context with soft = 0 the histogram equals the binning of neighbours_of's r2 exactly, for all bodies and for lists
    under a mask; with all bodies as points and as S every count is even; the bits are the same under every chunk count and both
    launch cuts.  The sums against fp64 within the derived bound."""
    s, soft, _ = fixture("plummer", n)
    mask = mask_of(n)
    want_all, want_masked = R.sums64(R.positions(s)), R.sums64(R.positions(s), member=mask)
    wanted, by_chunks = {}, {}
    for opts in settings(n):
        bound = R.sum_bound(tiles_of(n), opts["field_chunks"])
        with make_sim(gpu, s, soft, **opts) as sim:
            if not wanted:
                idx, d2 = library_d2(sim, n)
                for params in PLUMMER_BINS:
                    k = R.bin_of(d2, *params)
                    wanted[params] = k
                wanted["in"] = mask[idx]
            plain, masked = sim.separation_of()[0], sim.separation_of(member=mask)[0]
            check_sums(plain, want_all, bound, (opts, "all"))
            check_sums(masked, want_masked, bound, (opts, "masked"))
            for params in PLUMMER_BINS:
                nb, k = params[2], wanted[params]
                total, hist, out4 = sim.separation_of(bins=params)
                want = (np.bincount(k[(k >= 0) & (k < nb)], minlength=nb).astype(np.uint64),
                        {"pairs": n * (n - 1), "below": int((k < 0).sum()), "above": int((k >= nb).sum())})
                check_counts((hist, out4), want, (opts, params, "all"))
                assert same(total, plain)
                assert np.all(hist % np.uint64(2) == 0) and out4["below"] % 2 == 0 and out4["above"] % 2 == 0, "every pair twice"
                for count, who in lists(n).items():
                    kk = k[who][wanted["in"][who]]
                    want = (np.bincount(kk[(kk >= 0) & (kk < nb)], minlength=nb).astype(np.uint64),
                            {"pairs": int(kk.size), "below": int((kk < 0).sum()), "above": int((kk >= nb).sum())})
                    total, hist, out4 = sim.separation_of(who, member=mask, bins=params)
                    check_counts((hist, out4), want, (opts, params, count))
                    assert same(total, masked[who])
        first = by_chunks.setdefault(opts["field_chunks"], (plain, masked))
        assert same(first[0], plain) and same(first[1], masked), ("field_batch changes no bit", opts)
    if n >= 513:
        spread = wanted[PLUMMER_BINS[0]]
        assert len(set(spread[(spread >= 0) & (spread < PLUMMER_BINS[0][2])])) > 100, "the pairs fill many bins"


# ------------------------------------------------------------------------------------------------------------- 3. the mask
@pytest.mark.parametrize("kind,n", [("lattice", 513), ("grid", 2047), ("dense", 2049), ("plummer", 2049)])
def test_mask_against_a_context_of_the_members(gpu, kind, n):
    """Under a mask of 40 % the histogram of the members against the members equals that of a second context that holds the
    members alone, count for count; both contexts' sums lie within the bound of the same fp64 values.  A mask of one member and of
    none: no pair."""
    s, soft, _ = fixture(kind, n)
    mask = mask_of(n)
    who = np.flatnonzero(mask).astype(np.int32)
    params = PLUMMER_BINS[0] if kind == "plummer" else LATTICE_BINS[1]
    want = R.sums64(R.positions(s)[:, mask])
    with make_sim(gpu, s, soft, field_chunks=tiles_of(n)) as sim:
        total, hist, out4 = sim.separation_of(who, member=mask, bins=params)
        one = np.zeros(n, bool)
        one[n // 2] = True
        single = sim.separation_of([n // 2, 0], member=one, bins=params)
        nobody = sim.separation_of(member=np.zeros(n, bool), bins=params)
    sub_n = len(who)
    with make_sim(gpu, {k: v[who] for k, v in s.items()}, soft, field_chunks=tiles_of(sub_n)) as sub:
        sub_total, sub_hist, sub_out4 = sub.separation_of(bins=params)
    assert np.array_equal(hist, sub_hist) and out4 == sub_out4 and out4["pairs"] == sub_n * (sub_n - 1)
    check_sums(total, want, R.sum_bound(tiles_of(n), tiles_of(n)), "masked")
    check_sums(sub_total, want, R.sum_bound(tiles_of(sub_n), tiles_of(sub_n)), "members alone")
    assert single[2]["pairs"] == 1 and single[2]["below"] + int(single[1].sum()) + single[2]["above"] == 1, "body 0 against the member"
    assert single[0][0] == 0.0 and single[0][1] > 0.0
    assert nobody[2] == {"pairs": 0, "below": 0, "above": 0} and not nobody[1].any() and not nobody[0].any()


# ------------------------------------------------------------------------------------------------- 4. mean separation and Q
@pytest.mark.parametrize("kind,n", [("plummer", 2), ("plummer", 513), ("plummer", 2049), ("grid", 2047)])
def test_mean_separation_and_q(gpu, kind, n):
    """mean_separation and q_parameter against the restatement over the same tree, for all bodies and under a mask; NaN for fewer
    than 2 members."""
    s, soft, _ = fixture(kind, n)
    mask = mask_of(n) if n > 2 else None
    with make_sim(gpu, s, soft) as sim:
        bound = R.sum_bound(tiles_of(n), int(sim.field_option("field_chunks")))
        for member in (None, mask) if mask is not None else (None,):
            got = sim.mean_separation(member)
            want = R.mean_separation(s, member)
            assert abs(got - want) <= bound * want, (got, want)
            q = sim.q_parameter(member)
            ref = R.q_parameter(s, sim.spanning_tree(member)["mean_length"], member)
            members = n if member is None else int(np.sum(member))
            assert q["members"] == members and q["radius"] == ref[3]
            assert abs(q["m_bar"] - ref[1]) <= 1e-14 * ref[1] and abs(q["s_bar"] - ref[2]) <= (bound + 1e-14) * ref[2]
            assert abs(q["q"] - ref[0]) <= (2 * bound + 1e-13) * ref[0]
            print(kind, n, "members", members, f"s_bar {q['s_bar']:.4f} m_bar {q['m_bar']:.4f} Q {q['q']:.4f}")
        one = np.zeros(n, bool)
        one[0] = True
        assert np.isnan(sim.mean_separation(one)) and np.isnan(sim.q_parameter(one)["q"]) and sim.q_parameter(one)["members"] == 1
        assert np.isnan(sim.mean_separation(np.zeros(n, bool)))


def test_shell_density_about_the_density_centre(gpu):
    """A one-point separation_at about the density centre of a Plummer sphere: the counts are those of numpy over the same
    library r2, and the shell density falls outwards."""
    n = 2049
    s, soft, _ = fixture("plummer", n)
    params = (-8, 1, 24)      # r from 1/16 to 4, two bins per octave of d2
    with make_sim(gpu, s, soft) as sim:
        centre = np.asarray(sim.density_centre()["x"], np.float32)
        total, hist, out4 = sim.separation_at(centre.reshape(3, 1), bins=params)
        _, _, r2 = sim.neighbours_at(centre.reshape(3, 1), h=1e6)
    k = R.bin_of(r2, *params)
    assert np.array_equal(hist, np.bincount(k[(k >= 0) & (k < params[2])], minlength=params[2]).astype(np.uint64))
    assert out4 == {"pairs": n, "below": int((k < 0).sum()), "above": int((k >= params[2]).sum())}
    rho = gpu.shell_density(hist, gpu.separation_edges(*params)[1])
    assert rho[4:8].mean() > 10 * rho[20:24].mean() > 0, rho      # r in 1/8 .. 1/4 against 2 .. 4 of a sphere of scale 1


# -------------------------------------------------------------------------------------------------- 5. observer and refusals
@pytest.mark.parametrize("nearest", (0, 1))
def test_observers_leave_the_run_alone(gpu, nearest):
    """step; separation_of; separation_at; step under "integrator" 2: every later bit (state, acc, nearest(), knn_of,
    neighbours_of, potential_of) is what it is without the read-outs, and each returns the bits it returns as the only observer."""
    n = 1025
    s, _ = K.plummer(n)
    soft = np.float32(1e-3)
    mask = mask_of(n)
    pts = np.stack([s[k][:40] + np.float32(0.25) for k in ("qx", "qy", "qz")])
    seen = {}

    def run(probe):
        with make_sim(gpu, s, soft, integrator=2, nearest=nearest) as sim:
            sim.steps(2.0 ** -10, 1)
            if probe in ("both", "of"):
                seen[probe, "of"] = sim.separation_of(member=mask, bins=PLUMMER_BINS[0])
            if probe in ("both", "at"):
                seen[probe, "at"] = sim.separation_at(pts, bins=PLUMMER_BINS[2])
            sim.steps(2.0 ** -10, 1)
            sim.sync()
            st = sim.state()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.knn_of(k=3)) + list(sim.neighbours_of(h=0.2))
            rec.append(sim.potential_of(member=mask))
            if nearest:
                rec += list(sim.nearest())
            return [bits(x) for x in rec]

    plain = run(None)
    for probe in ("both", "of", "at"):
        assert all(np.array_equal(x, y) for x, y in zip(plain, run(probe))), probe
    for kind in ("of", "at"):
        a, b = seen["both", kind], seen[kind, kind]
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2], kind


def test_refusals(gpu):
    n = 600
    s, soft, _ = fixture("plummer", n)
    lib = gpu.lib()
    total, hist, out4 = np.zeros(n, np.float64), np.zeros(16, np.uint64), np.zeros(4, np.uint64)
    px, py, pz = (np.ascontiguousarray(s[k][:8]) for k in ("qx", "qy", "qz"))
    ptr = lambda x, t: x.ctypes.data_as(t) if x is not None else None      # noqa: E731
    keep = {}

    def of(bodies=None, count=None, out_s=total, params=(0, 0, 16), out_h=hist, out_4=out4, ctx=True):
        b = None if bodies is None else np.ascontiguousarray(bodies, np.int32)
        count = (n if b is None else len(b)) if count is None else count
        keep["b"] = b
        return lib.murbsep_of(sim._h if ctx else None, count, ptr(b, _ip), None, ptr(out_s, _dp), *params, ptr(out_h, _qp), ptr(out_4, _qp))

    def at(x=px, y=py, z=pz, out_s=total, params=(0, 0, 16), out_h=hist, out_4=out4, ctx=True):
        return lib.murbsep_at(sim._h if ctx else None, 8, ptr(x, _fp), ptr(y, _fp), ptr(z, _fp), None, ptr(out_s, _dp), *params,
                              ptr(out_h, _qp), ptr(out_4, _qp))

    def refused(code, rc, what):
        """The call returned its code, wrote nothing, and the following calls return what they returned before."""
        assert rc == code, (what, rc)
        assert np.all(total == -7.0) and np.all(hist == 77) and np.all(out4 == 77), what
        again = sim.separation_of(bins=(-20, 4, 480))
        assert same(again[0], before[0]) and same(again[1], before[1]) and again[2] == before[2], what

    with gpu.Simulation(n, soft=soft, g=1.0) as sim:
        assert of() == E_STATE and of([0, 1]) == E_STATE and at() == E_STATE, "before the first upload"
        assert of([0], count=0) == 0 and lib.murbsep_at(sim._h, 0, None, None, None, None, None, 0, 0, 0, None, None) == 0, "count 0"
        assert of(ctx=False) == E_INVALID and at(ctx=False) == E_INVALID, "no context"
        sim.upload(s)
        before = sim.separation_of(bins=(-20, 4, 480))
        total[:], hist[:], out4[:] = -7.0, 77, 77
        for call, name in ((of, "of"), (at, "at")):
            refused(E_INVALID, call(out_s=None, params=(0, 0, 0)), name + ": no sum and no histogram")
            refused(E_INVALID, call(out_h=None), name + ": no hist")
            refused(E_INVALID, call(out_4=None), name + ": no out4")
            for params in ((-127, 0, 16), (128, 0, 1), (0, -1, 16), (0, 7, 16), (0, 0, -1), (0, 0, 1023), (0, 0, 128), (127, 6, 64)):
                refused(E_INVALID, call(params=params), name + f": parameters {params}")
        refused(E_INVALID, of(count=3), "all bodies, but count != n")
        for bad in (-1, n, -2 ** 31, 2 ** 31 - 1):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
        for k in range(3):
            args = [px, py, pz]
            args[k] = None
            refused(E_INVALID, at(*args), "a NULL position array")
            for bad in (np.nan, np.inf, -np.inf):
                args[k] = px.copy()
                args[k][5] = bad
                refused(E_INVALID, at(*args), f"coordinate {bad}")
        assert of([n - 1, 0, 0]) == 0 and of(out_s=None) == 0 and at() == 0 and at(params=(0, 0, 0), out_h=None, out_4=None) == 0
        assert out4[0] == 8 * n and out4[1] + hist.sum() + out4[2] == out4[0]
        with pytest.raises(ValueError):
            sim.separation_of(member=np.ones(n - 1, bool))
        with pytest.raises(ValueError):
            sim.separation_at([px, py])
        with pytest.raises(ValueError):
            sim.separation_of(bins=(0, 0, 0))


def test_open_block_and_two_shards_are_refused(gpu):
    n = 600
    s, _ = K.plummer(n)
    soft = np.float32(1e-3)
    pts = np.zeros((3, 2), np.float32)

    def code_of(call):
        with pytest.raises(gpu.MurbHipError) as e:
            call()
        return e.value.code

    def run(probe):
        with make_sim(gpu, s, soft, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(sim.separation_of) == E_STATE and code_of(lambda: sim.separation_at(pts, bins=(0, 0, 4))) == E_STATE
                assert code_of(sim.mean_separation) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(sim.separation_of()[0])]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    with gpu.Simulation(n, soft=soft, g=1.0, devices=[0, 0]) as sim:
        sim.upload(s)
        assert code_of(sim.separation_of) == E_STATE and code_of(lambda: sim.separation_at(pts)) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the sweep launches as spans of the kind "sep" (40 points under "field_batch" 16: three launches; all
    600 bodies: 38), outside the force_* figures and the other read-outs' spans."""
    s, soft, _ = fixture("plummer", 600)

    def run(level, sep):
        with make_sim(gpu, s, soft, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if sep:
                sim.separation_of(np.arange(40))
                sim.separation_of(bins=(-20, 4, 480))
            sim.knn_of([0, 1], k=1)
            return {k: sim.info(k) for k in ("span_sep_count", "span_sep_ms_avg", "span_knn_count", "span_pot_count", "span_mst_count",
                                             "force_launches")}

    with_it, without = run(2, True), run(2, False)
    assert with_it["span_sep_count"] == 3 + 38 and with_it["span_sep_ms_avg"] > 0
    assert without["span_sep_count"] == 0 == without["span_sep_ms_avg"] and with_it["span_pot_count"] == 0 == with_it["span_mst_count"]
    assert with_it["span_knn_count"] == without["span_knn_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)["span_sep_count"] == 0


# ------------------------------------------------------------------------------------------------------------------ 6. plugin
def test_plugin_mean_separation(gpu):
    """HostSim.mean_separation() (SimulationNBodyHIP::meanSeparation) equals Simulation.mean_separation() of the same bodies bit
    for bit, after an iteration too, and the fp64 value within the bound."""
    n, soft, dt = 2049, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt) as host:
        for _ in range(2):
            st = host.state()
            got = host.mean_separation()
            with gpu.Simulation(n, soft=soft) as sim:
                sim.upload(st)
                want = sim.mean_separation()
            assert got == want and got > 0
            ref = R.mean_separation(st)
            assert abs(got - ref) <= R.sum_bound(tiles_of(n), 1) * ref
            print(f"galaxy n={n}: mean separation {got:.6e}")
            host.step(1)

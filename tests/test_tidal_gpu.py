"""GPU: the tidal read-out murbtidal_at / murbtidal_of through the C ABI, the Python interface and the plugin.

Yardstick and bound: tests/helpers/tidal_ref.py (numpy fp64 written from include/murbtidal.h, pinned by tests/test_tidal_host.py
against central differences of the field yardstick).  A point's error is the Frobenius norm of got - fp64 over the symmetric
matrix, scaled by the sum of the Frobenius norms of its pair terms and bounded by C * 2^-24, C = 4 x what the float32 emulation
attains against fp64 on the case's points; it is computed once per case on the CPU, and every check prints the GPU's figure
beside it (pytest -s).  Everything about reproducibility and about the read-out leaving the context alone is differential, bit
for bit."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import field_ref as F         # noqa: E402
import field_wrap as FW       # noqa: E402
import hermite_ref as H       # noqa: E402
import potential_ref as PR    # noqa: E402
import tidal_ref as T         # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
COUNTS = (1, 17, 33)
# One point, one term, no sum: what the float32 emulation attains on that single sample is luck (0.2 to 4 x 2^-24 over the 16
# sources), so the bound comes from the formats instead.  v_rsq_f32 is within 1 ulp: inv (1 + e) with |e| <= 2^-23.  The term
# G m (3 d_a d_b inv^5 - delta_ab inv^3) then moves by s e (15 n_a n_b - 3 delta_ab), whose Frobenius norm over that of the term
# is sqrt((225 x^2 - 90 x + 27) / (9 x^2 - 6 x + 3)) |e| with x = |n|^2 <= 1: at most sqrt(27) |e| = 10.4 x 2^-24.  Roundings
# of 2^-25 each: r2's three fused steps (halved by the root), inv2, gi, s, s3, n, t and the last fused step: 4.25 x 2^-24 of a
# component, so of the norm at most.  14.65, taken as 16.
ONE_TERM_C = 16.0
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)


def make_sim(gpu, s, soft=F.SOFT, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft)
    for k, v in opts.items():
        (sim.set_field_option if k in gpu.FIELD_OPTIONS else sim.set_option)(k, v)
    sim.upload(s)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def first(x, count):
    return None if x is None else x[..., :count]


def plus_zero(got, k=None):
    """Every component (of point k) is +0.0f."""
    return all((got[q] == 0).all() and not np.signbit(got[q]).any() for q in T.KEYS) if k is None else \
        all(got[q][k] == 0 and not np.signbit(got[q][k]) for q in T.KEYS)


@lru_cache(maxsize=None)
def case(n):
    """(state, {name: (points, skip, fp64 reference, C)}) of the dense n-body system, 33 points a set: CPU only."""
    s = F.system(n)
    sets = {}
    for name, (p, _, skip) in (("bodies", F.body_points(s, np.arange(33) % n)), ("midpoints", F.midpoints(s, 33))):
        ref, c = T.bound_of(p, skip, s, F.SOFT)
        sets[name] = (p, skip, ref, c)
    return s, sets


# ------------------------------------------------------------------------------------------------- 1. sizes, counts, chunk cuts
@pytest.mark.parametrize("n", [1, 2, 63, 513, 1025, 2049])
def test_sizes_counts_chunks(gpu, n):
    """One to five layout tiles with and without padding, counts around the group of 16, "field_chunks" 0 (the rule), 1, 2 and
    10^6 (clamped to one per tile); the bodies themselves (tidal_of, and tidal_at with the bodies' own positions and skip entries:
    the same bits) and midpoints of body pairs with nobody skipped."""
    s, sets = case(n)
    tiles = -(-n // 512)
    with make_sim(gpu, s) as sim:
        for option in (0, 1, 2, 10 ** 6):
            sim.set_field_option("field_chunks", option)
            assert sim.field_option("field_chunks") == (min(option, tiles) if option else 1)
            for name, (p, skip, ref, c) in sets.items():
                whole = sim.tidal_at(p, skip)
                for count in COUNTS:
                    got = sim.tidal_at(first(p, count), first(skip, count))
                    T.check(got, ref, c, f"n={n} field_chunks={option} {name} count={count}", rows=np.arange(count))
                    assert all(np.array_equal(T.bits(got[k]), T.bits(whole[k][:count])) for k in T.KEYS), "the count changed a point's bits"
                    if name == "bodies":
                        assert T.same_bits(sim.tidal_of(skip[:count]), got), "tidal_of is tidal_at at the bodies' own positions"
                if n == 1 and name == "bodies":
                    assert plus_zero(whole), "a lone body, itself skipped: +0.0f six times"
        lib = gpu.lib()
        pts = [np.ascontiguousarray(x) for x in sets["midpoints"][0]]
        assert lib.murbtidal_at(sim._h, 33, *[x.ctypes.data_as(_fp) for x in pts], None, *([None] * 6)) == 0, "no outputs: validated, run, 0"


# -------------------------------------------------------------------------------------------------------------- 2. sparse sources
def test_sparse_sources(gpu):
    """Mass at every tile's first and last slot and a few between (potential_ref.SPARSE_SOURCES), then one run per source with
    that source alone massive: the sums are that one body's tensor, at midpoints, at the listed bodies and at a point displaced
    from the source by 10 x soft.  A dropped or doubled j slot, tile edge or lane half is a whole term."""
    s, soft, src = F.sparse_sources()
    n = len(s["m"])
    p, _, skip = F.midpoints(s, 64, stride=11)
    bodies = np.concatenate([src, [1, 510, 513, 1022, 2046]]).astype(np.int32)
    bp, _, bskip = F.body_points(s, bodies)
    ref, c = T.bound_of(p, skip, s, soft)
    bref, bc = T.bound_of(bp, bskip, s, soft)
    with make_sim(gpu, s, soft) as sim:
        for chunks in (1, 2, 5):
            sim.set_field_option("field_chunks", chunks)
            T.check(sim.tidal_at(p), ref, c, f"sparse, all sources, chunks={chunks}: midpoints")
            T.check(sim.tidal_of(bodies), bref, bc, f"sparse, all sources, chunks={chunks}: bodies")
    gm = H._gm(s)
    with gpu.Simulation(n, soft=soft) as sim:
        for k in src:
            one = F.only_source(s, k)
            sim.upload(one)
            ref1, c1 = T.bound_of(p, skip, one, soft)
            got = sim.tidal_at(p)
            T.check(got, ref1, c1, f"sparse, source {k} alone: midpoints")
            assert (T.stack(got)[:3].max(0) > 0).all(), "one body stretches along the line to it"
            bref1, bc1 = T.bound_of(bp, bskip, one, soft)
            gotb = sim.tidal_of(bodies)
            T.check(gotb, bref1, bc1, f"sparse, source {k} alone: bodies")
            assert plus_zero(gotb, int(np.flatnonzero(bodies == k)[0])), "the lone source sees nothing of itself"
            dp = F.displaced(one, k, soft)[0]
            dref = T.tidal_f64(dp, None, one, soft)
            near = sim.tidal_at(dp)
            T.check(near, dref, ONE_TERM_C, f"sparse, source {k} alone: displaced point")
            r2 = 101.0 * float(soft) ** 2      # d = (10 soft, 0, 0): txx = G m (3 d^2 / r2 - 1) r2^(-3/2)
            assert np.isclose(near["txx"][0], gm[k] * (300.0 / 101.0 - 1.0) * r2 ** -1.5, rtol=1e-4)


# ----------------------------------------------------------------------------------------------------------------------- 3. skip
@pytest.mark.parametrize("n", [2, 514])
def test_own_term(gpu, n):
    """potential_ref.own_term_pair: the softening is 1e-4 of the separation, so a body's own term, -G m / soft^3 on the diagonal,
    is 1e12 x the other body's.  tidal_of([k]) is the tensor of the others within the bound, and bit-equal to tidal_at at q_k with
    skip = [k]."""
    s, soft, (a, b) = PR.own_term_pair(n)
    p, _, skip = F.body_points(s, [a, b])
    ref, c = T.bound_of(p, skip, s, soft)
    leaked = T.tidal_f64(p, None, s, soft)
    assert (np.abs(leaked[0][0]) > 1e11 * np.abs(ref[0][0])).all(), "CPU: a leaked own term is (sep / soft)^3 x the pair term"
    with make_sim(gpu, s, soft) as sim:
        got = sim.tidal_of([a, b])
        T.check(got, ref, c, f"own term n={n}: tidal_of")
        assert T.same_bits(sim.tidal_at(p, skip), got)
        for k in (a, b):
            one = sim.tidal_of([k])
            assert all(T.bits(one[q])[0] == T.bits(got[q])[[a, b].index(k)] for q in T.KEYS)
        bare = sim.tidal_at(p)
    assert (np.abs(bare["txx"]) > 1e11 * np.abs(got["txx"])).all(), "without a skip entry the own term counts"


def test_skipped_slot_positions(gpu):
    """n = 1537 (four layout tiles, the last with one body): the skipped slot at both lane halves of a record (0, 1; 510, 511),
    at both ends of a tile (511, 512; 1023, 1024) and at the last real slot, under chunk cuts that put the skipped tile into
    the first, a middle and the last chunk; the points beside the bodies, not on them, in both orders."""
    n = 1537
    s = F.system(n)
    slots = np.array([0, 1, 510, 511, 512, 1023, 1024, n - 1], np.int32)
    p, _, skip = F.body_points(s, slots)
    p = (p + np.float32(0.003)).astype(np.float32)
    ref, c = T.bound_of(p, skip, s, F.SOFT)
    with_it = T.tidal_f64(p, None, s, F.SOFT)
    assert (T.scaled_errors(with_it[0], ref) > 100 * c * T.U24).all(), "CPU: the skipped body's term is far above the bound"
    with make_sim(gpu, s) as sim:
        for chunks in (1, 2, 3, 4):
            sim.set_field_option("field_chunks", chunks)
            cut = FW.cut(n, chunks)
            if chunks == 3:
                assert cut == [(0, 1), (1, 2), (2, 4)] and {int(x) // 512 for x in slots} == {0, 1, 2, 3}
            T.check(sim.tidal_at(p, skip), ref, c, f"skipped slots, chunks={chunks}")
            T.check(sim.tidal_at(p[:, ::-1], skip[::-1]), ref, c, f"skipped slots reversed, chunks={chunks}", rows=np.arange(len(slots))[::-1])


@pytest.mark.parametrize("pair", PR.COINCIDENT_PAIRS)
def test_coincident_bodies_count(gpu, pair):
    """Two bodies at one place, one skipped: the other counts, with -G m / soft^3 on the diagonal.  The exclusion is by slot, not
    by d == 0."""
    s, soft = PR.coincident(pair)
    a, b = pair
    p, _, skip = F.body_points(s, [a, b, a, a])      # the same body listed three times
    ref, c = T.bound_of(p, skip, s, soft)
    gm = H._gm(s)
    assert np.sqrt(3.0) * gm[b] / float(soft) ** 3 > 1e3 * c * T.U24 * ref[1][0], "CPU: the coincident body's term is far above the bound"
    with make_sim(gpu, s, soft) as sim:
        got = sim.tidal_of([a, b, a, a])
        T.check(got, ref, c, f"coincident {pair}")
        assert all(T.bits(got[k])[0] == T.bits(got[k])[2] == T.bits(got[k])[3] for k in T.KEYS), "the same body twice: the same bits"


# ------------------------------------------------------------------------------------------------------------------- 4. company
def test_company(gpu):
    """64 points over the dense 2 049-body system, the first wave's four skipping bodies in four different tiles: every point's
    six results have the same bits alone (so as the first, 16th, 17th and last of a call too), in the call of 64, in the reversed
    call, under "field_batch" 16, 32 and the default, and in a second run — for the default chunk cut, for two chunks and for
    one per tile.  They change with "field_chunks" alone."""
    s, _ = case(2049)
    rng = np.random.default_rng(7)
    p = rng.uniform(0.0, 1.0, (3, 64)).astype(np.float32)
    skip = np.full(64, -1, np.int32)
    skip[:4] = (5, 600, 1100, 1700)
    skip[4:40:3] = rng.integers(0, 2049, 12)
    skip[63] = 2048
    assert len({int(x) // F.TILE for x in skip[:4]}) == 4
    ref, c = T.bound_of(p, skip, s, F.SOFT)
    kept = {}
    for chunks in (0, 2, 5):
        with make_sim(gpu, s, field_chunks=chunks) as sim:
            whole = sim.tidal_at(p, skip)
            T.check(whole, ref, c, f"company, chunks option {chunks}")
            alone = [sim.tidal_at(p[:, k:k + 1], skip[k:k + 1]) for k in range(64)]
            for k in T.KEYS:
                assert np.array_equal(T.bits(np.concatenate([x[k] for x in alone])), T.bits(whole[k])), f"{k}: alone against the call of 64"
            for at in (0, 15, 16, 32):      # point 40 as the first, 16th, 17th and last of a call of 33 others
                order = np.concatenate([np.arange(at), [40], np.arange(at, 32)])
                got = sim.tidal_at(p[:, order], skip[order])
                assert all(T.bits(got[k])[at] == T.bits(whole[k])[40] for k in T.KEYS), f"point 40 at place {at}"
            rev = sim.tidal_at(p[:, ::-1], skip[::-1])
            assert all(np.array_equal(T.bits(rev[k][::-1]), T.bits(whole[k])) for k in T.KEYS), "the call reversed"
            other = sim.tidal_at(p, np.roll(skip, 7))      # among other skip entries: the points that keep theirs keep their bits
            same = np.flatnonzero(np.roll(skip, 7) == skip)
            assert len(same) > 20 and all(np.array_equal(T.bits(other[k][same]), T.bits(whole[k][same])) for k in T.KEYS)
            for batch in (16, 32, 0):
                sim.set_field_option("field_batch", batch)
                assert T.same_bits(sim.tidal_at(p, skip), whole), f"field_batch {batch}"
        with make_sim(gpu, s, field_chunks=chunks) as again:
            assert T.same_bits(again.tidal_at(p, skip), whole), "a second run"
        kept[chunks] = whole
    assert not T.same_bits(kept[0], kept[5]) and not T.same_bits(kept[2], kept[5]), "the chunk cut is the fp32 sums' cut"


# --------------------------------------------------------------------------------------------------------------------- 5. trace
@pytest.mark.parametrize("n", [513, 2049])
def test_trace(gpu, n):
    """txx + tyy + tzz against -3 soft^2 sum G m inv^5 in fp64, at far points (every term nearly the same matrix) and at midpoints
    with soft = 2^-20 (the trace is nearly 0): within three times the case's bound of the scaling sum (three components, each
    within the bound)."""
    s = F.system(n)
    for name, p, soft in (("far", F.far_points(33)[0], F.SOFT), ("midpoints, soft 2^-20", F.midpoints(s, 33)[0], np.float32(2.0 ** -20))):
        ref, c = T.bound_of(p, None, s, soft)
        with make_sim(gpu, s, soft) as sim:
            got = sim.tidal_at(p)
        T.check(got, ref, c, f"n={n} {name}")
        e = T.trace_errors(got, ref).max() / T.U24
        print(f"n={n} {name}: trace off by {e:.2f} x 2^-24 of the scaling sum (bound {3 * c:.2f}); |trace| / scaling sum = {np.abs(ref[2] / ref[1]).max():.2e}")
        assert e <= 3 * c


# -------------------------------------------------------------------------------------------------------------- 6. unit scaling
def test_unit_scaling(gpu):
    """n = 513: lengths x 2^4, masses x 2^-6, soft x 2^4: every result's bits are the unscaled ones x 2^(-6 - 3 * 4) = 2^-18."""
    s, sets = case(513)
    p = sets["midpoints"][0]
    bodies = np.arange(40, dtype=np.int32) * 11
    t = {k: v.copy() for k, v in s.items()}
    for k in F.Q:
        t[k] = (t[k] * np.float32(16.0)).astype(np.float32)
    t["m"] = (t["m"] * np.float32(2.0 ** -6)).astype(np.float32)
    with make_sim(gpu, s) as sim:
        want = [sim.tidal_at(p), sim.tidal_of(bodies)]
    with make_sim(gpu, t, np.float32(16.0) * F.SOFT) as sim:
        got = [sim.tidal_at((p * np.float32(16.0)).astype(np.float32)), sim.tidal_of(bodies)]
    for w, g in zip(want, got):
        for k in T.KEYS:
            assert np.isfinite(w[k]).all() and (np.abs(w[k]) > 2.0 ** -100).all()
            assert np.array_equal(T.bits(g[k]), T.bits(w[k] * np.float32(2.0 ** -18))), k


# -------------------------------------------------------------------------------------------------------- 7. beyond one grid pass
@pytest.fixture(scope="module")
def grid(gpu):
    """Workgroups of the sweep on the device at hand: the field sweep's, 4 per CU."""
    with gpu.Simulation(16, soft=F.SOFT) as sim:
        return FW.grid_of(sim.info("block_grid"))


@pytest.mark.parametrize("name", ["A", "B"])
def test_past_one_pass(gpu, grid, name):
    """tests/helpers/field_wrap.py's cases A (2 049 bodies, one chunk a tile, 3 passes or more, the last group filled with
    copies) and B (513 bodies, one chunk, one launch under a batch of its own): behind a call of the same count at the doubled
    points, which writes the same rows, fp64 on field_wrap's subset of rows, and every row's bits against calls so short that
    no workgroup takes a second unit."""
    case_ = FW.cases(grid)[name]
    assert case_.passes(grid) >= case_.passes_min
    s = F.system(case_.n)
    count = case_.count
    p, _, skip = FW.mixed_points(s, count, case_.chunks, 100 + count % 89)
    rows = FW.subset(case_, grid, count)
    ref, c = T.bound_of(p[:, rows], skip[rows], s, F.SOFT, block=FW.eval_block(case_.n))
    stale = T.tidal_f64(FW.doubled(p[:, rows]), skip[rows], s, F.SOFT, want_abs=False, block=FW.eval_block(case_.n))[0]
    assert np.median(T.scaled_errors(stale, ref)) > 100 * c * T.U24, "CPU: a row left from the call before misses the bound"
    with make_sim(gpu, s, **case_.options()) as sim:
        assert sim.field_option("field_chunks") == case_.chunks
        sim.tidal_at(FW.doubled(p), skip)
        big = sim.tidal_at(p, skip)
        T.check({k: big[k][rows] for k in T.KEYS}, ref, c, f"case {name}: {count} points, {case_.passes(grid)} passes, {len(rows)} rows")
        for sl in FW.one_pass_slices(count, case_.chunks, grid):
            part = sim.tidal_at(p[:, sl], skip[sl])
            for k in T.KEYS:
                bad = np.flatnonzero(T.bits(part[k]) != T.bits(big[k][sl]))
                assert len(bad) == 0, f"case {name}: {k} of {len(bad)} points from {sl.start + bad[0]} on differs from the call of points {sl.start} ... {sl.stop}"
        if name == "A":
            bodies = FW.repeated_bodies(count, case_.n)
            sim.tidal_at(FW.doubled(p), skip)
            of = sim.tidal_of(bodies)
            for lo in range(case_.n, count, case_.n):
                assert all(np.array_equal(T.bits(of[k][lo:lo + case_.n]), T.bits(of[k][:case_.n][:count - lo])) for k in T.KEYS), "a body listed again"
            bp, _, bskip = F.body_points(s, bodies[:33])
            bref, bc = T.bound_of(bp, bskip, s, F.SOFT)
            T.check({k: of[k][:33] for k in T.KEYS}, bref, bc, f"case {name}: tidal_of")


# -------------------------------------------------------------------------------------------------------------------- 8. observer
def _probe(sim, s):
    """Tidal calls of every kind, and a refused one."""
    n = len(s["m"])
    p = F.midpoints(s, 17)[0]
    sim.tidal_at(p)
    sim.tidal_at(p, np.arange(17, dtype=np.int32) % n)
    sim.tidal_of(np.arange(40) % n)
    with pytest.raises(Exception):
        sim.tidal_of([n])


def _field(sim, s):
    """A field call, in both runs at the same places: its bits do not see the tidal calls that share its buffers."""
    p, v, _ = F.midpoints(s, 21)
    got = sim.field_at(p, v, (np.arange(21, dtype=np.int32) * 5) % len(s["m"]))
    return [got[k] for k in F.KEYS]


def _record(sim, *extra):
    st = sim.state()
    return [st[k] for k in sorted(st)] + list(sim.acc()) + list(extra)


def _hermite_run(gpu, s, probe):
    """compute_acc_jerk, evolve, evolve_block with "potential", evolve_block with "nearest", a contact sweep, on one context;
    everything read."""
    look = (lambda sim: _probe(sim, s)) if probe else (lambda sim: None)
    rec = []
    with make_sim(gpu, s, integrator=2) as sim:
        look(sim)
        sim.compute_acc_jerk()
        look(sim)
        rec += list(sim.acc()) + list(sim.jerk()) + _field(sim, s)
        look(sim)
        out = sim.evolve(1e-2, max_steps=6)
        look(sim)
        rec += _record(sim, *sim.jerk(), sim.evolve_dts(), np.array([out[k] for k in sorted(out)]), np.array(sim.energy()))
        sim.set_option("potential", 1)
        look(sim)
        out = sim.evolve_block(1e-2, blocks=1, kmax=4)
        assert out["steps"] > 2 and out["body_steps"] > len(s["m"]), "the block ran in steps of several sizes"
        look(sim)
        rec += _record(sim, *sim.jerk(), sim.potential(), *sim.block_state(), np.array([float(out[k]) for k in sorted(out)]),
                       np.array([sim.potential_energy()]), *_field(sim, s))
        sim.set_option("potential", 0)
        sim.set_option("nearest", 1)
        look(sim)
        out = sim.evolve_block(1e-2, blocks=1, kmax=4)
        look(sim)
        rec += _record(sim, *sim.jerk(), *sim.nearest(), *sim.block_state(), np.array([float(out[k]) for k in sorted(out)]))
        sim.set_option("nearest", 0)
        sim.set_option("contact", 1)
        sim.upload_radii(np.full(len(s["m"]), 0.01, np.float32))
        look(sim)
        sim.compute_acc_jerk()
        look(sim)
        rec += list(sim.acc()) + list(sim.jerk()) + list(sim.contact()) + _field(sim, s)
    return rec


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"record entry {k} differs"


def test_readout_leaves_the_hermite_context_alone(gpu):
    s = F.system(1025)
    _same(_hermite_run(gpu, s, False), _hermite_run(gpu, s, True))


def test_readout_leaves_the_reference_integrator_alone(gpu):
    s = F.system(1025)

    def run(probe):
        rec = []
        with make_sim(gpu, s) as sim:      # "integrator" 0
            for _ in range(2):
                if probe:
                    _probe(sim, s)
                sim.steps(1e-4, 3)
                if probe:
                    _probe(sim, s)
                rec += _record(sim, np.array(sim.energy()), *_field(sim, s))
        return rec

    _same(run(False), run(True))


def test_open_block_refuses_and_continues(gpu):
    s = F.system(1025)
    p = F.midpoints(s, 5)[0]

    def run(probe):
        with make_sim(gpu, s, integrator=2) as sim:
            out = sim.evolve_block(5e-2, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, lambda: sim.tidal_at(p)) == E_STATE
                assert code_of(gpu, lambda: sim.tidal_of([0, 1])) == E_STATE
            out = sim.evolve_block(5e-2, blocks=1, kmax=5)
            assert out["synchronised"]
            got = sim.tidal_at(p)
            return _record(sim, *sim.jerk(), *sim.block_state(), *[got[k] for k in T.KEYS])

    _same(run(False), run(True))


# -------------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(gpu):
    n = 600
    s = F.system(n)
    lib = gpu.lib()
    p = F.midpoints(s, 20)[0]
    skip = np.full(20, -1, np.int32)
    P = [np.ascontiguousarray(x) for x in p]
    out = [np.zeros(20, np.float32) for _ in range(6)]
    fp = lambda x: x.ctypes.data_as(_fp)

    def at(count=20, pos=None, sk=skip, outs=None):
        pos = [fp(x) for x in P] if pos is None else pos
        outs = [fp(x) for x in out] if outs is None else outs
        return lib.murbtidal_at(sim._h, count, *pos, sk.ctypes.data_as(_ip) if sk is not None else None, *outs)

    def of(bodies, count=None, outs=None):
        b = np.ascontiguousarray(bodies, np.int32)
        outs = [fp(x) for x in out] if outs is None else outs
        return lib.murbtidal_of(sim._h, len(b) if count is None else count, b.ctypes.data_as(_ip), *outs)

    with make_sim(gpu, s) as fresh:
        fresh.compute_acc()
        acc_fresh = fresh.acc()

    def refused(code, rc, what):
        """The call returned its code, and nothing changed: the tensor at the same points and at bodies, the field, the forces."""
        assert rc == code, (what, rc)
        assert T.same_bits(sim.tidal_at(p, skip), before), what
        assert T.same_bits(sim.tidal_of(np.arange(16)), bodies_before), what
        assert F.same_bits(sim.field_of(np.arange(16)), field_before), what
        sim.compute_acc()
        assert all(np.array_equal(T.bits(x), T.bits(y)) for x, y in zip(sim.acc(), acc_fresh)), what

    with gpu.Simulation(n, soft=F.SOFT) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE, "before the first upload"
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        assert lib.murbtidal_at(None, 20, *[fp(x) for x in P], None, *[fp(x) for x in out]) == E_INVALID, "no context"
        assert lib.murbtidal_of(None, 0, None, *([None] * 6)) == E_INVALID
        sim.upload(s)
        before = sim.tidal_at(p, skip)
        bodies_before = sim.tidal_of(np.arange(16))
        field_before = sim.field_of(np.arange(16))
        assert at(count=0, pos=[None] * 3) == 0 and of([0], count=0) == 0
        refused(E_INVALID, at(pos=[None, fp(P[1]), fp(P[2])]), "one position array missing")
        refused(E_INVALID, at(pos=[None] * 3), "no position arrays")
        refused(E_INVALID, lib.murbtidal_of(sim._h, 3, None, *[fp(x) for x in out]), "no body list")
        for k in range(6):      # one pointer of the output group missing, and one alone set
            outs = [fp(x) for x in out]
            outs[k] = None
            refused(E_INVALID, at(outs=outs), f"tidal_at, output {k} missing")
            refused(E_INVALID, of([0, 1], outs=outs), f"tidal_of, output {k} missing")
        only = [None] * 6
        only[3] = fp(out[3])
        refused(E_INVALID, at(outs=only), "tidal_at, one output alone")
        refused(E_INVALID, of([0, 1], outs=only), "tidal_of, one output alone")
        assert at(outs=[None] * 6) == 0 and of([0, 1], outs=[None] * 6) == 0 and at(sk=None) == 0
        for bad in (np.nan, np.inf, -np.inf):
            for arr in (P[0], P[1], P[2]):
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate of {bad}")
        for bad in (-2, n, 2 ** 31 - 1):
            sk = skip.copy()
            sk[19] = bad
            refused(E_INVALID, at(sk=sk), f"skip entry {bad}")
        sk = skip.copy()
        sk[0], sk[19] = n - 1, 0
        assert at(sk=sk) == 0
        for bad in (-1, n, -2 ** 31):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
        assert of([n - 1, 0]) == 0


def test_two_shards_are_refused(gpu):
    n = 2049
    s, _ = case(n)
    p = F.midpoints(s, 5)[0]
    with gpu.Simulation(n, soft=F.SOFT, devices=[0, 0]) as sim:
        sim.upload(s)
        sim.compute_acc()
        before = sim.acc()
        assert code_of(gpu, lambda: sim.tidal_at(p)) == E_STATE
        assert code_of(gpu, lambda: sim.tidal_of([0, 1])) == E_STATE
        sim.compute_acc()
        assert all(np.array_equal(T.bits(x), T.bits(y)) for x, y in zip(before, sim.acc()))


def test_span_kind(gpu):
    """"profile" 2 records a call's sweep launches as spans of the kind "tidal" (40 points under "field_batch" 16: three
    launches), "profile" 1 does not; the field's spans and the force_* figures count what they count without the tidal calls."""
    s = F.system(600)
    p = F.midpoints(s, 40)[0]

    def run(level, tidal):
        with make_sim(gpu, s, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if tidal:
                sim.tidal_at(p)
                sim.tidal_of([1, 2, 3])
            sim.field_of([0, 1])
            return {k: sim.info(k) for k in ("span_tidal_count", "span_tidal_ms_avg", "span_field_count", "force_launches")}

    with_it, without = run(2, True), run(2, False)
    assert with_it["span_tidal_count"] == 4 and with_it["span_tidal_ms_avg"] > 0 and without["span_tidal_count"] == 0 == without["span_tidal_ms_avg"]
    assert with_it["span_field_count"] == without["span_field_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)["span_tidal_count"] == 0


# --------------------------------------------------------------------------------------------------------------------- 10. layers
def test_plugin_tidal_at(gpu):
    """HostSim.tidal_at (SimulationNBodyHIP::tidalAt through host/capi.cpp) returns Simulation.tidal_at's bits for the same bodies
    and points; tidal_matrix gives matrices whose eigenvalues sum to the trace."""
    n, soft = 1500, np.float32(2e8)
    with gpu.HostSim(n, scheme="galaxy", soft=soft) as host:
        s = host.state()
        p = F.midpoints(s, 40)[0]
        skip = (np.arange(40, dtype=np.int32) * 37) % n
        skip[::5] = -1
        got = host.tidal_at(p, skip)
        nobody = host.tidal_at(p)
        with pytest.raises(gpu.MurbHipError) as e:
            host.tidal_at(p, np.full(40, n, np.int32))
        assert e.value.code == E_INVALID
    ref, c = T.bound_of(p, skip, s, soft)
    T.check(got, ref, c, "plugin")
    with make_sim(gpu, s, soft) as sim:
        assert T.same_bits(sim.tidal_at(p, skip), got) and T.same_bits(sim.tidal_at(p), nobody)
    m = gpu.tidal_matrix(got)
    ev = np.linalg.eigvalsh(m.astype(np.float64))
    assert m.shape == (40, 3, 3) and np.allclose(ev.sum(1), T.stack(got)[:3].astype(np.float64).sum(0), rtol=1e-9, atol=1e-12 * np.abs(ev).max())

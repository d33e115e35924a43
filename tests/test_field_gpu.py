"""GPU: the field read-out murbfield_at / murbfield_of through the C ABI, the Python interface and the plugin.

Yardstick and bound: tests/helpers/field_ref.py (numpy fp64 written from include/murbfield.h, pinned by tests/test_field_host.py).
A point's error is scaled by the sum of the magnitudes of its terms and bounded by C * 2^-24, C = 4 x what the float32 emulation
attains against fp64 on the case's points, for a, j and phi alike; it is computed once per case on the CPU, and every check
prints the GPU's figure beside it (pytest -s).  Everything about reproducibility and about the read-out leaving the context
alone is differential, bit for bit."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import field_ref as F         # noqa: E402
import hermite_ref as H       # noqa: E402
import potential_ref as PR    # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
COUNTS = (1, 15, 16, 17, 33)
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


@lru_cache(maxsize=None)
def case(n):
    """(state, {name: (points, velocities, skip, fp64 reference, C)}) of the dense n-body system, 33 points a set: CPU only."""
    s = F.system(n)
    sets = {}
    for name, (p, v, skip) in (("bodies", F.body_points(s, np.arange(33) % n)), ("midpoints", F.midpoints(s, 33)),
                               ("far", F.far_points(33))):
        ref, c = F.bound_of(p, v, skip, s, F.SOFT)
        sets[name] = (p, v, skip, ref, c)
    return s, sets


# ------------------------------------------------------------------------------------------------- 1. sizes, counts, chunk cuts
@pytest.mark.parametrize("n", [1, 2, 63, 513, 1025, 2049])
def test_sizes_counts_chunks(gpu, n):
    """One to five layout tiles with and without padding, counts around the group of 16, one chunk, two, one per tile; the
    bodies themselves (field_of, and field_at with the bodies' own values and skip entries: the same bits), midpoints of body
    pairs with nobody skipped, points far outside at rest."""
    s, sets = case(n)
    tiles = -(-n // 512)
    with make_sim(gpu, s) as sim:
        for chunks in sorted({1, min(2, tiles), tiles}):
            sim.set_field_option("field_chunks", chunks)
            assert sim.field_option("field_chunks") == chunks
            for name, (p, v, skip, ref, c) in sets.items():
                whole = sim.field_at(p, v, skip)
                for count in COUNTS:
                    got = sim.field_at(first(p, count), first(v, count), first(skip, count))
                    F.check(got, ref, c, f"n={n} chunks={chunks} {name} count={count}", rows=np.arange(count))
                    assert all(np.array_equal(F.bits(got[k]), F.bits(whole[k][:count])) for k in F.KEYS), "the count changed a point's bits"
                    if name == "bodies":
                        assert F.same_bits(sim.field_of(skip[:count]), got), "field_of is field_at at the bodies' own values"
                if n == 1 and name == "bodies":
                    for k in F.KEYS:
                        assert (whole[k] == 0).all() and not np.signbit(whole[k]).any(), k
            only = sim.field_at(sets["far"][0], None, None)
            lib = gpu.lib()
            phi = np.zeros(33, np.float32)
            pts = [np.ascontiguousarray(x) for x in sets["far"][0]]
            rc = lib.murbfield_at(sim._h, 33, *[x.ctypes.data_as(_fp) for x in pts], None, None, None, None, *([None] * 6),
                                      phi.ctypes.data_as(_fp))
            assert rc == 0 and np.array_equal(F.bits(phi), F.bits(only["phi"])), "phi alone: the other output groups are optional"


# -------------------------------------------------------------------------------------------------------------- 2. sparse sources
def test_sparse_sources(gpu):
    """Mass at every tile's first and last slot and a few between (potential_ref.SPARSE_SOURCES), then one run per source with
    that source alone massive: a dropped or doubled j slot is a whole term, at 10 x the bound or more
    (tests/test_field_host.py::test_sparse_probe_has_power asserts that on the same inputs)."""
    s, soft, src = F.sparse_sources()
    n = len(s["m"])
    p, v, skip = F.midpoints(s, 64, stride=11)
    bodies = np.concatenate([src, [1, 510, 513, 1022, 2046]]).astype(np.int32)
    bp, bv, bskip = F.body_points(s, bodies)
    ref, c = F.bound_of(p, v, skip, s, soft)
    bref, bc = F.bound_of(bp, bv, bskip, s, soft)
    with make_sim(gpu, s, soft) as sim:
        for chunks in (1, 2, 5):
            sim.set_field_option("field_chunks", chunks)
            F.check(sim.field_at(p, v), ref, c, f"sparse, all sources, chunks={chunks}: midpoints")
            F.check(sim.field_of(bodies), bref, bc, f"sparse, all sources, chunks={chunks}: bodies")
    sim = gpu.Simulation(n, soft=soft)
    with sim:
        for k in src:
            one = F.only_source(s, k)
            sim.upload(one)
            ref1, c1 = F.bound_of(p, v, skip, one, soft)
            got = sim.field_at(p, v)
            F.check(got, ref1, c1, f"sparse, source {k} alone: midpoints")
            assert (got["phi"] > 0).all()
            bref1, bc1 = F.bound_of(bp, bv, bskip, one, soft)
            gotb = sim.field_of(bodies)
            F.check(gotb, bref1, bc1, f"sparse, source {k} alone: bodies")
            me = int(np.flatnonzero(bodies == k)[0])
            assert all(gotb[q][me] == 0 and not np.signbit(gotb[q][me]) for q in F.KEYS), "the lone source sees nothing of itself"


# ----------------------------------------------------------------------------------------------------------------------- 3. skip
@pytest.mark.parametrize("n", [2, 514])
def test_skip_own_term(gpu, n):
    """potential_ref.own_term_pair: the own term is 1e4 x the pair term.  With skip = own, phi meets the bound; without, it is
    phi + G m / soft to fp32."""
    s, soft, (a, b) = PR.own_term_pair(n)
    p, v, skip = F.body_points(s, [a, b])
    ref, c = F.bound_of(p, v, skip, s, soft)
    with make_sim(gpu, s, soft) as sim:
        got = sim.field_at(p, v, skip)
        F.check(got, ref, c, f"own term n={n}: skipped")
        assert F.same_bits(sim.field_of([a, b]), got)
        bare = sim.field_at(p, v)
    own = float(H.G) * PR.OWN_MASS / float(soft)
    want = ref[2] + own
    err = np.abs(bare["phi"] - want) / want
    # fp32: v_rsq_f32 within 1 ulp (2 x 2^-24), soft^2 rounded (half of 2^-24 behind the root), G m * inv and the addition rounded
    # (2^-24 each): 4.5, taken as 6
    print(f"own term n={n}: without skip phi off by {err.max() * 2.0 ** 24:.2f} x 2^-24 of phi + G m / soft (bound 6)")
    assert err.max() <= 6 * 2.0 ** -24
    assert np.array_equal(F.bits(bare["ax"]), F.bits(got["ax"])), "the own term adds nothing to a: d = 0"


def test_skip_masks_a_and_j_too(gpu):
    """A point 10 x soft beside a body that outweighs all others together, that body skipped: a, j and phi are the fp64 field of
    the others.  A mask on phi alone leaves the body's pull in a and j, orders of magnitude above the rest."""
    s = F.system(1025)
    s["m"][700] = np.float32(1e16)
    p, v = F.displaced(s, 700, F.SOFT)
    skip = np.array([700], np.int32)
    ref, c = F.bound_of(p, v, skip, s, F.SOFT)
    with_it = F.field_f64(p, v, None, s, F.SOFT)
    assert np.linalg.norm(with_it[0][:, 0]) > 1e3 * ref[3]["a"][0] and with_it[2][0] > 1e2 * ref[2][0]      # CPU: the probe has power
    with make_sim(gpu, s) as sim:
        for chunks in (1, 3):
            sim.set_field_option("field_chunks", chunks)
            F.check(sim.field_at(p, v, skip), ref, c, f"displaced point, chunks={chunks}")


def test_skipped_slot_positions(gpu):
    """The skipped slot at a tile's first and last slot, the last real slot, and in every chunk."""
    n = 2049
    s, sets = case(n)
    slots = np.array([0, 511, 512, 1023, 1024, 1535, 2047, n - 1], np.int32)
    p, v, skip = F.body_points(s, slots)
    p = (p + np.float32(0.003)).astype(np.float32)      # beside the body, not on it
    ref, c = F.bound_of(p, v, skip, s, F.SOFT)
    with make_sim(gpu, s) as sim:
        for chunks in (1, 2, 5):
            sim.set_field_option("field_chunks", chunks)
            F.check(sim.field_at(p, v, skip), ref, c, f"skipped slots, chunks={chunks}")
            F.check(sim.field_at(p[:, ::-1], v[:, ::-1], skip[::-1]), ref, c, f"skipped slots reversed, chunks={chunks}", rows=np.arange(len(slots))[::-1])


@pytest.mark.parametrize("pair", PR.COINCIDENT_PAIRS)
def test_coincident_bodies_count(gpu, pair):
    """Two bodies at one place, one skipped: the other counts with G m / soft.  The exclusion is by slot, not by d == 0."""
    s, soft = PR.coincident(pair)
    a, b = pair
    p, v, skip = F.body_points(s, [a, b, a, a])      # the same body listed three times
    ref, c = F.bound_of(p, v, skip, s, soft)
    gm = H._gm(s)
    assert ref[2][0] > gm[b] / float(soft) > 1e3 * c["phi"] * F.U24 * ref[2][0]
    with make_sim(gpu, s, soft) as sim:
        got = sim.field_of([a, b, a, a])
        F.check(got, ref, c, f"coincident {pair}")
        assert all(F.bits(got[k])[0] == F.bits(got[k])[2] == F.bits(got[k])[3] for k in F.KEYS), "the same body twice: the same bits"


# ------------------------------------------------------------------------------------------------------------------- 4. company
def test_company(gpu):
    """64 points over the dense 2 049-body system, the first wave's four skipping bodies in four different tiles: every point's
    seven results have the same bits alone, in the call of 64, in the reversed call, under "field_batch" 16, 32 and the default,
    and in a second run — for the default chunk cut (one chunk at this size), for two chunks and for one per tile."""
    s, _ = case(2049)
    rng = np.random.default_rng(7)
    p = rng.uniform(0.0, 1.0, (3, 64)).astype(np.float32)
    v = (1e-3 * rng.standard_normal((3, 64))).astype(np.float32)
    skip = np.full(64, -1, np.int32)
    skip[:4] = (5, 600, 1100, 1700)
    skip[4:40:3] = rng.integers(0, 2049, 12)
    skip[63] = 2048
    assert len({int(x) // F.TILE for x in skip[:4]}) == 4
    ref, c = F.bound_of(p, v, skip, s, F.SOFT)
    for chunks in (0, 2, 5):
        with make_sim(gpu, s, field_chunks=chunks) as sim:
            whole = sim.field_at(p, v, skip)
            F.check(whole, ref, c, f"company, chunks option {chunks}")
            alone = [sim.field_at(p[:, k:k + 1], v[:, k:k + 1], skip[k:k + 1]) for k in range(64)]
            for k in F.KEYS:
                assert np.array_equal(F.bits(np.concatenate([x[k] for x in alone])), F.bits(whole[k])), f"{k}: alone against the call of 64"
            rev = sim.field_at(p[:, ::-1], v[:, ::-1], skip[::-1])
            assert all(np.array_equal(F.bits(rev[k][::-1]), F.bits(whole[k])) for k in F.KEYS), "the call reversed"
            for batch in (16, 32, 0):
                sim.set_field_option("field_batch", batch)
                assert F.same_bits(sim.field_at(p, v, skip), whole), f"field_batch {batch}"
        with make_sim(gpu, s, field_chunks=chunks) as again:
            assert F.same_bits(again.field_at(p, v, skip), whole), "a second run"


# ----------------------------------------------------------------------------------------------------- 5. agreement with the sweeps
@pytest.mark.parametrize("n", [1, 513, 2049])
def test_agrees_with_the_sweeps(gpu, n):
    """field_of(every body) and murbhip_compute_acc_jerk with "potential" 1 each meet the bound against fp64; a lone body gets
    +0.0f from both."""
    s, _ = case(n)
    p, v, skip = F.body_points(s, np.arange(n))
    ref, c = F.bound_of(p, v, skip, s, F.SOFT)
    with make_sim(gpu, s, integrator=2, potential=1) as sim:
        field = sim.field_of(np.arange(n))
        sim.compute_acc_jerk()
        sweep = dict(zip(F.KEYS, list(sim.acc()) + list(sim.jerk()) + [sim.potential()]))
        again = sim.field_of(np.arange(n))
    F.check(field, ref, c, f"n={n}: field_of")
    F.check(sweep, ref, c, f"n={n}: the sweep")
    assert F.same_bits(field, again)
    if n == 1:
        for got in (field, sweep):
            assert all(got[k][0] == 0 and not np.signbit(got[k][0]) for k in F.KEYS)


# -------------------------------------------------------------------------------------------------------------------- 6. read-out
def _probe(sim, s):
    """Field calls of every kind, and refused ones."""
    n = len(s["m"])
    p, v, skip = F.midpoints(s, 17)
    sim.field_at(p, v, skip)
    sim.field_at(p, None, np.arange(17, dtype=np.int32) % n)
    sim.field_of(np.arange(40) % n)
    with pytest.raises(Exception):
        sim.field_of([n])


def _record(sim, *extra):
    st = sim.state()
    return [st[k] for k in sorted(st)] + list(sim.acc()) + list(extra)


def _hermite_run(gpu, s, probe):
    """compute_acc_jerk, evolve, evolve_block with "potential", evolve_block with "nearest" on one context; everything read."""
    look = (lambda sim: _probe(sim, s)) if probe else (lambda sim: None)
    rec = []
    with make_sim(gpu, s, integrator=2) as sim:
        look(sim)
        sim.compute_acc_jerk()
        look(sim)
        rec += list(sim.acc()) + list(sim.jerk())
        look(sim)
        out = sim.evolve(1e-2, max_steps=6)
        look(sim)
        rec += _record(sim, *sim.jerk(), sim.evolve_dts(), np.array([out[k] for k in sorted(out)]))
        sim.set_option("potential", 1)
        look(sim)
        out = sim.evolve_block(1e-2, blocks=1, kmax=4)
        assert out["steps"] > 2 and out["body_steps"] > len(s["m"]), "the block ran in steps of several sizes"
        look(sim)
        rec += _record(sim, *sim.jerk(), sim.potential(), *sim.block_state(), np.array([float(out[k]) for k in sorted(out)]))
        sim.set_option("potential", 0)
        sim.set_option("nearest", 1)
        look(sim)
        out = sim.evolve_block(1e-2, blocks=1, kmax=4)
        look(sim)
        rec += _record(sim, *sim.jerk(), *sim.nearest(), *sim.block_state(), np.array([float(out[k]) for k in sorted(out)]))
        sim.compute_acc_jerk()
        look(sim)
        rec += list(sim.acc()) + list(sim.jerk()) + list(sim.nearest())
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
                rec += _record(sim)
        return rec

    _same(run(False), run(True))


def test_open_block_refuses_and_continues(gpu):
    s = F.system(1025)
    p, v, skip = F.midpoints(s, 5)

    def run(probe):
        with make_sim(gpu, s, integrator=2) as sim:
            out = sim.evolve_block(5e-2, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, lambda: sim.field_at(p, v, skip)) == E_STATE
                assert code_of(gpu, lambda: sim.field_of([0, 1])) == E_STATE
            out = sim.evolve_block(5e-2, blocks=1, kmax=5)
            assert out["synchronised"]
            field = sim.field_at(p, v, skip)
            return _record(sim, *sim.jerk(), *sim.block_state(), *[field[k] for k in F.KEYS])

    _same(run(False), run(True))


# -------------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(gpu):
    n = 600
    s = F.system(n)
    lib = gpu.lib()
    p, v, skip = F.midpoints(s, 20)
    skip = np.full(20, -1, np.int32)
    P, Vv = [np.ascontiguousarray(x) for x in p], [np.ascontiguousarray(x) for x in v]
    out = [np.zeros(20, np.float32) for _ in range(7)]
    fp = lambda x: x.ctypes.data_as(_fp)

    def at(count=20, pos=None, vel=None, sk=skip, outs=None):
        pos = [fp(x) for x in P] if pos is None else pos
        vel = [fp(x) for x in Vv] if vel is None else vel
        outs = [fp(x) for x in out] if outs is None else outs
        return lib.murbfield_at(sim._h, count, *pos, *vel, sk.ctypes.data_as(_ip) if sk is not None else None, *outs)

    def of(bodies, count=None, outs=None):
        b = np.ascontiguousarray(bodies, np.int32)
        outs = [fp(x) for x in out] if outs is None else outs
        return lib.murbfield_of(sim._h, len(b) if count is None else count, b.ctypes.data_as(_ip), *outs)

    with make_sim(gpu, s) as fresh:
        fresh.compute_acc()
        acc_fresh = fresh.acc()

    def refused(code, rc, what):
        """The call returned its code, and nothing changed: the field of the same points, the field of bodies, the forces."""
        assert rc == code, (what, rc)
        assert F.same_bits(sim.field_at(p, v, skip), before), what
        assert F.same_bits(sim.field_of(np.arange(16)), bodies_before), what
        sim.compute_acc()
        assert all(np.array_equal(F.bits(x), F.bits(y)) for x, y in zip(sim.acc(), acc_fresh)), what

    with gpu.Simulation(n, soft=F.SOFT) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE, "before the first upload"
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        sim.upload(s)
        before = sim.field_at(p, v, skip)
        bodies_before = sim.field_of(np.arange(16))
        assert at(count=0, pos=[None] * 3) == 0 and of([0], count=0) == 0
        refused(E_INVALID, at(pos=[None, fp(P[1]), fp(P[2])]), "one position array missing")
        refused(E_INVALID, at(pos=[None] * 3), "no position arrays")
        refused(E_INVALID, lib.murbfield_of(sim._h, 3, None, *[fp(x) for x in out]), "no body list")
        refused(E_INVALID, at(vel=[fp(Vv[0]), None, None]), "one velocity array")
        refused(E_INVALID, at(vel=[None, fp(Vv[1]), fp(Vv[2])]), "two velocity arrays")
        assert at(vel=[None] * 3) == 0
        for k in (0, 1, 2, 3, 5):      # one pointer of an output group missing
            outs = [fp(x) for x in out]
            outs[k] = None
            refused(E_INVALID, at(outs=outs), f"field_at, output {k} missing")
            refused(E_INVALID, of([0, 1], outs=outs), f"field_of, output {k} missing")
        assert at(outs=[None] * 6 + [fp(out[6])]) == 0 and at(outs=[fp(x) for x in out[:6]] + [None]) == 0
        for bad in (np.nan, np.inf, -np.inf):
            for arr in (P[1], Vv[2]):
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate or velocity of {bad}")
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
        refused(E_INVALID, lib.murbfield_set_option(sim._h, b"jsplit", 1), "a key of another interface")
        for key, bad in (("field_chunks", -1), ("field_batch", 8), ("field_batch", -16), ("field_batch", (1 << 20) + 16)):
            refused(E_INVALID, lib.murbfield_set_option(sim._h, key.encode(), bad), f"{key} = {bad}")
        assert sim.field_option("field_batch") == 16384 and sim.field_option("field_chunks") == 1


def test_two_shards_are_refused(gpu):
    n = 2049
    s, _ = case(n)
    p, v, skip = F.midpoints(s, 5)
    with gpu.Simulation(n, soft=F.SOFT, devices=[0, 0]) as sim:
        sim.upload(s)
        sim.compute_acc()
        before = sim.acc()
        assert code_of(gpu, lambda: sim.field_at(p, v, skip)) == E_STATE
        assert code_of(gpu, lambda: sim.field_of([0, 1])) == E_STATE
        sim.compute_acc()
        assert all(np.array_equal(F.bits(x), F.bits(y)) for x, y in zip(before, sim.acc()))


# ---------------------------------------------------------------------------------------------------------------------- 8. layers
def test_plugin_field_at(gpu):
    """HostSim.field_at (SimulationNBodyHIP::fieldAt through host/capi.cpp) returns Simulation.field_at's bits for the same bodies
    and points."""
    n, soft = 1500, np.float32(2e8)
    with gpu.HostSim(n, scheme="galaxy", soft=soft) as host:
        s = host.state()
        p, v, _ = F.midpoints(s, 40)
        skip = (np.arange(40, dtype=np.int32) * 37) % n
        skip[::5] = -1
        got = host.field_at(p, v, skip)
        at_rest = host.field_at(p)
        with pytest.raises(gpu.MurbHipError) as e:
            host.field_at(p, v, np.full(40, n, np.int32))
        assert e.value.code == E_INVALID
    ref, c = F.bound_of(p, v, skip, s, soft)
    F.check(got, ref, c, "plugin")
    with make_sim(gpu, s, soft) as sim:
        assert F.same_bits(sim.field_at(p, v, skip), got) and F.same_bits(sim.field_at(p), at_rest)


# ------------------------------------------------------------------------------------------------- 9. after the state has moved
MOVE_N = 1025
MOVE_DT = 2.0 ** -10      # one step of it moves a body by about 1e-3 of the box and its velocity by about 2 (CPU estimate: |a| is
#                           about 2e3): the field of the state before that step misses the bound by 100 x or more nearly everywhere
MOVES = [(0, "steps", 1), (0, "steps", 2), (1, "steps", 1), (1, "steps", 2), (2, "steps", 1), (2, "steps", 2), (2, "evolve", 3),
         (2, "evolve_block", 0)]


def _advance(sim, how, k, whole=None):
    """Take the context through the run (k steps of its integrator, evolve() in k steps, or one block of evolve_block()) and
    return its number of steps; with `whole`, that number, stop one step before the run's end."""
    if how == "steps":
        if whole is None or k > 1:
            sim.steps(MOVE_DT, k if whole is None else k - 1)
        return k
    if how == "evolve":      # dt_min = dt_max: k steps of MOVE_DT
        steps = k if whole is None else k - 1
        out = sim.evolve(k * MOVE_DT, dt_min=MOVE_DT, dt_max=MOVE_DT, max_steps=steps)
        assert out["steps"] == steps and out["dt_min"] == out["dt_max"] == MOVE_DT, out
        return k
    sim.compute_acc_jerk()
    sim.set_block_levels(np.arange(sim.n) % 3, 2)      # by hand: the starting rule puts every body of this system at level 0, one step a block
    out = sim.evolve_block(4 * MOVE_DT, blocks=1, kmax=2, **({} if whole is None else {"max_steps": whole - 1}))
    assert out["synchronised"] == (whole is None) and out["steps"] == (whole - 1 if whole else out["steps"]) and out["steps"] >= 1, out
    return out["steps"]


def _check_some(got, ref, c, what, quantities):
    if len(quantities) == 3:
        return F.check(got, ref, c, what)
    e = F.scaled_errors(got, ref)
    fig = {k: float(np.max(e[k], initial=0.0)) / F.U24 for k in quantities}
    print(f"{what}: scaled error in 2^-24: " + ", ".join(f"{k} {fig[k]:.2f} (bound {c[k]:.2f})" for k in quantities))
    for k in quantities:
        assert fig[k] <= c[k], f"{what}: {k} of point {int(np.argmax(e[k]))} off by {fig[k]:.2f} x 2^-24, bound {c[k]:.2f}"


@pytest.mark.parametrize("integrator,how,k", MOVES)
def test_field_of_the_moved_state(gpu, integrator, how, k):
    """After steps of every integrator (k = 1 and 2: both record buffers have been the current one), after an evolve() to its end
    and after an evolve_block() to its synchronised end: field_of(every body) and field_at(midpoints) meet the bound against fp64
    evaluated at the state the context returns.  The probe has power (CPU): the fp64 field of the bodies as they were one step
    earlier, and as they were uploaded, at the same points misses 100 x the bound on at least half the points, in every compared
    quantity — a read-out that swept the other record buffer, or velocities a step old, fails.
    "integrator" 1: the device's velocities are half a step behind the ones murbhip_download_state returns (include/murbfield.h),
    so there a and phi alone are compared; they read positions only."""
    s = F.system(MOVE_N)
    n = MOVE_N
    quantities = ("a", "phi") if integrator == 1 else ("a", "j", "phi")

    def moved(sim):
        return dict(sim.state(), m=s["m"])

    with make_sim(gpu, s, integrator=integrator) as sim:
        steps = _advance(sim, how, k)
        assert steps >= 2 or how == "steps", "the run has a step before its last"
        now = moved(sim)
        of = sim.field_of(np.arange(n))
        mp, mv, _ = F.midpoints(now, 64)
        at = sim.field_at(mp, mv)
        assert F.same_bits(of, sim.field_of(np.arange(n))) and all(np.array_equal(now[q], moved(sim)[q]) for q in now), "the read-out moved something"
    with make_sim(gpu, s, integrator=integrator) as sim:
        _advance(sim, how, k, whole=steps)
        earlier = moved(sim)
    bp, bv, bskip = F.body_points(now, np.arange(n))
    what = f"integrator {integrator}, {how}" + (f" {k}" if k else "")
    for name, got, (p, v, skip) in (("field_of", of, (bp, bv, bskip)), ("midpoints", at, (mp, mv, None))):
        ref, c = F.bound_of(p, v, skip, now, F.SOFT)
        for old_name, old in (("a step earlier", earlier), ("as uploaded", s)):
            e = F.scaled_errors(F.field_f64(p, v, skip, old, F.SOFT, want_abs=False)[:3], ref)
            share = {q: float((e[q] >= 100.0 * c[q] * F.U24).mean()) for q in quantities}
            print(f"{what}, {name}: the bodies {old_name} miss 100 x the bound on " + ", ".join(f"{100 * share[q]:.0f} % ({q})" for q in quantities))
            assert min(share.values()) >= 0.5, (what, name, old_name, share)
        _check_some(got, ref, c, f"{what}: {name}", quantities)


# --------------------------------------------------------------------------------------------------- 10. the sweeps' side options
def test_side_options_change_nothing(gpu):
    """The field bits of one set of points and of every body are the same with all side options off, with "nearest" 1, with
    "contact" 1 and large radii uploaded (they ride in the velocity records' spare lanes, which the field never reads) and with
    "potential" 1: on the uploaded state, and again behind a compute_acc_jerk() and one Hermite step."""
    n = 2049
    s, _ = case(n)
    rng = np.random.default_rng(19)
    p = rng.uniform(0.0, 1.0, (3, 64)).astype(np.float32)
    v = (1e-3 * rng.standard_normal((3, 64))).astype(np.float32)
    skip = rng.integers(-1, n, 64).astype(np.int32)
    skip[:4] = (-1, 0, 511, n - 1)
    want = None
    for option in (None, "nearest", "contact", "potential"):
        with make_sim(gpu, s, integrator=2, **({option: 1} if option else {})) as sim:
            if option == "contact":
                sim.upload_radii(np.full(n, 8.0, np.float32))
            rec = [sim.field_at(p, v, skip), sim.field_of(np.arange(n))]
            sim.compute_acc_jerk()
            sim.step(MOVE_DT)
            rec += [sim.field_at(p, v, skip), sim.field_of(np.arange(n))]
            st = sim.state()
        assert not F.same_bits(rec[0], rec[2]) and not F.same_bits(rec[1], rec[3]), "the step moved the bodies"
        if want is None:
            want, want_state = rec, st
            continue
        assert all(np.array_equal(F.bits(st[k]), F.bits(want_state[k])) for k in st), f'"{option}" 1 changed the step'
        for k, (x, y) in enumerate(zip(rec, want)):
            assert F.same_bits(x, y), f'"{option}" 1: field call {k} differs from the call with all side options off'

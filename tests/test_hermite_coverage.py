"""GPU: what the dense Hermite tests cannot see.  All tests here need an MI355X.

1. Pair coverage of the acceleration + jerk sweep, body by body, with the sparse-mass probes of tests/test_pair_coverage.py
   (oracle.probe_sources, oracle.probe_state with the base problem's velocities): at most 256 bodies carry mass, so the fp64
   truth (hermite_ref.acc_jerk_sources) costs O(n K), EVERY body is checked, and one source's term is a visible share of every
   body's jerk.  A j body that is skipped, counted twice, paired with the wrong velocity or lost at a chunk or stage boundary
   is >= 10 x the bound on 99 % of the bodies, which every probe asserts of itself (tests/test_hermite_coverage_host.py shows
   it on the checker).  The probes of one size run back to back in ONE context, each with its sources in other slots than the
   one before, over every chunk count "jsplit" can ask for — up, down and up again, so that the partial rows are re-allocated
   and a shorter sum runs over a longer buffer.
2. The minimum behind every adaptive step: one fast body decides the step; it is moved through the lanes, halves, waves and
   workgroups of the fold, and every recorded step must be the restatement's, bit for bit.
3. murbhip_evolve's batch length ("evolve_batch") and the wrap-around of its ring of 4096 recorded steps.

Bounds (tests/helpers/hermite_probe.py): accelerations oracle.probe_err <= 2e-6; jerks hermite_ref.scaled_err <= C 2^-24 with
C = 4 x what the same numpy formula attains in float32 against fp64 on the same probe.  The bounds were derived on the CPU
only, never from a device's output: float32 numpy attains 1.9-13.9 x 2^-24 on these probes (n = 2 ... 30 000, K = 1 ... 239;
the largest with two sources), so C is 8-55; the 1 % quantile of the smallest-term share is at least 4.5 x the condition.

Measured on an MI355X (worst body of the probes of a test, jerk in units of 2^-24, beside the smallest C of those probes;
accelerations as a share of the source terms, bound 2e-6; forced chunk counts: the first of the two probes of each count):
    probes                                              galaxy: jerk (smallest C)  acc     random: jerk (smallest C)  acc
    n = 2 ... 2 049, default chunking (33 probes each)     3.91 (1.06; n = 2, K = 1)  2.1e-7     7.06 (7.66)            2.7e-7
    n = 3 035,  "jsplit" 1 5 2 6 3 9 4                     3.28 (8.51)                1.6e-7     4.77 (15.59)           1.8e-7
    n = 12 001, "jsplit" 1 7 0 24 5 32                     3.89 (8.03)                2.3e-7     2.97 (9.76)            1.7e-7
    n = 30 000, "jsplit" 0 32 13                           4.60 (9.87)                2.6e-7     2.36 (7.55)            2.1e-7
    step route, n = 987 / 3 035 / 12 001, at the prediction   3.37 / 3.16 / 2.71 (12.3 / 10.3 / 8.7)     6.50 / 4.87 / 3.00 (31.5 / 19.3 / 11.0)
No probe's jerk error exceeds 0.46 of its own bound (0.25 x the bound = the float32 numpy figure itself).  The ring-wrap run
takes 6 127 steps of 628 s ... 3.58e5 s on the device (restatement: 6 121)."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_adaptive_ref as A   # noqa: E402
import hermite_probe as P          # noqa: E402

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
E_INVALID = -2000
MAX_PARTS = 32           # kMaxParts / 2: the most j chunks "jsplit" can ask for


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def everything(sim):
    """q, v and the remembered (a, j) of a context, as one dict of fp32 arrays."""
    out = dict(sim.state())
    out.update({"a" + "xyz"[k]: x for k, x in enumerate(sim.acc())})
    out.update({"j" + "xyz"[k]: x for k, x in enumerate(sim.jerk())})
    return out


def assert_same_bits(got, want, what=""):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what} {k}"


def hermite_sim(gpu, n, soft=SOFT, **opts):
    sim = gpu.Simulation(n, soft=soft)
    sim.set_option("integrator", 2)
    for k, v in opts.items():
        sim.set_option(k, v)
    return sim


# ------------------------------------------------------------------------------------------------------ probes of the sweep
@lru_cache(maxsize=None)
def _problem(n, scheme):
    """(base state, source sets): CPU only, shared by every test of that size."""
    import murbhip
    import oracle
    first, count = murbhip.partition(n, 1, 0)
    sources = oracle.probe_sources(n, [first], [count], murbhip.slice_slots(n, 1), probes=14, k_max=256, per_block=8)
    return oracle.init_bodies(n, scheme), [s for s in sources if len(s)]     # (2 bodies: a probe may find no unused slot)


@lru_cache(maxsize=None)
def _probe(n, scheme, k):
    """(state, sources, truth) of probe k of a size (cyclic)."""
    import oracle
    base, sources = _problem(n, scheme)
    k %= len(sources)
    ps = oracle.probe_state(base, sources[k], seed=k, zero_velocities=False)
    return ps, sources[k], P.Truth(ps, sources[k], SOFT)


class Run:
    """The probes of one size, taken in turn; collects the figures of the checks."""

    def __init__(self, n, scheme):
        self.n, self.scheme, self.next, self.lines, self.last = n, scheme, 0, [], ()

    def take(self):
        self.next += 1
        ps, src, truth = _probe(self.n, self.scheme, self.next - 1)
        if self.n > 17:     # (fewer bodies than that leave no unused slots to move to)
            assert not set(src.tolist()) & set(self.last), "a probe repeats a slot of the one before"
        self.last = src.tolist()
        return ps, src, truth

    def evaluate(self, sim, what):
        """Upload the next probe, compute_acc_jerk, check every body; returns (state, sources, acc, jerk)."""
        ps, src, truth = self.take()
        sim.upload(ps)
        sim.compute_acc_jerk()
        a, j = sim.acc(), sim.jerk()
        self.lines.append(P.check(a, j, truth, f"{self.scheme} n={self.n} {what}"))
        return ps, src, a, j

    def step(self, sim, what):
        """The step route: evaluate() for the device's own (a0, j0), one step, then (a1, j1) against the truth at the
        restated prediction.  Returns the probe state."""
        ps, src, a0, j0 = self.evaluate(sim, what)
        sim.step(DT)
        a1, j1 = sim.acc(), sim.jerk()
        p = P.predicted(ps, a0, j0, DT)
        self.lines.append(P.check(a1, j1, P.Truth(p, src, SOFT), f"{self.scheme} n={self.n} {what} (step, at the prediction)"))
        return ps


def parts_of(sim):
    return int(sim.info("hermite_parts"))


SMALL = (1, 2, 15, 16, 17, 511, 512, 513, 987, 1024, 1025, 2049)


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
def test_default_chunking_small_sizes(gpu, O, scheme):
    """i-group ends at every count mod 16, a ragged last tile, the first body of a second block; three probes per size in
    one context."""
    for n in SMALL:
        run = Run(n, scheme)
        with hermite_sim(gpu, n) as sim:
            tiles = int(sim.info("slots")) // P.TILE
            assert 1 <= parts_of(sim) <= min(tiles, MAX_PARTS)
            for k in range(3):
                ps, src, a, j = run.evaluate(sim, f"probe {k}")
                if n == 1:      # the self term is exactly 0 in both sums
                    assert all(float(x[0]) == 0.0 for x in a + j)


# chunk counts in the order they are set: up (re-allocation of the partial rows), down (fewer rows summed than the buffer
# holds), up again
FORCED = {3035: (1, 5, 2, 6, 3, 9, 4), 12001: (1, 7, 0, 24, 5, 32), 30000: (0, 32, 13)}


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
@pytest.mark.parametrize("n", sorted(FORCED))
def test_forced_chunk_counts(gpu, O, scheme, n):
    """n = 3035: 6 tiles, chunks of one tile, odd chunks, the half-filled last stage; 12 001: 24 tiles; 30 000: 60 tiles.
    info("hermite_parts") is the chunk count the sweep runs with, clamped to the tiles and to 32.  Two probes per chunk
    count, each in other slots than the one before."""
    run = Run(n, scheme)
    with hermite_sim(gpu, n) as sim:
        tiles = int(sim.info("slots")) // P.TILE
        assert tiles == -(-n // 1024) * 2
        for jsplit in FORCED[n]:
            sim.set_option("jsplit", jsplit)
            parts = parts_of(sim)
            if jsplit:
                assert parts == min(jsplit, tiles, MAX_PARTS), (jsplit, parts)
            else:
                assert 1 <= parts <= min(tiles, MAX_PARTS)
                if n == 30000:
                    assert parts > 1
            # two probes per chunk count: between them their sources sit in every tile, so in every chunk
            tiles_hit = set()
            for k in range(2):
                _, src, _, _ = run.evaluate(sim, f"jsplit {jsplit} ({parts} chunks) probe {k}")
                tiles_hit |= set((src // P.TILE).tolist())
            assert tiles_hit == set(range(-(-n // P.TILE))), sorted(tiles_hit)


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
@pytest.mark.parametrize("n,jsplit", [(987, 0), (3035, 3), (12001, 0)])
def test_step_route(gpu, O, scheme, n, jsplit):
    """The sweep of a step runs at the PREDICTED state: (a1, j1) after step(DT) against the truth at hermite_ref.predict of the
    uploaded state, from the device's own (a0, j0), rounded to fp32.  Twice per context, on different probes.  (A probe's
    masses are small: its prediction moves the positions by v dt, 1e-4 of the distances, and the velocities by a few ulp only.
    That the sweep reads the predicted VELOCITIES is pinned bit for bit by test_hermite_gpu.test_corrector_bit_exact.)"""
    run = Run(n, scheme)
    with hermite_sim(gpu, n, jsplit=jsplit) as sim:
        for k in range(2):
            run.step(sim, f"jsplit {jsplit} probe {k}")


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
def test_pinned_evolve_is_one_step(gpu, O, scheme):
    """Several chunks: evolve(DT, dt_min = dt_max = DT) is step(DT), bit for bit, in q, v, a, j; the adaptive launches run the
    same sweep over the same chunks."""
    n = 12001
    ps, src, truth = _probe(n, scheme, 1)
    with hermite_sim(gpu, n, jsplit=7) as ada, hermite_sim(gpu, n, jsplit=7) as fix:
        assert parts_of(ada) == parts_of(fix) == 7
        for sim in (ada, fix):
            sim.upload(ps)
        out = ada.evolve(float(DT), dt_min=float(DT), dt_max=float(DT))
        fix.step(DT)
        assert out["steps"] == 1 and out["time"] == float(DT) and bits(ada.evolve_dts()[0]) == bits(DT)
        assert_same_bits(everything(ada), everything(fix))


# ------------------------------------------------------------------------------------------- where the deciding body sits
@lru_cache(maxsize=None)
def _fast(n):
    import murbhip
    return P.fast_state(murbhip.init_bodies(n, "random"))


def decide(ada, rep, s, t):
    """Upload `s` (the fast body in slot t) to both contexts, evolve four steps on `ada`, replay them one by one on `rep` with
    (a, j) downloaded around each; assert where the minimum sat and every step's bits.  Returns ada's result and steps."""
    ada.upload(s)
    rep.upload(s)
    out = ada.evolve(P.DECIDE_DURATION, eta=P.ETA, eta_start=P.ETA_START, max_steps=P.DECIDE_STEPS)
    dts = ada.evolve_dts()
    assert out["steps"] == len(dts) == P.DECIDE_STEPS
    rep.compute_acc_jerk()
    r = P.Replay(rep.acc(), rep.jerk(), P.DECIDE_DURATION)
    for k, dt in enumerate(dts):
        want = r.want()     # k = 0: the starting rule — the upload dropped whatever proposal the context had retained
        assert bits(want) == bits(dt), f"slot {t}: step {k} is {float(dt)!r}, the restatement takes {float(want)!r}; decided by {r.deciders[-1]}"
        rep.step(dt)
        r.took(dt, rep.acc(), rep.jerk())
    assert bits(r.dt_next()) == bits(np.float32(out["dt_next"])), f"slot {t}: dt_next"
    for k in (0, 2, 3):     # the first step, and the sizes chosen after steps 2 and 3
        who, margin = r.deciders[k]
        assert who == t and margin >= P.MARGIN, f"slot {t}: choice {k} is decided by body {who}, runner-up x {margin:.3f}"
    return out, dts


@pytest.mark.parametrize("group", sorted(P.TARGET_GROUPS))
def test_deciding_body_in_every_place_of_the_fold(gpu, group):
    """n = 1500: four workgroups of 512 slots, the third partly padding, the fourth all padding.  The fast body in every lane
    and half of wave 0, in the row ends of waves 1-3 and of workgroups 1 and 2, on both sides of the workgroup boundaries,
    and in the last real slot."""
    n = 1500
    targets = list(P.TARGET_GROUPS[group]) + ([n - 1] if group == "edges" else [])
    s = _fast(n)
    with hermite_sim(gpu, n) as ada, hermite_sim(gpu, n) as rep:
        seen = {}
        for t in targets:
            seen[t] = decide(ada, rep, P.swapped(s, t), t)
        print(f"{group}: {len(targets)} slots; first steps {min(float(d[0]) for _, d in seen.values()):.6g} ... "
              f"{max(float(d[0]) for _, d in seen.values()):.6g} s")
        if group == "wave0":
            # after all those uploads the reused contexts give, for the unswapped state, what fresh ones give
            with hermite_sim(gpu, n) as fresh_ada, hermite_sim(gpu, n) as fresh_rep:
                out, dts = decide(fresh_ada, fresh_rep, s, 0)
                again, dts_again = decide(ada, rep, P.swapped(s, 0), 0)
                assert out == again and np.array_equal(bits(dts), bits(dts_again))
                assert_same_bits(everything(ada), everything(fresh_ada))
                assert_same_bits(everything(rep), everything(fresh_ada))


def test_deciding_body_before_the_padding(gpu):
    """n = 1501: the last real body is an even half whose partner is padding.  n = 1025: a body at rest sits alone in the last
    live workgroup (511 padding slots beside it) and must not capture the minimum, which stays with the fast body in slot 0."""
    n = 1501
    with hermite_sim(gpu, n) as ada, hermite_sim(gpu, n) as rep:
        for t in (n - 1, n - 2, 0):
            decide(ada, rep, P.swapped(_fast(n), t), t)
    n = 1025
    s = {k: np.array(v) for k, v in _fast(n).items()}
    for k in P.V:
        s[k][n - 1] = 0.0
    with hermite_sim(gpu, n) as ada, hermite_sim(gpu, n) as rep:
        decide(ada, rep, s, 0)


# ---------------------------------------------------------------------------------------------- batch length and the ring
def test_evolve_batch_changes_nothing(gpu):
    """Galaxy, N = 2048, a free run of 360 000 s: "evolve_batch" 0 (automatic), 1, 3 and 64 give the same steps, the same
    result and the same bits — with 64 most of the last batch is no-op launches, and the state must still be in the buffer
    the host reads.  65 and negative values are refused."""
    n = 2048
    s = gpu.init_bodies(n, "galaxy")
    ref = None
    for batch in (0, 1, 3, 64):
        with hermite_sim(gpu, n, evolve_batch=batch) as sim:
            sim.upload(s)
            out = sim.evolve(360000.0)
            got = (out, sim.evolve_dts(), everything(sim))
            for bad in (65, -1, -64):
                with pytest.raises(gpu.MurbHipError) as e:
                    sim.set_option("evolve_batch", bad)
                assert e.value.code == E_INVALID
        if ref is None:
            ref = got
            assert out["time"] == 360000.0 and 4 <= out["steps"] == len(got[1]) < 64
            continue
        assert got[0] == ref[0], (batch, got[0], ref[0])
        assert np.array_equal(bits(got[1]), bits(ref[1])), batch
        assert_same_bits(got[2], ref[2], f"evolve_batch {batch}:")


def test_ring_wrap(gpu):
    """More steps than the ring holds, of widely varying size (equal ones would hide an index error): the eccentric binary over
    18 periods at eta 0.005.  One call against consecutive calls of 1000 steps: the ring read back after the long call is the
    last 4096 steps of the pieces, bit for bit, and the states agree."""
    s, duration = P.ring_run()
    with hermite_sim(gpu, 2, P.RING_SOFT) as a, hermite_sim(gpu, 2, P.RING_SOFT) as b:
        a.upload(s)
        b.upload(s)
        out = a.evolve(duration, eta=P.RING_ETA, dt_max=duration)
        pieces, t, calls = [], 0.0, 0
        while t < duration:
            part = b.evolve(duration - t, eta=P.RING_ETA, dt_max=duration, max_steps=1000)     # one clamp for every piece
            pieces.append(b.evolve_dts())
            assert part["steps"] == len(pieces[-1]) <= 1000
            t += part["time"]
            calls += 1
            assert calls <= 10
        whole = np.concatenate(pieces)
        print(f"{out['steps']} steps, dt {out['dt_min']:.6g} ... {out['dt_max']:.6g} s; {calls} calls of at most 1000 steps")
        assert t == duration and out["time"] == duration
        assert P.RING_STEPS[0] <= out["steps"] <= P.RING_STEPS[1] and out["dt_max"] / out["dt_min"] > 100.0
        assert out["steps"] == len(whole)
        kept = a.evolve_dts()
        assert len(kept) == P.RING
        assert np.array_equal(bits(kept), bits(whole[-P.RING:]))
        assert len(set(bits(kept).tolist())) > P.RING // 2          # the steps do vary
        assert_same_bits(everything(a), everything(b))
        # a buffer that cannot hold what is kept: refused, and the count says how much there is
        count = C.c_ulong(0)
        small = np.zeros(P.RING - 1, np.float32)
        assert gpu.lib().murbhip_evolve_dts(a._h, small.ctypes.data_as(C.POINTER(C.c_float)), len(small), C.byref(count)) == E_INVALID
        assert count.value == P.RING and not small.any()

"""Pair coverage of every force plan, checked body by body with sparse-mass probes (oracle.py: probe_*).  All tests here
need an MI355X.

A probe keeps a problem's positions and gives mass to at most 256 "source" bodies placed in slot space (every block,
the offsets where the kernels' tiles, packed pairs and item ends fall, both sides of every shard boundary).  The plan
and its work list depend on n, the shards and the options only, so a probe runs exactly the launches of the real
problem, while its fp64 truth costs O(n K): EVERY body is checked, and each source's term is a visible share of every
body's sum.  A pair that a kernel skips, counts twice, gives the wrong mass or the wrong position, or a reaction of the
wrong sign, is 10-1000x the tolerance (tests/test_probe_oracle.py shows it on the checker).  The error of body i is
measured against sum_s |c_is|, the limit is the dense tests' TOL_F64_MAX, and every probe asserts its own power: for
99 % of the bodies the smallest source term is at least 10x the tolerance.

The probes of one problem run back to back in ONE context, each with its sources in other slots than the one before:
a partial row, pass buffer or remembered force left over from the previous probe shows as an error."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
TOL_F64_MAX = 2e-6       # tests/test_gpu_parity.py, forces
TOL_PE_FUSED = 1e-7      # ... the potential out of the pair-symmetric force evaluation
TOL_PE_SWEEP = 5e-7      # ... the separate potential sweep
BLOCK = 1024             # MURB_SYM_BLOCK: slots per block of the pair-symmetric kernel

# plan defaults (csrc/murb_choose.h, PlanInputs; csrc/murb_ctx.h, murbhip_ctx): every forced configuration starts from these
DEFAULTS = dict(variant=0, jsplit=0, sym_waves=0, taper=-1, diag_tri=-1, sym_red=-1, pad_aware=1, xcd_order=0, sym_pass_mb=0,
                overlap=1, tri_div=0, tri_first_pct=50, energy_sweep=0)


class Problem:
    """One size and shard count: the base positions, the slot geometry, and the probes' source sets."""

    def __init__(self, gpu, O, n, world=1, scheme="galaxy", probes=2, k_max=256, per_block=8):
        self.O, self.n, self.world = O, n, world
        fc = [gpu.partition(n, world, r) for r in range(world)]
        self.firsts, self.counts = [f for f, _ in fc], [c for _, c in fc]
        self.slice = gpu.slice_slots(n, world)
        self.base = O.init_bodies(n, scheme)
        self.sources = O.probe_sources(n, self.firsts, self.counts, self.slice, probes, k_max, per_block)
        self.next = 0

    def slot(self, i):
        r = np.searchsorted(self.firsts, i, side="right") - 1
        return int(r * self.slice + (i - self.firsts[r]))

    def blocks_of(self, src):
        return {self.slot(int(i)) // BLOCK for i in src}

    def take(self):
        """The next probe (cyclic): (state, sources)."""
        k = self.next % len(self.sources)
        self.next += 1
        src = self.sources[k]
        return self.O.probe_state(self.base, src, seed=k), src

    def truth(self, ps, src):
        """fp64 accelerations and the term-magnitude sums, after asserting the probe's power to see one term."""
        a, abs_sum, min_term = self.O.accel_f64_sources(ps, src, SOFT)
        power = self.O.probe_power(abs_sum, min_term)
        assert (power >= 10 * TOL_F64_MAX).mean() >= 0.99, f"probe too weak: 1 % share {np.quantile(power, 0.01):.2e}"
        return a, abs_sum, power

    def check(self, got, truth, abs_sum, what):
        e = self.O.probe_err(got, truth, abs_sum)
        assert np.isfinite(e).all(), what
        worst = int(np.argmax(e))
        s = self.slot(worst)
        assert e[worst] <= TOL_F64_MAX, (f"{what}: body {worst} (slot {s}, block {s // BLOCK}, offset {s % BLOCK}) off by "
                                         f"{e[worst]:.3e} of its source terms; {(e > TOL_F64_MAX).sum()} bodies over")


def set_options(sim, **opts):
    for k, v in dict(DEFAULTS, **opts).items():
        sim.set_option(k, v)


def probe_forces(P, sim, what):
    """Upload the next probe, evaluate, check every body; returns the probe's sources."""
    ps, src = P.take()
    truth, abs_sum, _ = P.truth(ps, src)
    sim.upload(ps)
    sim.compute_acc()
    sim.sync()
    P.check(sim.acc(), truth, abs_sum, what)
    return src


def probe_step(P, sim, what):
    """The step route: the next probe with v = 0, one step, v / DT against the truth."""
    ps, src = P.take()
    truth, abs_sum, _ = P.truth(ps, src)
    sim.upload(ps)
    sim.step(DT)
    sim.sync()
    st = sim.state()
    P.check(tuple(st[k].astype(np.float64) / np.float64(DT) for k in ("vx", "vy", "vz")), truth, abs_sum, what + " (step)")
    return src


def probe_potential(P, sim, what, tol):
    """Upload the next probe, energy()[1] against the fp64 sum over its source pairs."""
    ps, src = P.take()
    pe, min_pair = P.O.potential_f64_sources(ps, src, SOFT)
    assert min_pair >= 10 * tol * abs(pe), f"potential probe too weak: {min_pair / abs(pe):.2e}"
    sim.upload(ps)
    _, got = sim.energy()
    assert abs(got - pe) <= tol * abs(pe), f"{what}: potential off by {(got - pe) / pe:.3e}"
    return src


# ---------------------------------------------------------------------------------------------------- block-count sweep
SWEEP_PLANS = {}   # n -> (variant, sym_waves, jsplit, taper) of the default plan


def sweep_sizes(T):
    """T blocks: full; 37 bodies short (no item is cut: 987 rounds up to 1024); and, from two blocks on, 65 bodies in the
    last block (its items cut to 128 of 1024 slots) and one body (cut to one granule)."""
    return (BLOCK * T, BLOCK * T - 37) + ((BLOCK * (T - 1) + 65, BLOCK * (T - 1) + 1) if T >= 2 else ())


@pytest.mark.parametrize("T", range(1, 31))
def test_block_count_sweep(gpu, O, T):
    """One GPU, the default plan at every block count T = 1 ... 30 (the small-plan table, the fused one-launch rule), full
    and with a ragged last block: compute_acc and the step route (the fused one-launch kernel for T <= 4 and T = 6)."""
    for n in sweep_sizes(T):
        P = Problem(gpu, O, n)
        with gpu.Simulation(n, soft=SOFT) as sim:
            SWEEP_PLANS[n] = tuple(int(sim.info(k)) for k in ("variant", "sym_waves", "jsplit", "taper"))
            covered = probe_forces(P, sim, f"n={n} plan {SWEEP_PLANS[n]}")
            covered = np.concatenate([covered, probe_step(P, sim, f"n={n} plan {SWEEP_PLANS[n]}")])
        assert P.blocks_of(covered) == set(range(T))


def test_block_count_sweep_reached_every_plan(gpu, O):
    """The sweep above must keep reaching every plan of the table: if an edit of kSmallPlanOfBlocks or of the fused rule
    leaves one out, this says so."""
    for T in range(1, 31):
        for n in sweep_sizes(T):
            if n not in SWEEP_PLANS:
                with gpu.Simulation(n, soft=SOFT) as sim:
                    SWEEP_PLANS[n] = tuple(int(sim.info(k)) for k in ("variant", "sym_waves", "jsplit", "taper"))
    plans = set(SWEEP_PLANS.values())
    print("block-count sweep reached (variant, sym_waves, jsplit, taper):", sorted(plans))
    assert {p[0] for p in plans} >= {1, 8}
    sym = [p for p in plans if p[0] == 8]
    assert {p[1] for p in sym} >= {4, 8}
    assert {p[2] for p in sym} >= {4, 8, 16}
    assert {p[3] for p in sym} >= {5, 30}


# ---------------------------------------------------------------------------------------------------- forced options
# every variant with its defaults, then the pair-symmetric kernel's knobs in a covering list (each value of each knob, most
# pairs of values): (sym_waves, jsplit, taper, diag_tri, sym_red, pad_aware, xcd_order)
SYM_COVER = [(4, 1, 0, 0, 0, 1, 0), (4, 2, 30, 1, 1, 0, 0), (4, 4, 100, 1, 0, 1, 0), (4, 8, 0, 1, 1, 1, 0), (4, 16, 30, 0, 1, 1, 0),
             (8, 1, 100, 1, 1, 1, 0), (8, 2, 0, 0, 1, 1, 0), (8, 4, 30, 1, 0, 0, 0), (8, 8, 100, 0, 0, 0, 0), (8, 16, 0, 1, 1, 0, 0),
             (4, 16, 100, 1, 0, 0, 0), (8, 4, 0, 0, 1, 1, 1), (4, 2, 30, 1, 1, 1, 1), (4, 8, 100, 0, 0, 1, 1)]
FORCED = [{}] + [dict(variant=v) for v in range(1, 9)] + [
    dict(variant=8, sym_waves=w, jsplit=j, taper=t, diag_tri=d, sym_red=r, pad_aware=p, xcd_order=x) for (w, j, t, d, r, p, x) in SYM_COVER]


@pytest.mark.parametrize("n", [12001, 30000])
def test_forced_options(gpu, O, n):
    """Every variant still settable through the ABI, and the pair-symmetric kernel's work-list knobs, one context."""
    P = Problem(gpu, O, n, probes=len(FORCED))
    with gpu.Simulation(n, soft=SOFT) as sim:
        for opts in FORCED:
            set_options(sim, **opts)
            probe_forces(P, sim, f"n={n} {opts}")


@pytest.mark.parametrize("n", [30000, 60001])
def test_multi_pass(gpu, O, n):
    """One GPU, partial rows larger than the per-pass budget: items evaluated in passes over j ranges of one buffer."""
    P = Problem(gpu, O, n, probes=4)
    Q = Problem(gpu, O, n, probes=2, k_max=64, per_block=2)
    with gpu.Simulation(n, soft=SOFT) as sim:
        for mb in (1, 2, 1, 2):
            set_options(sim, sym_pass_mb=mb)
            probe_forces(P, sim, f"n={n} sym_pass_mb={mb}")
            assert int(sim.info("variant")) == 8 and sim.info("sym_passes") >= 2, sim.info("sym_passes")
        for mb in (1, 2):
            set_options(sim, sym_pass_mb=mb)
            probe_potential(Q, sim, f"n={n} sym_pass_mb={mb}", TOL_PE_FUSED)
            assert sim.info("sym_passes") >= 2


# ---------------------------------------------------------------------------------------------------- benchmark sizes
@pytest.mark.parametrize("n", [200000, 1000000, 2000003])
def test_benchmark_sizes(gpu, O, n):
    """BASELINE sizes on one GPU with the default plan: every body of every probe, every block holding a source."""
    P = Problem(gpu, O, n, probes=2)
    covered, margins = [], []
    with gpu.Simulation(n, soft=SOFT) as sim:
        assert int(sim.info("variant")) == 8
        for _ in range(len(P.sources)):
            ps, src = P.take()
            truth, abs_sum, power = P.truth(ps, src)
            margins.append((np.quantile(power, 0.01) / TOL_F64_MAX, power.min() / TOL_F64_MAX))
            sim.upload(ps)
            sim.compute_acc()
            sim.sync()
            P.check(sim.acc(), truth, abs_sum, f"n={n} probe {len(covered)}")
            covered.append(src)
    assert P.blocks_of(np.concatenate(covered)) == set(range(P.slice // BLOCK))
    print(f"n={n}: {len(covered)} probes; sensitivity margin (smallest term share / tol) at the 1 % quantile "
          f"{min(m[0] for m in margins):.1f}, over all bodies {min(m[1] for m in margins):.2f}")


# ---------------------------------------------------------------------------------------------------- shards
SHARD_COVER = [dict(), dict(variant=1, overlap=0), dict(variant=1, overlap=1), dict(variant=8, overlap=0),
               dict(variant=8, overlap=1, tri_div=2, tri_first_pct=0), dict(variant=8, overlap=2, tri_div=8, tri_first_pct=100),
               dict(variant=8, overlap=1, tri_div=8, tri_first_pct=100), dict(variant=8, overlap=2, tri_div=2, tri_first_pct=0)]


@pytest.mark.parametrize("shards", [2, 3, 4, 8])
@pytest.mark.parametrize("n", [6151, 30000])
def test_shards_time_sharing_one_gpu(gpu, O, n, shards):
    """Body-range shards on one GPU (peer-copy exchange): the one-sided and half-ring pair-symmetric schedules, the
    exchange pipeline's options; sources on both sides of every shard boundary."""
    P = Problem(gpu, O, n, world=shards, probes=len(SHARD_COVER))
    with gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as sim:
        for opts in SHARD_COVER:
            set_options(sim, **opts)
            if not opts:
                assert int(sim.info("variant")) in (2, 8)
            probe_forces(P, sim, f"n={n} shards={shards} {opts}")


def test_shards_benchmark_size(gpu, O):
    n, shards = 200000, 8
    P = Problem(gpu, O, n, world=shards, probes=2)
    covered = []
    with gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as sim:
        assert int(sim.info("variant")) == 8
        for _ in range(len(P.sources)):
            covered.append(probe_forces(P, sim, f"n={n} shards={shards}"))
    assert P.blocks_of(np.concatenate(covered)) == set(range(shards * P.slice // BLOCK))


# ---------------------------------------------------------------------------------------------------- potential
@pytest.mark.parametrize("n,shards,opts,tol", [(5000, 1, {}, TOL_PE_FUSED), (12001, 1, {}, TOL_PE_FUSED), (27000, 1, {}, TOL_PE_FUSED),
                                               (200000, 1, {}, TOL_PE_FUSED), (30000, 3, dict(variant=8), TOL_PE_FUSED),
                                               (1500, 1, {}, TOL_PE_SWEEP), (2048, 1, {}, TOL_PE_SWEEP),
                                               (12001, 1, dict(energy_sweep=1), TOL_PE_SWEEP)])
def test_potential(gpu, O, n, shards, opts, tol):
    """energy()[1] of probes with at most 64 sources (one missing pair >= 10x the tolerance), several sources per block so
    that the diagonal pieces and the diagonal-block potential kernel carry pairs: the potential out of the pair-symmetric
    force evaluation, over 3 shards, and the separate sweep (few bodies, "energy_sweep" 1)."""
    P = Problem(gpu, O, n, world=shards, probes=3, k_max=64, per_block=4)
    kw = {"devices": [0] * shards} if shards > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as sim:
        set_options(sim, **opts)
        if n <= 2048:
            assert int(sim.info("variant")) == 1
        for _ in range(len(P.sources)):
            probe_potential(P, sim, f"n={n} shards={shards} {opts}", tol)
    assert any(len(P.blocks_of(src)) < len(src) for src in P.sources)   # some block held two sources or more


# ---------------------------------------------------------------------------------------------------- caches
@pytest.mark.parametrize("n,devices", [(3000, [0]), (12001, [0]), (30000, [0, 0])])
def test_no_stale_forces_or_potential_across_uploads(gpu, O, n, devices):
    """compute_acc -> upload(next probe) -> compute_acc; energy -> upload -> energy; energy -> step -> energy: whatever the
    context remembers of one state (forces, the pair potential, metric sums, partial rows) must not leak into the next."""
    P = Problem(gpu, O, n, world=len(devices), probes=4, k_max=64, per_block=2)
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as sim:
        for k in range(2):
            ps, src = P.take()
            sim.upload(ps)
            sim.compute_acc()
            sim.sync()
            ps, src = P.take()
            truth, abs_sum, _ = P.truth(ps, src)
            sim.upload(ps)
            sim.compute_acc()
            sim.sync()
            P.check(sim.acc(), truth, abs_sum, f"n={n} compute_acc -> upload -> compute_acc")
        probe_potential(P, sim, f"n={n} energy", TOL_PE_SWEEP)
        ps, src = P.take()
        sim.energy()
        pe, _ = O.potential_f64_sources(ps, src, SOFT)
        sim.upload(ps)
        _, got = sim.energy()
        assert abs(got - pe) <= TOL_PE_SWEEP * abs(pe), f"energy -> upload -> energy: {(got - pe) / pe:.3e}"
        # with the probe's own velocities the step moves the sources by ~1 % of their distances: the potential changes by far
        # more than the tolerance, so a remembered one shows
        ps = O.probe_state(P.base, src, seed=7, zero_velocities=False)
        pe, _ = O.potential_f64_sources(ps, src, SOFT)
        sim.upload(ps)
        _, got = sim.energy()
        assert abs(got - pe) <= TOL_PE_SWEEP * abs(pe)
        sim.step(DT)
        _, got = sim.energy()
        st = dict(sim.state(), m=ps["m"])
        pe2, _ = O.potential_f64_sources(st, src, SOFT)
        assert abs(pe2 - pe) > 10 * TOL_PE_SWEEP * abs(pe)
        assert abs(got - pe2) <= TOL_PE_SWEEP * abs(pe2), f"energy -> step -> energy: {(got - pe2) / pe2:.3e}"

"""Parity of the HIP path (through the C ABI, include/murbhip.h) against the CPU oracle and the
committed reference fixtures.  All tests here need an MI355X.

Tolerances (fp32; relative vector error per body, |a_gpu - a_ref| / |a_ref|):
  * vs the fp64 direct sum ("truth"):            max <= 2e-6   — the GPU sums in 128 x jsplit partial
    sums per body, so it sits closer to the truth than cpu+optim itself (1.2e-5 max at N=30000);
  * vs cpu+optim (the reference's parity oracle), galaxy scheme: max <= 3e-5, rms <= 1e-5 — this is
    cpu+optim's own rounding noise (sequential fp32 sums + rsqrtss/Newton), BASELINE.json's "within
    1e-5 rel" holds in rms;
  * vs cpu+optim, random scheme: max <= 2e-3, rms <= 5e-5.  The reference executable runs
    flush-to-zero and forms G*inv^3 first (SimulationNBodyOptim.cpp:69): for pairs farther apart than
    ~1.8e9 m that product is subnormal and becomes 0, so ~1 % of the bodies of the `random` box lose
    up to 9e-4 of their acceleration IN THE REFERENCE (oracle/ftz.h).  The GPU forms GM_j*inv*inv^2 and
    keeps those pairs; it is held to the fp64 truth at 2e-6 there as everywhere else;
  * positions after k <= 5 steps vs cpu+optim:   max relative component error <= 2e-6 (positions
    ~1e8 m move ~1e6 m per step, so acceleration noise enters at the 1e-7 level);
  * the reference's own test tolerances (test_SimulationNBody.cpp:76-81: 1e-3 random / 1e-1 galaxy
    vs cpu+naive) are asserted as well;
  * integrator alone: bit exact.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
TOL_F64_MAX = 2e-6
TOL_OPTIM = {"galaxy": (3e-5, 1e-5), "random": (2e-3, 5e-5)}   # (max, rms) vs cpu+optim
TOL_POS = 2e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_acc(gpu, s, **opts):
    with gpu.Simulation(len(s["qx"]), soft=SOFT) as sim:
        for k, v in opts.items():
            sim.set_option(k, v)
        sim.upload(s)
        sim.compute_acc()
        sim.sync()
        return sim.acc()


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
@pytest.mark.parametrize("n", [2048, 2049, 4000, 12001, 30000])
def test_acceleration_vs_oracles(gpu, O, scheme, n):
    s = O.init_bodies(n, scheme)
    a = gpu_acc(gpu, s)
    assert all(np.isfinite(c).all() for c in a)
    truth = O.accel_f64(s, SOFT)
    e64 = O.rel_err(a, truth)
    assert e64.max() <= TOL_F64_MAX, f"vs fp64: max {e64.max():.3e}"
    opt = O.accel_optim(s, SOFT)
    eo = O.rel_err(a, opt)
    assert eo.max() <= TOL_OPTIM[scheme][0] and np.sqrt((eo ** 2).mean()) <= TOL_OPTIM[scheme][1], \
        f"vs cpu+optim: max {eo.max():.3e} rms {np.sqrt((eo ** 2).mean()):.3e}"
    # the GPU result must be at least as close to the truth as the reference's own CPU path
    assert e64.max() <= max(O.rel_err(opt, truth).max(), 1e-6)


# the four sections of the reference's hot-path test (src/test/implem/test_SimulationNBody.cpp:73-82)
@pytest.mark.parametrize("n,iters,scheme,eps", [(2048, 1, "random", 1e-3), (2049, 3, "random", 1e-3),
                                                (2048, 4, "galaxy", 1e-1), (2049, 3, "galaxy", 1e-1)])
def test_reference_test_sections(gpu, O, n, iters, scheme, eps):
    s_naive = O.init_bodies(n, scheme)
    s_opt = {k: v.copy() for k, v in s_naive.items()}
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s_naive)
        st = sim.state()
        for k in ("qx", "qy", "qz"):     # step 0: exact (test_SimulationNBody.cpp:63)
            assert np.array_equal(bits(st[k]), bits(s_naive[k]))
        for it in range(iters):
            O.simulate(s_naive, 1, "cpu+naive", SOFT, DT)
            O.simulate(s_opt, 1, "cpu+optim", SOFT, DT)
            sim.step(DT)
            sim.sync()
            st = sim.state()
            for k in ("qx", "qy", "qz"):
                np.testing.assert_allclose(st[k], s_naive[k], rtol=eps, atol=0)      # the reference's bar
                np.testing.assert_allclose(st[k], s_opt[k], rtol=TOL_POS, atol=1.0)  # ours (atol: 1 m of 1e8)
            # velocities change by a*dt per step: cpu+optim's acceleration noise (TOL_OPTIM) times that
            vtol = TOL_OPTIM[scheme][0] * (it + 1) * float(DT) * max(np.abs(c).max() for c in O.accel_optim(s_opt, SOFT))
            for k in ("vx", "vy", "vz"):
                np.testing.assert_allclose(st[k], s_opt[k], rtol=1e-5, atol=vtol)


@pytest.mark.parametrize("scheme,n", [("random", 2048), ("random", 2049), ("galaxy", 2048), ("galaxy", 2049)])
def test_against_reference_fixtures(gpu, scheme, n):
    g = np.load(os.path.join(GOLDEN, f"ref_{scheme}_{n}.npz"))
    s = {k: g["init_" + k][:n] for k in ("qx", "qy", "qz", "vx", "vy", "vz", "m")}
    iters = int(g["iters"][0])
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        sim.step(DT)
        sim.sync()
        a = sim.acc()
        ref_a = [g["optim_acc1_a" + c] for c in "xyz"]
        num = np.sqrt(sum((np.float64(x) - np.float64(y)) ** 2 for x, y in zip(a, ref_a)))
        den = np.sqrt(sum(np.float64(y) ** 2 for y in ref_a))
        assert (num / den).max() <= TOL_OPTIM[scheme][0]
        assert np.sqrt(((num / den) ** 2).mean()) <= TOL_OPTIM[scheme][1]
        st = sim.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(st[k], g["optim_step1_" + k], rtol=TOL_POS, atol=1.0)
        if iters > 1:
            sim.steps(DT, iters - 1)
            sim.sync()
            st = sim.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(st[k], g["optim_final_" + k], rtol=TOL_POS, atol=1.0)
            np.testing.assert_allclose(st[k], g["naive_final_" + k], rtol=1e-3 if scheme == "random" else 1e-1)


# src/test/implem/test_CUDABodies.cpp:42-75 — integrator alone, synthetic accelerations, bit exact
@pytest.mark.parametrize("scheme", ["random", "galaxy"])
def test_integrator_bit_exact(gpu, O, scheme):
    n = 4000
    s = O.init_bodies(n, scheme)
    acc = (np.arange(1, n + 1, dtype=np.float32), np.full(n, 3.0, np.float32), (n - np.arange(n)).astype(np.float32))
    g = np.load(os.path.join(GOLDEN, f"ref_integrator_{scheme}_{n}.npz"))
    ref = {k: v.copy() for k, v in s.items()}
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        st = sim.state()
        for k in ("qx", "qy", "qz", "vx", "vy", "vz"):   # test_cuda_bodies: upload/download round trip
            assert np.array_equal(bits(st[k]), bits(s[k]))
        for step in range(1, 5):
            sim.integrate_host_acc(acc, np.float32(0.01))
            O.integrate(ref, acc, np.float32(0.01))
            st = sim.state()
            for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
                assert np.array_equal(bits(st[k]), bits(ref[k])), f"{k} differs at step {step}"
                if step in (1, 4):
                    assert np.array_equal(bits(st[k]), bits(g[f"steps{step}_{k}"]))


def test_integrator_bit_exact_real_accelerations(gpu, O):
    """dt = 3600 with the device's own accelerations: positions ~1e8, fp64 intermediates matter."""
    n = 3001
    s = O.init_bodies(n, "galaxy")
    ref = {k: v.copy() for k, v in s.items()}
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        for _ in range(3):
            sim.step(DT)
            sim.sync()
            O.integrate(ref, sim.acc(), DT)
            st = sim.state()
            for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
                assert np.array_equal(bits(st[k]), bits(ref[k]))


def test_variants_and_jsplit_agree(gpu, O):
    n = 5000
    s = O.init_bodies(n, "galaxy")
    truth = O.accel_f64(s, SOFT)
    base = gpu_acc(gpu, s)
    for variant in range(1, 9):
        for jsplit in ((1, 2, 4) if variant == 8 else (1, 3, 7)):
            a = gpu_acc(gpu, s, variant=variant, jsplit=jsplit)
            assert O.rel_err(a, truth).max() <= TOL_F64_MAX, (variant, jsplit)
            assert O.rel_err(a, base).max() <= 2e-6
    # the pair-symmetric kernel's workgroup shapes and item sizes ("sym_waves" x "jsplit")
    for waves in (4, 8):
        for jsplit in (1, 4, 8, 16):
            a = gpu_acc(gpu, s, variant=8, sym_waves=waves, jsplit=jsplit)
            assert O.rel_err(a, truth).max() <= TOL_F64_MAX, (waves, jsplit)
    # bit-reproducible run to run (partial sums are added in a fixed order, no atomics)
    again = gpu_acc(gpu, s)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(base, again))


@pytest.mark.parametrize("n,budget_mb,opts", [(12001, 1, {}), (30000, 4, {}), (30000, 2, {"taper": 40, "diag_tri": 1, "sym_waves": 8, "jsplit": 4}),
                                              (20000, 1, {"integrator": 1}),
                                              # the XCD-interleaved item order scatters a j column over the table; passes are cut
                                              # at column boundaries, so a multi-pass plan must fall back to the j-major order
                                              (30000, 2, {"xcd_order": 1, "taper": 40, "diag_tri": 1, "jsplit": 4}), (20000, 1, {"xcd_order": 1})])
def test_multi_pass_evaluation(gpu, O, n, budget_mb, opts):
    """One GPU, partial sums larger than the per-pass budget ("sym_pass_mb"; by default a quarter of the HBM, reached
    beyond ~2.4 M bodies): the items are evaluated in several passes over ranges of j columns sharing one buffer, row sums
    accumulated in fp64.  Forced here at small N: forces, potential and a few steps against the single-pass run."""
    s = O.init_bodies(n, "galaxy")
    truth = O.accel_f64(s, SOFT)
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT) as multi:
        for sim in (one, multi):
            sim.set_option("variant", 8)
            for k, v in opts.items():
                sim.set_option(k, v)
        multi.set_option("sym_pass_mb", budget_mb)
        for sim in (one, multi):
            sim.upload(s)
            sim.compute_acc()
            sim.sync()
        assert one.info("sym_passes") == 1 and multi.info("sym_passes") >= 3, multi.info("sym_passes")
        assert multi.info("device_bytes") < one.info("device_bytes")
        assert O.rel_err(multi.acc(), truth).max() <= TOL_F64_MAX
        # same partial sums, fp64 additions regrouped; with "xcd_order" the single-pass run keeps the interleaved item order
        # (other tail items, other partial sums) while the passes fall back to the j-major one: fp32 noise between them
        assert O.rel_err(multi.acc(), one.acc()).max() <= (6e-7 if opts.get("xcd_order") else 2e-7)
        # both take the pair potential out of their force evaluation (the multi-pass one adds the groups' sums up pass by pass:
        # every pass has a layout of its own in the shared buffer) — and no second N^2 launch for it in either
        ke, pe = O.energy_f64(s, SOFT)
        for sim in (one, multi):
            sim.set_option("profile", 1)
        (k1, p1), (k2, p2) = one.energy(), multi.energy()
        assert abs(p1 - pe) <= 1e-7 * abs(pe) and abs(p2 - pe) <= 1e-7 * abs(pe), ((p1 - pe) / pe, (p2 - pe) / pe)
        assert abs(k2 - k1) <= 1e-12 * abs(k1) and abs(k1 - ke) <= 1e-9 * abs(ke)
        assert one.info("sym_launches") == 1 and multi.info("sym_launches") == multi.info("sym_passes")
        (k3, p3) = multi.energy()                      # nothing changed: the remembered sums, no launch
        assert p3 == p2 and multi.info("sym_launches") == multi.info("sym_passes")
        multi.set_option("energy_sweep", 1)            # the separate sweep of rounds 1-2 as a cross-check
        (k4, p4) = multi.energy()
        assert abs(p4 - pe) <= 5e-7 * abs(pe)
        multi.set_option("energy_sweep", 0)
        for sim in (one, multi):
            sim.set_option("profile", 0)
        one.steps(DT, 3); multi.steps(DT, 3)
        one.sync(); multi.sync()
        s1, s2 = one.state(), multi.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(s2[k], s1[k], rtol=6e-7 if opts.get("xcd_order") else 2e-7, atol=1.0)


@pytest.mark.parametrize("scheme,n", [("galaxy", 12001), ("random", 6151), ("galaxy", 30000)])
def test_pair_symmetric_item_shapes_and_reductions(gpu, O, scheme, n):
    """The knobs of the pair-symmetric kernel's work list — tapered item sizes ("taper"), diagonal blocks as triangular
    pieces ("diag_tri"), the i-side reduction through LDS ("sym_red"), 4 or 8 waves — change the order of the sums, never
    the physics: every combination is held to the fp64 truth, one GPU and two shards, forces and the potential sweep."""
    s = O.init_bodies(n, scheme)
    truth = O.accel_f64(s, SOFT)
    ke, pe = O.energy_f64(s, SOFT)
    combos = [dict(taper=t, diag_tri=d, sym_red=r, sym_waves=w, jsplit=j)
              for (t, d, r, w, j) in [(0, 0, 0, 4, 4), (50, 0, 0, 4, 2), (0, 1, 0, 4, 1), (0, 1, 0, 8, 8), (0, 0, 1, 4, 2), (0, 0, 1, 8, 8),
                                      (100, 1, 1, 4, 1), (40, 1, 1, 8, 4), (30, 1, 1, 4, 16), (5, 1, 1, 4, 1), (60, 1, 0, 8, 2)]]
    for opts in combos:
        with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, devices=[0, 0]) as two:
            for sim in (one, two):
                sim.set_option("variant", 8)
                for k, v in opts.items():
                    sim.set_option(k, v)
                sim.upload(s)
                sim.compute_acc()
                sim.sync()
                assert O.rel_err(sim.acc(), truth).max() <= TOL_F64_MAX, (opts, sim is two)
            k1, p1 = one.energy()
            assert abs(p1 - pe) <= 2e-6 * abs(pe) and abs(k1 - ke) <= 2e-6 * abs(ke), opts
            # and a few steps: the row sums feed the integrator
            one.steps(DT, 2); two.steps(DT, 2)
            one.sync(); two.sync()
            s1, s2 = one.state(), two.state()
            for k in ("qx", "qy", "qz"):
                np.testing.assert_allclose(s2[k], s1[k], rtol=TOL_POS, atol=1.0)


@pytest.mark.parametrize("soft", [1e3, 1e6, 1e7, 1e10])
@pytest.mark.parametrize("variant", [1, 8])
def test_other_softening_lengths(gpu, O, soft, variant):
    """--soft is a CLI parameter of the reference (main.cpp:111,144-151): small values make close pairs
    dominate (and fp32 differences of 1e8-sized coordinates noisy for every implementation), large ones
    flatten the field.  The GPU must stay as close to the fp64 truth as cpu+optim does."""
    n = 3000
    s = O.init_bodies(n, "galaxy")
    soft = np.float32(soft)
    truth = O.accel_f64(s, soft)
    opt_err = O.rel_err(O.accel_optim(s, soft), truth).max()
    with gpu.Simulation(n, soft=soft) as sim:
        sim.set_option("variant", variant)
        sim.upload(s)
        sim.compute_acc()
        sim.sync()
        a = sim.acc()
    assert all(np.isfinite(c).all() for c in a)
    assert O.rel_err(a, truth).max() <= max(TOL_F64_MAX, 2.0 * opt_err)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 513])
def test_tiny_and_ragged_sizes(gpu, O, n):
    s = O.init_bodies(n, "random")
    a = gpu_acc(gpu, s)
    truth = O.accel_f64(s, SOFT)
    if n == 1:
        assert all(float(c[0]) == 0.0 for c in a)     # the self term is exactly 0
    else:
        assert O.rel_err(a, truth).max() <= TOL_F64_MAX


def test_massless_bodies_do_not_pull(gpu, O):
    """SIMD padding bodies of the reference carry m = 0 (Bodies.cpp:201-213): no influence."""
    n = 1500
    s = O.init_bodies(n, "galaxy")
    s2 = {k: np.concatenate([v, O.init_bodies(7, "random")[k]]) for k, v in s.items()}
    s2["m"][n:] = 0
    a = gpu_acc(gpu, s)
    a2 = gpu_acc(gpu, s2)
    assert all(np.array_equal(bits(x), bits(y[:n])) for x, y in zip(a, a2))


@pytest.mark.parametrize("shards", [2, 3, 4, 8])
@pytest.mark.parametrize("variant,overlap,jsplit", [(1, 1, 0), (1, 0, 0), (8, 1, 0), (8, 0, 1), (8, 1, 2), (8, 2, 0), (8, 2, 4),
                                                    (8, 125, 0), (8, 200, 0)])   # overlap >= 100: overlap 1 with tri_first_pct = overlap - 100
def test_sharded_matches_single(gpu, O, shards, variant, overlap, jsplit):
    """Body-range partition + per-step position exchange, several shards time-sharing one GPU.
    variant 1: every rank sweeps all j for its own i slice (one-sided).  variant 8: half-ring
    pair-symmetric schedule, every body pair evaluated by exactly one rank, accelerations combined by a
    reduce-scatter (here its peer-read emulation)."""
    n = 6151   # uneven slices
    s = O.init_bodies(n, "galaxy")
    truth = O.accel_f64(s, SOFT)
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as many:
        one.set_option("variant", 1)
        many.set_option("variant", variant)
        many.set_option("overlap", 1 if overlap >= 100 else overlap)
        if overlap >= 100:
            many.set_option("tri_first_pct", overlap - 100)
        many.set_option("jsplit", jsplit)   # variant 8: i-side sub-blocks per item (0 = auto)
        one.upload(s)
        many.upload(s)
        many.compute_acc()
        many.sync()
        assert O.rel_err(many.acc(), truth).max() <= TOL_F64_MAX
        for _ in range(4):
            one.step(DT)
            many.step(DT)
        one.sync()
        many.sync()
        a1, a2 = one.acc(), many.acc()
        assert O.rel_err(a2, a1).max() <= 2e-6
        s1, s2 = one.state(), many.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(s2[k], s1[k], rtol=TOL_POS, atol=1.0)
        for k in ("vx", "vy", "vz"):
            np.testing.assert_allclose(s2[k], s1[k], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shards", [2, 4, 8])
def test_sharded_benchmark_size(gpu, O, shards):
    """N = 200 000 cut over 2/4/8 shards (BASELINE configs[3]) with the library's own choice of
    schedule (half-ring pair-symmetric, auto split): spot check against the fp64 truth, momentum
    balance, and two steps against the single-GPU run."""
    n = 200000
    s = O.init_bodies(n, "galaxy")
    idx = np.random.default_rng(11).choice(n, 1024, replace=False)
    truth = O.accel_f64_subset(s, idx, SOFT)
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as many:
        assert many.info("variant") == 8
        one.upload(s)
        many.upload(s)
        many.compute_acc()
        many.sync()
        a = many.acc()
        assert O.rel_err(tuple(c[idx] for c in a), truth).max() <= TOL_F64_MAX
        m = s["m"].astype(np.float64)
        tot = np.array([(m * c.astype(np.float64)).sum() for c in a])
        scale = np.array([(m * np.abs(c.astype(np.float64))).sum() for c in a])
        assert (np.abs(tot) / scale).max() <= 1e-6
        one.steps(DT, 2)
        many.steps(DT, 2)
        one.sync()
        many.sync()
        s1, s2 = one.state(), many.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(s2[k], s1[k], rtol=TOL_POS, atol=1.0)


def test_sharded_config4_one_million_over_8_shards(gpu, O):
    """BASELINE.json configs[4]: N = 1 000 000 cut over 8 shards (here time-sharing one GPU, peer-copy exchange), the
    library's own choice of schedule: spot check against the fp64 truth, momentum balance, per-shard footprint, and two
    steps against the single-GPU run."""
    n, shards = 1000000, 8
    s = O.init_bodies(n, "galaxy")
    idx = np.random.default_rng(12).choice(n, 1024, replace=False)
    truth = O.accel_f64_subset(s, idx, SOFT)
    with gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as many:
        assert many.info("variant") == 8 and many.info("world") == shards
        many.upload(s)
        many.compute_acc()
        many.sync()
        a = many.acc()
        assert O.rel_err(tuple(c[idx] for c in a), truth).max() <= TOL_F64_MAX
        m = s["m"].astype(np.float64)
        tot = np.array([(m * c.astype(np.float64)).sum() for c in a])
        scale = np.array([(m * np.abs(c.astype(np.float64))).sum() for c in a])
        assert (np.abs(tot) / scale).max() <= 1e-6
        many.steps(DT, 2)
        many.sync()
        s2 = many.state()
        per_shard = many.info("device_bytes") / shards
    with gpu.Simulation(n, soft=SOFT) as one:
        one.upload(s)
        one.steps(DT, 2)
        one.sync()
        s1 = one.state()
        single = one.info("device_bytes")
    for k in ("qx", "qy", "qz"):
        np.testing.assert_allclose(s2[k], s1[k], rtol=TOL_POS, atol=1.0)
    vscale = max(np.abs(s1[k]).max() for k in ("vx", "vy", "vz"))
    for k in ("vx", "vy", "vz"):
        assert np.abs(s2[k] - s1[k]).max() <= 2e-5 * vscale, k
    # a rank only holds the partial-sum rows it writes: well under a third of the single-GPU footprint
    assert per_shard < 0.3 * single, (per_shard, single)


def test_cu_reserve_changes_nothing_but_the_streams(gpu, O):
    """"cu_reserve": the compute streams are re-created with a CU mask (CUs left to the exchange stream's kernels);
    results stay bit-identical, the option can be switched back and forth mid-run."""
    n = 20000
    s = O.init_bodies(n, "galaxy")
    with gpu.Simulation(n, soft=SOFT) as a, gpu.Simulation(n, soft=SOFT, devices=[0, 0]) as b, gpu.Simulation(n, soft=SOFT) as ref:
        for sim in (a, b, ref):
            sim.upload(s)
        a.set_option("cu_reserve", 8)
        b.set_option("cu_reserve", 16)
        assert a.info("cu_reserve") == 8 and b.info("cu_reserve") == 16
        for sim in (a, b, ref):
            sim.steps(DT, 2)
        a.set_option("cu_reserve", 0)
        for sim in (a, b, ref):
            sim.steps(DT, 1)
            sim.sync()
        sa, sb, sr = a.state(), b.state(), ref.state()
        for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
            assert np.array_equal(bits(sa[k]), bits(sr[k])), k
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(sb[k], sr[k], rtol=TOL_POS, atol=1.0)
        with pytest.raises(gpu.MurbHipError):
            a.set_option("cu_reserve", 100000)


def test_rank_mode_single_rank(gpu, O):
    """One process per GPU entry point with world = 1 (RCCL not needed, same results)."""
    n = 2048
    s = O.init_bodies(n, "galaxy")
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, rank=0, world=1, uid=None) as r0:
        one.upload(s); r0.upload(s)
        one.steps(DT, 2); r0.steps(DT, 2)
        one.sync(); r0.sync()
        for k, v in one.state().items():
            assert np.array_equal(bits(v), bits(r0.state()[k]))


def test_rccl_binding_single_rank(gpu, O):
    """dlopen'd RCCL end to end on one GPU: unique id, a 1-rank communicator, in-place all-gather of the
    rank's slice every step on the second stream — results identical to the plain single-GPU run."""
    n = 3000
    s = O.init_bodies(n, "galaxy")
    uid = gpu.unique_id()
    assert len(uid) == 128 and any(uid)
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, rank=0, world=1, uid=uid) as r0:
        r0.set_option("force_exchange", 1)
        one.upload(s); r0.upload(s)
        one.steps(DT, 5); r0.steps(DT, 5)
        one.sync(); r0.sync()
        a, b = one.state(), r0.state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    # the pair-symmetric multi-rank path: item table + row sum + ncclReduceScatter (1 rank) + all-gather
    uid = gpu.unique_id()   # a unique id founds exactly one communicator
    with gpu.Simulation(n, soft=SOFT) as one, gpu.Simulation(n, soft=SOFT, rank=0, world=1, uid=uid) as r0:
        one.set_option("variant", 8)
        r0.set_option("variant", 8)
        r0.set_option("force_exchange", 1)
        one.upload(s); r0.upload(s)
        one.steps(DT, 3); r0.steps(DT, 3)
        one.sync(); r0.sync()
        a, b = one.state(), r0.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(b[k], a[k], rtol=TOL_POS, atol=1.0)


@pytest.mark.parametrize("scheme,n", [("galaxy", 5000), ("random", 3001), ("galaxy", 30000)])
def test_energy_metric(gpu, O, scheme, n):
    """the energy metric of the reference's gpu+tracking implementation
    (SimulationNBodyCUDAPropertyTracking.cu:217-304) against an fp64 evaluation, before and after
    stepping.  The reference's integrator is not symplectic: over 10 steps of an hour the galaxy drifts
    by ~3e-4 of its energy, on the GPU exactly as on the cpu+optim trajectory."""
    s = O.init_bodies(n, scheme)
    ke0, pe0 = O.energy_f64(s, SOFT)
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        ke, pe = sim.energy()
        assert abs(ke - ke0) <= 1e-6 * abs(ke0) and abs(pe - pe0) <= 2e-6 * abs(pe0)
        sim.steps(DT, 10)
        ke1, pe1 = sim.energy()
        st = sim.state()
    st["m"] = s["m"]
    ke2, pe2 = O.energy_f64(st, SOFT)
    assert abs(ke1 - ke2) <= 1e-6 * abs(ke2) and abs(pe1 - pe2) <= 2e-6 * abs(pe2)
    assert abs((ke1 + pe1) - (ke0 + pe0)) <= 2e-3 * abs(ke0 + pe0)
    if n <= 5000:   # same drift as the reference's own CPU trajectory
        ref = {k: v.copy() for k, v in s.items()}
        O.simulate(ref, 10, "cpu+optim", SOFT, DT)
        ke4, pe4 = O.energy_f64(ref, SOFT)
        assert abs((ke1 + pe1) - (ke4 + pe4)) <= 2e-6 * abs(ke4 + pe4)
    # sharded: every shard evaluates its own bodies against all positions
    with gpu.Simulation(n, soft=SOFT, devices=[0, 0, 0]) as many:
        many.upload(s)
        ke3, pe3 = many.energy()
        assert abs(ke3 - ke0) <= 1e-6 * abs(ke0) and abs(pe3 - pe0) <= 2e-6 * abs(pe0)
    # sharded under the half-ring schedule: the potential sweep is pair-symmetric too (every pair term once, one
    # reduce-scatter), before and after steps, and the step pipeline carries on unharmed after it
    for shards in (2, 3, 4):
        with gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as many:
            many.set_option("variant", 8)
            many.upload(s)
            ke3, pe3 = many.energy()
            assert abs(ke3 - ke0) <= 1e-6 * abs(ke0) and abs(pe3 - pe0) <= 2e-6 * abs(pe0), shards
            many.steps(DT, 5)
            ke5, pe5 = many.energy()
            many.steps(DT, 5)
            ke6, pe6 = many.energy()
            assert abs(ke6 - ke2) <= 2e-6 * abs(ke2) and abs(pe6 - pe2) <= 4e-6 * abs(pe2), shards
            st6 = many.state()
            scale = max(np.abs(st[k]).max() for k in ("qx", "qy", "qz"))
            for k in ("qx", "qy", "qz"):   # ten steps, two summation orders: relative to the size of the system, not of the component
                assert np.abs(st6[k] - st[k]).max() <= TOL_POS * scale, (shards, k)


def test_long_run_stays_on_the_reference_trajectory(gpu, O):
    """200 iterations (the benchmark's -i 200) at N = 2048: positions still agree with cpu+optim to 1e-5,
    the energy drifts like the reference's, momentum is conserved, state survives re-upload."""
    n = 2048
    s = O.init_bodies(n, "galaxy")
    ref = {k: v.copy() for k, v in s.items()}
    O.simulate(ref, 200, "cpu+optim", SOFT, DT)
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        sim.steps(DT, 120)
        mid = sim.state()          # download in the middle of a run, then continue from a fresh upload
        mid["m"] = s["m"]
        sim.upload(mid)
        sim.steps(DT, 80)
        st = sim.state()
        ke, pe = sim.energy()
    for k in ("qx", "qy", "qz"):
        np.testing.assert_allclose(st[k], ref[k], rtol=1e-5, atol=1.0e3)   # 1e-5 of the 1e8 m scale
    ke_r, pe_r = O.energy_f64(ref, SOFT)
    assert abs((ke + pe) - (ke_r + pe_r)) <= 1e-5 * abs(ke_r + pe_r)
    m = s["m"].astype(np.float64)
    p0 = np.array([(m * s[k].astype(np.float64)).sum() for k in ("vx", "vy", "vz")])
    p1 = np.array([(m * st[k].astype(np.float64)).sum() for k in ("vx", "vy", "vz")])
    scale = (m * np.abs(st["vx"].astype(np.float64))).sum()
    assert np.abs(p1 - p0).max() <= 1e-5 * scale


def test_errors_are_reported(gpu):
    with gpu.Simulation(100, soft=SOFT) as sim:
        with pytest.raises(gpu.MurbHipError):
            sim.step(DT)                      # no upload yet
        with pytest.raises(gpu.MurbHipError):
            sim.set_option("no-such-option", 1)
    with pytest.raises(gpu.MurbHipError):
        gpu.Simulation(0)
    with pytest.raises(gpu.MurbHipError):
        gpu.Simulation(100, device=99)


# ---- BASELINE.json sizes: size-independent properties -------------------------------------------
@pytest.mark.parametrize("n,scheme", [(30000, "galaxy"), (200000, "galaxy"), (200000, "random"), (1000000, "galaxy"),
                                      (2000003, "galaxy")])
def test_full_size_properties(gpu, O, n, scheme):
    """BASELINE.json's sizes (and one beyond them, odd: 47 GB of partial-sum planes) through properties that do
    not need an O(N^2) oracle run."""
    s = O.init_bodies(n, scheme)
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        sim.compute_acc()
        sim.sync()
        a = sim.acc()
    # Newton's third law: sum_i m_i a_i = 0 up to rounding (SURVEY.md §8c known-answer facts)
    m = s["m"].astype(np.float64)
    tot = np.array([(m * c.astype(np.float64)).sum() for c in a])
    scale = np.array([(m * np.abs(c.astype(np.float64))).sum() for c in a])
    assert (np.abs(tot) / scale).max() <= 1e-6
    # the heavy body dominates: a_i ~ -G M0 q_i / (|q_i|^2 + soft^2)^(3/2) to ~1 (galaxy has comparable halo mass)
    # spot check against the fp64 truth on a fixed 2048-body subset (O(2048 N) on the host)
    idx = np.random.default_rng(7).choice(n, 2048, replace=False)
    truth = O.accel_f64_subset(s, idx, SOFT)
    sub = tuple(c[idx] for c in a)
    assert O.rel_err(sub, truth).max() <= TOL_F64_MAX


def test_benchmark_config_against_reference_summary(gpu, O):
    """N = 30000 galaxy (README.md:54-70): positions after 1 and 5 iterations vs the reference's
    cpu+optim run, held as samples + checksums in tests/golden/ref_galaxy_30000_summary.npz."""
    g = np.load(os.path.join(GOLDEN, "ref_galaxy_30000_summary.npz"))
    n = 30000
    s = O.init_bodies(n, "galaxy")
    sub, edge = g["sub"], g["edge"]
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.upload(s)
        sim.step(DT); sim.sync()
        a = sim.acc()
        ref_sub = [g["optim_acc1_sub_a" + c] for c in "xyz"]
        e = O.rel_err([c[sub] for c in a], ref_sub)
        assert e.max() <= TOL_OPTIM["galaxy"][0] and np.sqrt((e ** 2).mean()) <= TOL_OPTIM["galaxy"][1]
        e64 = O.rel_err([c[sub] for c in a], [g["f64_acc1_sub_a" + c] for c in "xyz"])
        assert e64.max() <= TOL_F64_MAX
        st = sim.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(st[k][sub], g["optim_step1_sub_" + k], rtol=TOL_POS, atol=1.0)
            np.testing.assert_allclose(st[k][edge], g["optim_step1_edge_" + k], rtol=TOL_POS, atol=1.0)
        sim.steps(DT, 4); sim.sync()
        st = sim.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(st[k][sub], g["optim_step5_sub_" + k], rtol=5 * TOL_POS, atol=5.0)
            # checksum of the whole array: sum of positions agrees to the same relative level
            assert abs(st[k].astype(np.float64).sum() - g["optim_step5_sum_" + k][0]) <= \
                5 * TOL_POS * np.abs(st[k].astype(np.float64)).sum()


# ---- the mirrored C++ plugin classes (host/), driven like the reference's Catch2 tests ----------------
@pytest.mark.parametrize("n,iters,scheme,eps", [(2048, 1, "random", 1e-3), (2049, 3, "random", 1e-3),
                                                (2048, 4, "galaxy", 1e-1), (2049, 3, "galaxy", 1e-1)])
def test_plugin_classes_like_reference_test(gpu, O, n, iters, scheme, eps):
    """test_SimulationNBody.cpp:28-82 with SimulationNBodyHIP behind HIPBodiesAllocator as the target:
    positions after every iteration vs cpu+naive WithinRel(eps), exact before the first."""
    g = np.load(os.path.join(GOLDEN, f"ref_{scheme}_{n}.npz"))
    ref = O.init_bodies(n, scheme)
    with gpu.HostSim(n, scheme, SOFT, DT) as sim:
        assert sim.flops_per_ite() == float(g["flops_per_ite"][0])
        assert sim.allocated_bytes() == float(g["allocated_bytes"][0])
        st = sim.state()
        for k in ("qx", "qy", "qz", "vx", "vy", "vz", "m", "r"):
            assert np.array_equal(bits(st[k]), bits(g["init_" + k][:n])), k
        for it in range(iters):
            sim.step(1)
            O.simulate(ref, 1, "cpu+naive", SOFT, DT)
            st = sim.state()            # lazy device->host copy, like CUDABodies::getDataSoA()
            for k in ("qx", "qy", "qz"):
                np.testing.assert_allclose(st[k], ref[k], rtol=eps)
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(st[k], g["optim_final_" + k], rtol=TOL_POS, atol=1.0)
        a = sim.acc()
        assert all(np.isfinite(c).all() for c in a)


@pytest.mark.parametrize("scheme", ["random", "galaxy"])
def test_hipbodies_integrator_like_reference_test(gpu, scheme):
    """test_CUDABodies.cpp:42-75: HIPBodies::updatePositionsAndVelocities(accSoA) == Bodies::…, here bit exact."""
    n = 4000
    g = np.load(os.path.join(GOLDEN, f"ref_integrator_{scheme}_{n}.npz"))
    acc = (np.arange(1, n + 1, dtype=np.float32), np.full(n, 3.0, np.float32), (n - np.arange(n)).astype(np.float32))
    dev = gpu.host_integrate(n, scheme, acc, np.float32(0.01), 4, on_device=True)
    host = gpu.host_integrate(n, scheme, acc, np.float32(0.01), 4, on_device=False)
    for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
        assert np.array_equal(bits(dev[k]), bits(host[k])), k
        assert np.array_equal(bits(dev[k]), bits(g["steps4_" + k])), k


def test_plugin_sharded_two_shards(gpu, O):
    n = 2049
    with gpu.HostSim(n, "galaxy", SOFT, DT) as one, gpu.HostSim(n, "galaxy", SOFT, DT, devices=(0, 0), exchange="copy") as two:
        one.step(3)
        two.step(3)
        s1, s2 = one.state(), two.state()
        for k in ("qx", "qy", "qz"):
            np.testing.assert_allclose(s2[k], s1[k], rtol=TOL_POS, atol=1.0)


def test_murb_hip_cli_output(gpu):
    """Same banner and final line as the reference driver (main.cpp:323-334, :393-398)."""
    import re
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    r = subprocess.run([exe, "-n", "30000", "-i", "20", "--nv", "--im", "hip+tile", "--gf"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "  -> implementation    (--im  ): hip+tile" in out and "  -> nb. of bodies     (-n    ): 30000" in out
    assert "  -> precision                 : fp32" in out and "Simulation started..." in out
    m = re.search(r"Entire simulation took ([0-9.e+]+) ms \(([0-9.e+]+) FPS, +([0-9.]+) Gflop/s\)", out)
    assert m, out
    ms, fps, gf = float(m.group(1)), float(m.group(2)), float(m.group(3))
    assert abs(fps - 20 * 1000.0 / ms) / fps < 1e-2
    assert abs(gf - 20.0 * 30000.0 ** 2 * fps / 1024 ** 3) / gf < 2e-2       # Perf.cpp:28 definition


def test_plugin_falls_back_to_peer_copies_without_rccl(gpu):
    """SimulationNBodyHIP over several devices asks for the RCCL exchange; where librccl cannot be loaded (here:
    MURBHIP_RCCL_LIBRARY=none) murbhip_create_sharded answers MURBHIP_E_NO_RCCL and HIPBodies::bindDevice must say so once
    and carry on with the in-process peer-copy exchange instead of exiting."""
    import subprocess
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r); import murbhip, numpy as np, ctypes as C\n"
            "h = C.c_void_p(); arr = (C.c_int * 2)(0, 0)\n"
            "assert murbhip.lib().murbhip_create_sharded(C.byref(h), 4096, 2e8, 6.67384e-11, 2, arr, 1) == -2003\n"   # MURBHIP_E_NO_RCCL
            "with murbhip.HostSim(9000, 'galaxy', devices=(0, 0), exchange='rccl') as two, murbhip.HostSim(9000, 'galaxy') as one:\n"
            "    two.step(3); one.step(3)\n"
            "    a, b = two.state(), one.state()\n"
            "    scale = max(np.abs(b[k]).max() for k in ('qx', 'qy', 'qz'))\n"
            "    assert all(np.abs(a[k] - b[k]).max() <= 2e-6 * scale for k in ('qx', 'qy', 'qz'))\n"
            "print('ok')\n") % os.path.join(ROOT, "nbody-eurohpc_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MURBHIP_RCCL_LIBRARY="none"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr[-1500:])
    assert "librccl could not be loaded" in r.stderr


def test_bench_contract(gpu):
    """bench.py prints exactly ONE JSON line on stdout with the contract's keys (small run)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--bodies", "30000", "--steps", "20", "--warmup", "2",
                        "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["metric"] == "body-interactions/s" and d["n_gpus"] == 1 and d["steps"] == 20 and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 30000.0 ** 2 * 20 / (d["ms_per_step"] * 20e-3)) / d["value"] < 1e-6
    roof = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["unit"] == "TFLOP/s" and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    assert 0.05 < roof["frac"] < 1.0 and d["value"] > 1e12
    # a truthful label: the kernel is bound by fp32 VECTOR issue (no MFMA instruction in it); which flops `frac` counts is in the key
    assert roof["bound"] == "valu" and "MFMA" in roof["bound_detail"] and "ALGORITHMIC" in roof["frac_from"]
    assert abs(roof["interactions_per_launch"] - 30000.0 ** 2) < 1 and roof["launches"] == 20
    assert d["parity"]["max_rel"] <= d["parity"]["tolerance_max_rel"]
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("reference", "port") and cb["value"] > 0 and d["gpu_over_cpu"] > 1
    assert cb["cpu"]["model"] and cb["cpu"]["logical_cpus"] >= cb["cores"] >= 1
    # the host's share as read at process start (affinity mask, physical cores, cgroup quota), and the baseline runs on all of it
    assert cb["cores"] == cb["cpu"]["cpus_usable"] and cb["cpu"]["cpus_in_affinity_mask"] >= cb["cores"]
    assert cb["best_cpu_value"] >= cb["value"] and d["gpu_over_best_cpu"] <= d["gpu_over_cpu"]
    if cb["kind"] == "reference":
        impls = [o["impl"] for o in cb["others"]]
        assert any("AVX2" in i for i in impls) and "cpu+simd" in impls
    # BASELINE.json's other single-GPU sizes ride along in the same line (here: N = 1 000 000, the main run being 30 000)
    oc = {e["n_bodies"]: e for e in d["other_configs"]}
    assert set(oc) == {1000000}
    e = oc[1000000]
    assert abs(e["value"] - 1e12 * e["steps"] / (e["ms_per_step"] * e["steps"] * 1e-3)) / e["value"] < 1e-6 and e["value"] > 3e12
    assert 0.5 < e["roofline"]["frac"] < 1.0 and e["roofline"]["kernel_ms_avg"] <= e["ms_per_step"] and e["plan"]["kernel_variant"] == 8
    assert e["wall_s_incl_setup"] < 15
    assert e["parity"]["max_rel"] <= e["parity"]["tolerance_max_rel"] and "N=1000000" in e["parity"]["vs"]   # fp64 spot check at that size too
    # the workload string names the size that ran and the BASELINE.json config it is
    assert "N=30000" in d["config"]["workload"] and "configs[1]" in d["config"]["workload"]
    # peak from the device's properties; algorithmic vs executed flops kept apart
    assert abs(roof["peak"] - d["device"]["cu_count"] * 256 * d["device"]["clock_mhz"] * 1e-6) < 1e-6
    assert abs(roof["frac_executed"] - roof["frac"] * roof["executed_flop_per_interaction"] / 20.0) < 1e-9
    # the parity gate at N = 30 000 after 1 and 5 steps, vs cpu+optim and vs fp64, max and rms
    gate = d["parity_gate_n30000"]
    assert gate["pass"] is True and gate["n_bodies"] == 30000 and gate["steps"] == [1, 5]
    for k in (1, 5):
        e = gate[f"after_{k}_steps"]
        assert e["acc_vs_cpu_optim"]["max"] <= 3e-5 and e["acc_vs_cpu_optim"]["rms"] <= 1e-5
        assert e["acc_vs_fp64"]["max"] <= 2e-6 and e["pos_vs_cpu_optim"]["max"] <= 2e-6 and e["pos_vs_fp64"]["max"] <= 2e-6
        assert e["acc_vs_fp64"]["max"] <= e["cpu_optim_acc_vs_fp64"]["max"]   # closer to the truth than the reference's CPU path


def test_bench_plain_run_and_its_outputs(gpu, tmp_path):
    """bench.py without --full: the headline figure only (no extras in the line), exactly --steps timed steps, and
    --dump-outputs writes what the last timed step left: the same state and accelerations as the same number of steps
    run here through the C ABI from the same initial conditions."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--bodies", "30000", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "body-interactions/s" and d["unit"] == "interactions/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 30000.0 ** 2 * 7 / (d["ms_per_step"] * 7e-3)) / d["value"] < 1e-6
    for k in ("roofline", "parity", "parity_gate_n30000", "cpu_baseline", "other_configs", "ms_per_step_sync_each_iteration"):
        assert k not in d, k
    names = ("qx", "qy", "qz", "vx", "vy", "vz", "ax", "ay", "az")
    assert sorted(d["dumped_outputs"]) == sorted(names)
    got = {k: np.load(out / f"{k}.npy") for k in names}
    assert all(a.dtype == np.float32 and a.shape == (30000,) for a in got.values())
    s = gpu.init_bodies(30000, "galaxy")
    with gpu.Simulation(30000, soft=SOFT) as sim:
        sim.upload(s)
        sim.steps(DT, d["prewarm_steps"] + 2 + 7)
        sim.sync()
        want = dict(sim.state(), **dict(zip(("ax", "ay", "az"), sim.acc())))
    for group in (("qx", "qy", "qz"), ("vx", "vy", "vz"), ("ax", "ay", "az")):
        scale = max(float(np.abs(want[k]).max()) for k in group)
        for k in group:
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-6 * scale, err_msg=k)


def test_bench_multi_pass_roofline(gpu):
    """A size evaluated in several passes (forced with a small "sym_pass_mb"): one launch covers N^2 / passes interactions,
    and the roofline must be priced with that, not with N^2 (it would exceed the peak)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--bodies", "60000", "--steps", "10", "--warmup", "2",
                        "--opt", "sym_pass_mb=8", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][0])
    passes = d["config"]["sym_passes"]
    assert passes >= 3 and "other_configs" not in d
    roof = d["roofline"]
    assert abs(roof["launches_per_step"] - passes) < 1e-9 and abs(roof["interactions_per_launch"] - 60000.0 ** 2 / passes) < 1
    assert 0.2 < roof["frac"] < 1.0 and roof["frac"] >= d["frac_fp32_peak_whole_step"]


def test_bench_under_torchrun_one_rank(gpu):
    """The launch line the driver uses for N > 1, with one rank: RCCL communicator from a broadcast unique id,
    reduce-scatter + all-gather every step (force_exchange), and the run's own end-to-end check against a
    plain single-GPU run of the same steps."""
    import json
    import subprocess
    import sys
    from conftest import ROOT, free_port
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--bodies", "30000", "--steps", "20",
           "--warmup", "2", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 1e12 and d["config"]["kernel_variant"] == 8
    chk = d["rank_mode_check"]
    assert chk["positions_identical_on_all_ranks"] and chk["finite"]
    assert chk["max_position_diff_rel"] < 1e-5, chk      # 20 steps from the initial state, two fp32 summation orders
    # the exchange explains itself: both collectives event-timed on the exchange stream, the compute stream's waits for
    # them (the exposed part), the three force launches of the pipeline.  One rank, real RCCL: tens of microseconds each
    ex = d["exchange"]
    assert ex["steps_profiled"] == 20 and abs(ex["launches_per_step"] - 2) < 1e-9   # one rank: two triangle parts, no rectangles
    for k in ("reduce_scatter_ms_avg", "all_gather_ms_avg"):
        assert 0.0 < ex[k] < 0.5, (k, ex)
    for k in ("compute_wait_gather_ms_avg", "compute_wait_reduce_ms_avg", "compute_wait_ms_avg"):
        assert 0.0 <= ex[k] < 0.5, (k, ex)
    assert ex["compute_wait_ms_avg"] <= ex["compute_stream_step_ms_avg"] <= ex["ms_per_step_with_profiling"] * 1.05
    f = ex["force_ms_avg"]
    assert f["triangle_part_1"] > 0 and f["triangle_part_2"] > 0 and f["rectangles"] == 0
    assert "one_sided_plan" not in d                       # needs more than one rank
    roof = d["roofline"]                                   # two launches per step share the step's N^2 interactions
    assert abs(roof["launches_per_step"] - 2) < 1e-9 and abs(roof["interactions_per_launch"] - 30000.0 ** 2 / 2) < 1 and 0.3 < roof["frac"] < 1.0
    assert d["other_configs"][0]["n_bodies"] == 1000000 and d["other_configs"][0]["plan"]["kernel_variant"] == 8


# ---------------------------------------------------------------------------------------------------
# moments, the tracked-metrics plugin and the leapfrog integrator

@pytest.mark.parametrize("scheme,n", [("galaxy", 4000), ("random", 2049)])
def test_moments(gpu, O, scheme, n):
    """murbhip_moments (linear / angular momentum, mass-weighted position, mass) against numpy fp64 on
    the same state, before and after stepping; one GPU and three shards."""
    s = O.init_bodies(n, scheme)
    for devices in ([0], [0, 0, 0]):
        with gpu.Simulation(n, soft=SOFT, devices=devices) as sim:
            sim.upload(s)
            for steps in (0, 3):
                if steps:
                    sim.steps(DT, steps)
                got = sim.moments()
                st = dict(sim.state(), m=s["m"])
                want = O.moments_f64(st)
                m = s["m"].astype(np.float64)
                qn = np.sqrt(sum(st[k].astype(np.float64) ** 2 for k in ("qx", "qy", "qz")))
                vn = np.sqrt(sum(st[k].astype(np.float64) ** 2 for k in ("vx", "vy", "vz")))
                scale = {"P": (m * vn).sum(), "L": (m * qn * vn).sum(), "Mq": (m * qn).sum()}   # sums cancel: scale by the terms
                for k in ("P", "L", "Mq"):
                    assert np.linalg.norm(got[k] - want[k]) <= 1e-12 * scale[k], k
                assert abs(got["M"] - want["M"]) <= 1e-12 * want["M"]


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
@pytest.mark.parametrize("scheme,n", [("galaxy", 2048), ("random", 2049), ("galaxy", 30000)])
def test_leapfrog_vs_restatement(gpu, O, scheme, n, devices):
    """Option "integrator" = 1 (kick-drift-kick) against oracle_leapfrog on the same inputs.  PARITY
    UNPINNED by the reference (its gpu+leapfrog evaluates a_n at x_{n-1}); same tolerances as the default
    integrator's position test: the kicks and the drift are bit-identical formulas, the accelerations
    differ by the force kernels' rounding noise."""
    steps = 5 if n <= 5000 else 2
    s = O.init_bodies(n, scheme)
    ref = {k: v.copy() for k, v in s.items()}
    O.leapfrog(ref, steps, SOFT, DT)
    with gpu.Simulation(n, soft=SOFT, devices=devices) as sim:
        sim.set_option("integrator", 1)
        sim.upload(s)
        sim.steps(DT, steps)
        st = sim.state()
        st2 = sim.state()      # reading out twice must not move the state (closing kick is not stored)
        for k in st:
            assert np.array_equal(bits(st[k]), bits(st2[k])), k
        with pytest.raises(gpu.MurbHipError):
            sim.set_option("integrator", 0)          # half-step velocities on the device
        with pytest.raises(gpu.MurbHipError):
            sim.integrate_host_acc((s["qx"], s["qy"], s["qz"]), DT)
        sim.upload(s)                                 # a fresh upload re-synchronises
        sim.set_option("integrator", 0)
    scale = max(np.abs(ref[k]).max() for k in ("qx", "qy", "qz"))
    for k in ("qx", "qy", "qz"):
        assert np.abs(st[k] - ref[k]).max() <= TOL_POS * scale, k
    vscale = max(np.abs(ref[k]).max() for k in ("vx", "vy", "vz"))
    # random scheme: cpu+optim's accelerations (the restatement's input) are themselves up to 2e-3 off for
    # ~1 % of the bodies (flush-to-zero, see the module docstring), and velocities there are small
    vtol = 2e-5 if scheme == "galaxy" else 2e-4
    for k in ("vx", "vy", "vz"):
        assert np.abs(st[k] - ref[k]).max() <= vtol * vscale, k


def test_leapfrog_conserves_energy(gpu, O):
    """What a kick-drift-kick scheme is for: over 100 one-hour steps of the 30 000-body galaxy the energy
    stays within 2e-5 and the angular momentum within 1e-5, while the reference's update (default) drifts
    by orders of magnitude more on the same inputs."""
    n = 30000
    s = O.init_bodies(n, "galaxy")
    drift = {}
    for integ in (0, 1):
        with gpu.Simulation(n, soft=SOFT) as sim:
            sim.set_option("integrator", integ)
            sim.upload(s)
            e0 = sum(sim.energy())
            L0 = sim.moments()["L"]
            sim.steps(DT, 100)
            e1 = sum(sim.energy())
            L1 = sim.moments()["L"]
        drift[integ] = (abs(e1 - e0) / abs(e0), np.linalg.norm(L1 - L0) / np.linalg.norm(L0))
    assert drift[1][0] < 2e-5 and drift[1][1] < 1e-5, drift
    assert drift[0][0] > 20 * drift[1][0], drift


@pytest.mark.parametrize("leapfrog", [False, True])
def test_tracking_plugin(gpu, O, leapfrog, tmp_path):
    """`--im hip+tracking` / `hip+leapfrog` (SimulationNBodyHIPTracking): row k of the history holds the
    metrics of the state iteration k starts from (reference computeOneIteration(),
    SimulationNBodyCUDAPropertyTracking.cu:121-133), checked against fp64 evaluations along the oracle's
    own trajectory; the CSV has the reference's layout."""
    n, iters = 2048, 4
    with gpu.HostSim(n, "galaxy", SOFT, DT, tracking=True, leapfrog=leapfrog) as sim:
        sim.step(iters)
        hist = sim.history()
        path = tmp_path / "metrics.csv"
        sim.save_history_csv(path)
    assert len(hist["energy"]) == iters
    s = O.init_bodies(n, "galaxy")
    for k in range(iters):
        st = {kk: v.copy() for kk, v in s.items()}
        if k:
            (O.leapfrog(st, k, SOFT, DT) if leapfrog else O.simulate(st, k, "cpu+optim", SOFT, DT))
        e = sum(O.energy_f64(st, SOFT))
        mom = O.moments_f64(st)
        assert abs(hist["energy"][k] - e) <= 1e-5 * abs(e), k
        assert abs(hist["ang_momentum"][k] - np.linalg.norm(mom["L"])) <= 1e-6 * np.linalg.norm(mom["L"]), k
        assert np.abs(hist["density_center"][k] - mom["Mq"] / mom["M"]).max() <= 1e-6 * 2e8, k
    rows = path.read_text().splitlines()
    assert rows[0] == "iteration,energy,ang_momentum,density_center_x,density_center_y,density_center_z"
    assert len(rows) == iters + 1 and float(rows[1].split(",")[1]) == hist["energy"][0]


def test_murb_hip_cli_tracking(gpu, tmp_path):
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    csv = tmp_path / "m.csv"
    r = subprocess.run([exe, "-n", "4000", "-i", "10", "--nv", "--im", "hip+leapfrog", "--csv", str(csv)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "  -> implementation    (--im  ): hip+leapfrog" in r.stdout and "Entire simulation took" in r.stdout
    assert "Energy at the first / last tracked iteration" in r.stdout
    rows = csv.read_text().splitlines()
    assert len(rows) == 11
    e = [float(x.split(",")[1]) for x in rows[1:]]
    assert abs(e[-1] - e[0]) < 1e-5 * abs(e[0])


def test_file_scheme_end_to_end(gpu, O, tmp_path, monkeypatch):
    """`-s <anything else>`: bodies from `milkyway_andromeda.tab` (Bodies.cpp:83-153; bit parity of the reader
    with the reference is in tests/test_oracle_vs_ref.py) through the plugin classes: kpc / km/s / solar-mass
    numbers, a softening of 0.05, 20 000 bodies — the pair-symmetric kernel against the fp64 sum."""
    rng = np.random.default_rng(5)
    n = 20000
    rows = rng.normal(size=(n, 7)).astype(np.float32)
    rows[:, 0] = np.abs(rows[:, 0]) * 1e-5
    with open(tmp_path / "milkyway_andromeda.tab", "w") as f:
        for r in rows:
            f.write(" ".join(f"{x:.9g}" for x in r) + "\n")
    monkeypatch.chdir(tmp_path)
    soft, dt = np.float32(0.05), np.float32(1e-3)
    with gpu.HostSim(n, "collision", soft, dt) as sim:
        assert sim.n == n
        s = sim.state()
        sim.step(1)
        a = sim.acc()
        moved = sim.state()
    truth = O.accel_f64(s, soft)
    assert O.rel_err(a, truth).max() <= TOL_F64_MAX
    ref = {k: v.copy() for k, v in s.items()}
    O.integrate(ref, a, dt)
    for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
        assert np.array_equal(bits(moved[k]), bits(ref[k])), k


@pytest.mark.parametrize("n,devices", [(4000, [0]), (20000, [0]), (20000, [0, 0, 0]), (9000, [0, 0])])
@pytest.mark.parametrize("integrator", [0, 1])
def test_remembered_forces_change_nothing(gpu, O, n, integrator, devices):
    """murbhip_compute_acc() results are remembered (a repeated call, a leapfrog read-out or a directly following
    step reuse them — with several shards too: the step is then the state update and the position exchange only), and
    murbhip_energy() on a pair-symmetric plan takes the potential out of a force evaluation whose forces are bit-identical
    to a plain one's.  Every mix of calls must land on the bits of the plain sequence."""
    s = O.init_bodies(n, "galaxy")
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as plain, gpu.Simulation(n, soft=SOFT, **kw) as mixed:
        for sim in (plain, mixed):
            sim.set_option("integrator", integrator)
            sim.upload(s)
        plain.steps(DT, 2)
        plain.set_option("jsplit", 2)                    # the same plan change, at the same step, in both contexts
        plain.steps(DT, 2)
        a_ref = None
        for k in range(4):
            mixed.compute_acc(); mixed.compute_acc()
            acc = mixed.acc()
            mixed.energy(); mixed.moments(); mixed.state()
            again = mixed.acc()                          # the energy sweep must not disturb the accelerations
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(acc, again))
            if k == 2:
                mixed.set_option("jsplit", 2)            # a plan change in between drops the remembered forces: the step
            mixed.step(DT)                               # evaluates them again under the new plan, which stays in force
        a, b = plain.state(), mixed.state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("scheme,n,devices", [("galaxy", 12001, [0]), ("galaxy", 30000, [0]), ("random", 20000, [0]), ("galaxy", 40000, [0, 0, 0]),
                                              ("galaxy", 30000, [0, 0])])
def test_energy_from_the_force_evaluation(gpu, O, scheme, n, devices):
    """murbhip_energy on a pair-symmetric plan: the potential energy summed inside a FORCE evaluation (one float per group of 4
    i bodies, fp64 from there on) against the fp64 value and against the separate potential sweep of rounds 1-2
    ("energy_sweep" 1) — and no second N^2 launch: the tracked sequence energy -> step runs ONE force launch per iteration."""
    s = O.init_bodies(n, scheme)
    ke, pe = O.energy_f64(s, SOFT)
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as fused, gpu.Simulation(n, soft=SOFT, **kw) as sweep:
        sweep.set_option("energy_sweep", 1)
        for sim in (fused, sweep):
            sim.set_option("variant", 8)
            sim.upload(s)
        (k1, p1), (k2, p2) = fused.energy(), sweep.energy()
        # the fused sum: off-diagonal pairs in fp32 chains of 32, the diagonal blocks in fp64 without self terms: measured 4e-9..3e-8
        assert abs(p1 - pe) <= 1e-7 * abs(pe) and abs(k1 - ke) <= 1e-9 * abs(ke), (p1 - pe) / pe
        assert abs(p2 - pe) <= 5e-7 * abs(pe) and abs(p1 - p2) <= 5e-7 * abs(pe)
        # tracked iterations: energy + moments + step.  ONE N^2 evaluation each where the potential rides on the forces (the
        # step reuses them), two with the separate sweep ("sym_launches" counts pair-symmetric launches of any form)
        per_force, per_sweep = (1, 1) if len(devices) == 1 else (3, 2)     # several shards: two triangle parts + rectangles
        for sim in (fused, sweep):
            sim.step(DT)                                  # new positions: nothing remembered
            sim.set_option("profile", 1)
            for _ in range(3):
                sim.energy(); sim.moments(); sim.step(DT)
        assert fused.info("sym_launches") == 3 * per_force * len(devices), fused.info("sym_launches")
        assert sweep.info("sym_launches") == 3 * (per_force + per_sweep) * len(devices), sweep.info("sym_launches")
        a, b = fused.state(), sweep.state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k          # the forces of a tracked evaluation are the plain ones
        (k1, p1), (k2, p2) = fused.energy(), sweep.energy()
        assert abs(p1 - p2) <= 5e-7 * abs(p2) and abs(k1 - k2) <= 1e-12 * abs(k2)


@pytest.mark.parametrize("n,devices,opts", [(1, [0], {}), (37, [0], {}), (1000, [0], {}), (2048, [0], {}), (2048, [0], {"integrator": 1}),
                                            (5000, [0], {"variant": 1}), (5000, [0], {"variant": 1, "jsplit": 5}), (30000, [0], {"variant": 1}),
                                            (9001, [0, 0], {"variant": 1}), (30000, [0] * 8, {"variant": 1}), (30000, [0] * 4, {"variant": 1, "overlap": 0}),
                                            (20000, [0, 0, 0], {"variant": 1, "integrator": 1})])
def test_state_update_in_the_force_launch_changes_nothing(gpu, O, n, devices, opts):
    """One-sided plan: the state update rides in the tail of the step's last force launch (murb_force_integrate_kernel: the
    workgroup that draws an i group's last ticket adds the group's partial sums and moves its bodies) instead of a launch
    of its own ("fuse_integrate" 0).  Same sums in the same order: bit-identical states and accelerations, step after step,
    one GPU and shards, both integrators, with evaluations and read-outs in between."""
    s = O.init_bodies(n, "galaxy")
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as two, gpu.Simulation(n, soft=SOFT, **kw) as one:
        two.set_option("fuse_integrate", 0)
        for sim in (two, one):
            for k, v in opts.items():
                sim.set_option(k, v)
            sim.upload(s)
        for rounds in range(3):
            for sim in (two, one):
                sim.steps(DT, 7)
                sim.compute_acc()            # an evaluation without a state update takes the same route
            a, b = two.acc(), one.acc()
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
            for sim in (two, one):
                sim.step(DT)                 # from remembered forces: the plain integrate launch in both
            a, b = two.state(), one.state()
            for k in a:
                assert np.array_equal(bits(a[k]), bits(b[k])), (rounds, k)
        assert int(one.info("variant")) == 1 and np.isfinite(a["qx"]).all()


@pytest.mark.parametrize("n,devices", [(3000, [0]), (30000, [0]), (30000, [0, 0, 0])])
def test_warmup_changes_nothing(gpu, O, n, devices):
    """murbhip_warmup: untimed force evaluations before a caller's first timed iteration.  The state is untouched, nothing
    is remembered (the step that follows launches its own force evaluation), the trajectory is bit-identical."""
    s = O.init_bodies(n, "galaxy")
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as plain, gpu.Simulation(n, soft=SOFT, **kw) as warm:
        for sim in (plain, warm):
            sim.upload(s)
        warm.warmup(20.0)
        a, b = plain.state(), warm.state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        warm.set_option("profile", 1)
        plain.set_option("profile", 1)
        for sim in (plain, warm):
            sim.steps(DT, 3)
            sim.sync()
        assert warm.info("force_launches") == plain.info("force_launches") > 0
        warm.warmup(5.0)                                   # between steps as well
        for sim in (plain, warm):
            sim.step(DT)
        a, b = plain.state(), warm.state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        with pytest.raises(gpu.MurbHipError):
            warm.warmup(-1.0)


@pytest.mark.parametrize("n,shards", [(29, 8), (132, 8), (300, 1), (300, 8), (1025, 2), (2500, 3)])
def test_fused_potential_with_few_bodies(gpu, O, n, shards):
    """The galaxy's central body is 10^4 times heavier than the rest: with a few dozen bodies its own term (G m)^2 / soft is
    100 times all pair terms together.  The fused potential never forms it (diagonal blocks: murb_sym_pe_diag_kernel, fp64,
    i != j), so it stays at fp32-rounding-of-one-term accuracy where the sweep (self term in, self term out) loses digits."""
    s = O.init_bodies(n, "galaxy")
    ke, pe = O.energy_f64(s, SOFT)
    kw = {"devices": [0] * shards} if shards > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as sim:
        sim.set_option("variant", 8)
        sim.upload(s)
        k1, p1 = sim.energy()
        assert int(sim.info("variant")) == 8
        assert abs(p1 - pe) <= 1e-7 * abs(pe) and abs(k1 - ke) <= 1e-9 * abs(ke), (p1 - pe) / pe
        sim.step(DT)
        k2, p2 = sim.energy()
        ke2, pe2 = O.energy_f64(dict(sim.state(), m=s["m"]), SOFT)
        assert abs(p2 - pe2) <= 1e-7 * abs(pe2) and abs(k2 - ke2) <= 1e-9 * abs(ke2)


def test_beyond_the_partial_plane_budget(gpu, O):
    """4 000 003 bodies: the pair-symmetric kernel's partial sums (N^2/1024 x 12 B = 187 GB) exceed the per-pass budget
    (a quarter of the GPU's memory).  Round 1 fell back to the one-sided kernel here; now the items are evaluated in
    several passes over ranges of j columns that share one buffer, row sums accumulated in fp64 — checked against the
    fp64 sum on a subset, and through Newton's third law over all bodies."""
    n = 4000003
    s = O.init_bodies(n, "galaxy")
    with gpu.Simulation(n, soft=SOFT) as sim:
        assert int(sim.info("variant")) == 8
        sim.upload(s)
        sim.compute_acc()
        sim.sync()
        assert sim.info("sym_passes") >= 2 and sim.info("device_bytes") < 100e9
        a = sim.acc()
    idx = np.random.default_rng(3).choice(n, 512, replace=False)
    assert O.rel_err(tuple(c[idx] for c in a), O.accel_f64_subset(s, idx, SOFT)).max() <= TOL_F64_MAX
    m = s["m"].astype(np.float64)
    tot = np.array([(m * c.astype(np.float64)).sum() for c in a])
    scale = np.array([(m * np.abs(c.astype(np.float64))).sum() for c in a])
    assert (np.abs(tot) / scale).max() <= 1e-6


@pytest.mark.parametrize("shards,variant,overlap", [(4, 8, 1), (3, 8, 2), (4, 1, 1), (1, 8, 1)])
def test_long_sharded_runs_are_bit_reproducible(gpu, O, shards, variant, overlap):
    """2 000 steps of the multi-stream pipeline (force launches, row sums, peer reduce, integrate and the position
    exchange on two or three streams per shard), twice: all sums are taken in a fixed order, so any difference
    between the two runs would be a missing dependency between streams."""
    n, steps = 12000, 2000
    s = O.init_bodies(n, "galaxy")
    out = []
    for _ in range(2):
        kw = {} if shards == 1 else {"devices": [0] * shards}
        with gpu.Simulation(n, soft=SOFT, **kw) as sim:
            sim.set_option("variant", variant)
            sim.set_option("overlap", overlap)
            sim.upload(s)
            sim.steps(DT, steps)
            out.append(sim.state())
    for k in out[0]:
        assert np.array_equal(bits(out[0][k]), bits(out[1][k])), k
    assert all(np.isfinite(out[0][k]).all() for k in out[0])


# ---------------------------------------------------------------------------------------------------
# initial conditions generated ON THE DEVICE (csrc/murb_init.h)

@pytest.mark.parametrize("scheme,n,seed,devices", [
    ("galaxy", 4096, 0, [0]), ("galaxy", 30000, 0, [0]), ("galaxy", 200000, 0, [0]), ("galaxy", 2049, 7, [0]), ("galaxy", 1, 0, [0]),
    ("galaxy", 1000000, 0, [0]), ("galaxy", 60001, 123456789, [0, 0, 0]), ("random", 2049, 0, [0]), ("random", 30000, 5, [0]),
    ("random", 12001, 1, [0, 0]), ("galaxy", 250, 0, [0]),
])
def test_device_initial_conditions_bit_identical_to_host(gpu, scheme, n, seed, devices):
    """murbhip_init_bodies against the product's host initialisation (host/core/Bodies.cpp, bit-identical to the compiled
    reference: tests/test_abi_and_host.py): every one of the eight arrays bit for bit — glibc's rand() sequence by
    jump-ahead (draws up to 4 million deep), the compiled float/double mix, glibc's sincosf — on one GPU and over shards."""
    want = gpu.init_bodies(n, scheme, seed)
    kw = {"devices": devices} if len(devices) > 1 else {}
    with gpu.Simulation(n, soft=SOFT, **kw) as sim:
        sim.init_bodies(scheme, seed)
        got = sim.state()
        got["m"], got["r"] = sim.masses(with_radii=True)
    for k in ("m", "r", "qx", "qy", "qz", "vx", "vy", "vz"):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert len(bad) == 0, (k, len(bad), bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def test_device_initial_conditions_run_like_uploaded_ones(gpu):
    """A run started from device-made bodies is the run started from the host's: same records (G*m folded in the same
    way), so the same bits after stepping."""
    n = 30000
    with gpu.Simulation(n, soft=SOFT) as a, gpu.Simulation(n, soft=SOFT) as b:
        a.init_bodies("galaxy", 0)
        b.upload(gpu.init_bodies(n, "galaxy", 0))
        for sim in (a, b):
            sim.steps(DT, 3)
            sim.sync()
        sa, sb = a.state(), b.state()
        ea, eb = a.energy(), b.energy()
    for k in ("qx", "qy", "qz", "vx", "vy", "vz"):
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
    assert ea == eb


def test_device_initial_conditions_sse2_libm_variant(gpu, O):
    """The other build of glibc's sincosf (plain SSE2, what a CPU without FMA/AVX2 runs; "init_libm_fma" = 0) against the
    numpy restatement that rounds every operation on its own: bit-identical.  And the two builds differ from each other
    in at most a few last bits per hundred thousand bodies."""
    n = 100000
    want = O.init_galaxy_spelled_out(n, 0)
    with gpu.Simulation(n, soft=SOFT) as sim:
        sim.set_option("init_libm_fma", 0)
        sim.init_bodies("galaxy", 0)
        got = sim.state()
        got["m"], got["r"] = sim.masses(with_radii=True)
        sim.set_option("init_libm_fma", 1)
        sim.init_bodies("galaxy", 0)
        fma = sim.state()
    for k in ("m", "r", "qx", "qy", "qz", "vx", "vy", "vz"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    differ = sum(int((fma[k].view(np.uint32) != got[k].view(np.uint32)).sum()) for k in ("qx", "qy", "qz"))
    assert differ <= 30, differ


def test_device_initial_conditions_errors(gpu):
    with gpu.Simulation(1000, soft=SOFT) as sim:
        with pytest.raises(gpu.MurbHipError):
            sim.init_bodies("spiral", 0)
        with pytest.raises(gpu.MurbHipError):
            sim.masses()                      # nothing uploaded or initialised yet
        sim.upload(gpu.init_bodies(1000, "galaxy"))
        with pytest.raises(gpu.MurbHipError):
            sim.masses(with_radii=True)       # the host never sent radii
        assert np.array_equal(sim.masses(), gpu.init_bodies(1000, "galaxy")["m"])


@pytest.mark.parametrize("scheme,n,devices", [("galaxy", 6151, (0,)), ("random", 4100, (0, 0))])
def test_plugin_bodies_initialised_on_the_device(gpu, scheme, n, devices):
    """HIPBodies::initOnDevice through the mirrored plugin classes: getDataSoA() after it returns the bodies the constructor
    made on the host, bit for bit (masses and radii included), and the run goes on from there."""
    with gpu.HostSim(n, scheme, devices=devices, exchange="copy") as sim:
        before = sim.state()
        sim.init_on_device(0)
        after = sim.state()
        for k in gpu.FIELDS:
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        sim.step(2)
        moved = sim.state()
    with gpu.HostSim(n, scheme, devices=devices, exchange="copy") as ref:
        ref.step(2)
        want = ref.state()
    for k in gpu.FIELDS:
        assert np.array_equal(moved[k].view(np.uint32), want[k].view(np.uint32)), k


def test_murb_hip_cli_device_init(gpu):
    """`murb-hip --dinit`: the same run from bodies generated on the device (the banner and the final line are unchanged)."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    r = subprocess.run([exe, "-n", "20000", "-i", "5", "--nv", "--im", "hip+tracking", "--dinit"], capture_output=True, text=True, timeout=300)
    r0 = subprocess.run([exe, "-n", "20000", "-i", "5", "--nv", "--im", "hip+tracking"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r0.returncode == 0, (r.stderr, r0.stderr)
    energy = [l for l in r.stdout.splitlines() if l.startswith("Energy at the first")]
    assert energy and energy == [l for l in r0.stdout.splitlines() if l.startswith("Energy at the first")]
    assert "Entire simulation took" in r.stdout

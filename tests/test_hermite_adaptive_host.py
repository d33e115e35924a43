"""CPU: murbhip_evolve / murbhip_evolve_dts exist in the library, the binding and the header; the numpy restatement of the
step rule (tests/helpers/hermite_adaptive_ref.py) does on an eccentric binary and on the galaxy what a shared adaptive step
is for; the control-block kernels of a fresh gfx950 build use no scratch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import code_object as CO           # noqa: E402
import hermite_adaptive_ref as A   # noqa: E402

SOFT_BINARY = 1e6


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


def test_evolve_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_evolve", "murbhip_evolve_dts"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    assert callable(mh.Simulation.evolve) and callable(mh.Simulation.evolve_dts)
    # the only argument check that needs no device: no context.  (Every other one sits behind a context, which cannot
    # be created without an MI355X; tests/test_hermite_adaptive_gpu.py walks through them.)
    import ctypes as C
    out = (C.c_double * 5)()
    count = C.c_ulong()
    assert mh.lib().murbhip_evolve(None, 1.0, 0.02, 0.01, 0.0, 1.0, 1, out) == -2000
    assert mh.lib().murbhip_evolve_dts(None, None, 0, C.byref(count)) == -2000


def test_host_mirror_knows_the_adaptive_integrator(mh):
    H = mh.host_lib()
    assert hasattr(H, "murbhost_sim_substeps")
    assert callable(mh.HostSim.substeps)


# e, eta -> steps, smallest dt, largest dt, adaptive relative energy error, fixed-step error at the same step count
BINARY_TABLE = {
    (0.9, 0.02): (850, 628.0, 7.2e5, 1.35e-4, 7.1),
    (0.9, 0.01): (1203, 423.0, 5.1e5, 3.3e-5, 5.2),
    (0.95, 0.02): (1016, 102.0, 7.5e5, 2.6e-4, 24.0),
}


@pytest.mark.parametrize("e,eta", sorted(BINARY_TABLE))
def test_restatement_reproduces_the_binary_table(e, eta):
    """Equal-mass binary, m = 1e30 kg, a = 1e11 m, softening 1e6 m, 5 periods from pericentre, state, a and j rounded to
    fp32 at every store: every figure within a factor of 2 of the table the feature was specified with.  (The smallest dt of
    the first row is the starting step eta_start |a0| / |j0| at pericentre; those of the other two are the final step that
    ends the run at `duration` exactly.)  Measured: 850 / 1203 / 1016 steps, dt 628 ... 7.17e5, 423 ... 5.07e5,
    102 ... 7.45e5 s, errors 1.35e-4 / 3.3e-5 / 2.6e-4, fixed step 7.1 / 5.2 / 24."""
    s, period = A.binary(e)
    duration = 5.0 * period
    e0 = A.energy(s, SOFT_BINARY)
    out, dts, t, _ = A.evolve(s, duration, SOFT_BINARY, eta=eta)
    err = abs(A.energy(out, SOFT_BINARY) - e0) / abs(e0)
    fixed, fdts, _, _ = A.evolve(s, duration, SOFT_BINARY, fixed_dt=duration / len(dts))
    ferr = abs(A.energy(fixed, SOFT_BINARY) - e0) / abs(e0)
    got = (len(dts), float(min(dts)), float(max(dts)), err, ferr)
    print(f"e = {e}, eta = {eta}: {got[0]} steps, dt {got[1]:.4g} ... {got[2]:.4g} s, relative energy error {err:.3e}; "
          f"{len(fdts)} fixed steps: {ferr:.3e}")
    assert t == duration
    assert abs(float(np.sum(np.asarray(dts, np.float64))) - duration) <= 0.5 * np.spacing(np.float32(dts[-1]))
    assert abs(len(fdts) - len(dts)) <= 1
    for name, g, want in zip(("steps", "smallest dt", "largest dt", "adaptive error", "fixed-step error"), got, BINARY_TABLE[(e, eta)]):
        assert want / 2.0 <= g <= want * 2.0, (name, g, want)
    if (e, eta) == (0.9, 0.02):
        assert err < 1e-3 and ferr > 1.0


def test_restatement_settles_on_the_galaxy(mh):
    """2048-body galaxy, eta = 0.02: the starting rule gives ~2500 s, the criterion ~2.5e4 s from the third step on
    (measured 2500, 22 660, 25 230, 25 390 s) — the fp32 differences a0 - a1 do not make it wander."""
    s = mh.init_bodies(2048, "galaxy")
    _, dts, _, _ = A.evolve(s, 3.6e5, 2e8, eta=0.02, max_steps=4)
    print("dt sequence:", ", ".join(f"{float(d):.0f}" for d in dts))
    assert len(dts) == 4
    assert 1250.0 <= dts[0] <= 5000.0
    assert all(2e4 <= d <= 3e4 for d in dts[2:])


def test_step_rule_edges():
    """A lone body and a body without jerk propose +inf (the clamp then takes dt_max); the last step ends at `duration`."""
    z = np.zeros((3, 1))
    assert np.isinf(A.candidate(z, z, z, z, 100.0, 0.02))
    assert np.isinf(A.first_candidate(np.ones((3, 1)), z, 0.01))
    assert A.clamp(np.float32(np.inf), 0.0, 50.0) == np.float32(50.0)
    assert A.clamp(np.float32(1.0), 10.0, 50.0) == np.float32(10.0)
    assert A.choose(np.float32(40.0), 70.0, 100.0, 0.0, 50.0) == (np.float32(30.0), True)
    assert A.choose(np.float32(20.0), 70.0, 100.0, 0.0, 50.0) == (np.float32(20.0), False)


def test_adaptive_kernels_use_no_scratch():
    """Code-object metadata of a fresh gfx950 build: the six control-block kernels are there, with 0 bytes of scratch and 0
    spilled registers; the adaptive sweep has the fixed-step sweep's LDS and arithmetic."""
    hipcc = CO.hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed: no code object to inspect")
    kernels = CO.metadata(r"murb_evolve_|_adaptive_kernel")
    for want in ("murb_evolve_begin_kernel", "murb_evolve_first_kernel", "murb_evolve_start_kernel", "murb_evolve_book_kernel",
                 "murb_hermite_predict_adaptive_kernel", "murb_force_jerk_adaptive_kernel", "murb_hermite_correct_adaptive_kernel"):
        assert any(want in k for k in kernels), want + " missing from the code object"
    for name, num in kernels.items():
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0, name

    def packed(kernel):   # the packed fp32 instructions and reciprocal square roots of a kernel's body
        return sorted(CO.ops(kernel, r"^\s*(v_pk_\w+|v_rsq_f32\w*|ds_read_b128)\b"))

    fixed, adaptive = "murb_force_jerk_kernel", "murb_force_jerk_adaptive_kernel"
    assert packed(fixed) == packed(adaptive) and len(packed(fixed)) > 100

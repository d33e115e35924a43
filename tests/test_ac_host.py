"""CPU: the Ahmad-Cohen scheme's entry points against include/murbac.h, the binding's checks, tests/helpers/ac_ref.py pinned against
hermite_ref and against itself (n_irr = 1, h = 0, a radius that takes in every body, the derivative update on a cubic, wrong
readings of the definition on the GPU tests' inputs, order and placement of the energy error), the pure header under g++ alone and
under the address and undefined-behaviour sanitizers, and the kernels' code-object metadata."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ac_ref as A            # noqa: E402
import code_object as CO      # noqa: E402
import hermite_ref as H       # noqa: E402

E_INVALID = -2000
CSRC = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc")
DT = np.float32(2.0 ** -13)   # tests/test_ac_gpu.py's


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


# -------------------------------------------------------------------------------------------------------------- entry points
def test_ac_entry_points_are_exported(mh):
    """include/murbac.h, the binding's list and the library's exports name the same six calls, disjoint from the other interfaces'
    lists; the version is unchanged; a NULL context is refused without a device; the header carries the definition and what is not
    covered."""
    header = open(os.path.join(ROOT, "include", "murbac.h")).read()
    declared = sorted(re.findall(r"^int (murbac_\w+)\(", header, re.M))
    assert declared == sorted(mh.AC_EXPORTS) and len(declared) == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbac_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS) | \
        set(mh.NBR_EXPORTS) | set(mh.BIND_EXPORTS) | set(mh.BOUND_EXPORTS) | set(mh.MST_EXPORTS) | set(mh.SEP_EXPORTS) | set(mh.LIST_EXPORTS)
    assert not set(mh.AC_EXPORTS) & others
    L = mh.lib()
    assert L.murbhip_version() == 103
    assert L.murbac_begin(None, None, 0.1, 4) == E_INVALID
    assert L.murbac_steps(None, 1.0, 1) == E_INVALID and L.murbac_steps(None, 1.0, 0) == E_INVALID
    assert L.murbac_end(None) == E_INVALID and L.murbac_state(None, None) == E_INVALID
    assert L.murbac_lists(None, None, None, 0) == E_INVALID and L.murbac_forces(None, None, None, None, None) == E_INVALID
    for text in ("tau = (double)(m + 1) * (double)dt", "T = (double)n_irr * (double)dt", "x2 = (-6 (A0 - A1) - T (4 J0 + 2 J1)) / (T T)",
                 "x3 = (12 (A0 - A1) + 6 T (J0 + J1)) / (T T T)", "a2R <- (float)(x2 + T x3)", "OLD lists", "PREDICTED sources",
                 "bit for bit murbhip_steps'", "aR == a0 bit for bit", "[1, 4096]", "MURBHIP_E_STATE", "ends it silently",
                 "2^31 - 1", "stays an observer", "Not covered", "block steps for the irregular force", "gained and lost neighbours",
                 "adaptive dt, n_irr or radii", "inside the", "several shards or ranks", "fp64 sums", "balancing long lists"):
        assert text in header, text
    assert mh.AC_NIRR_MAX == 4096 and "#define MURB_AC_NIRR_MAX 4096" in open(os.path.join(CSRC, "murb_ac.h")).read()
    make = open(os.path.join(ROOT, "nbody-eurohpc_amd", "Makefile")).read()
    assert make.count("../include/murbac.h") == 2


def test_binding_checks(mh):
    """The binding's methods exist; a radius array of the wrong length is refused before the library is called; the library's
    answer to a NULL context comes back as MurbHipError, never a crash."""
    for method in ("ac_begin", "ac_steps", "ac_end", "ac_state", "ac_lists", "ac_forces", "ac_radii"):
        assert callable(getattr(mh.Simulation, method))
    assert mh.AC_STATE_KEYS == ("n_irr", "m", "steps", "regular_steps", "entries", "longest", "empty", "mean", "time")
    sim = object.__new__(mh.Simulation)
    sim.n, sim._h, sim.soft = 8, None, 0.01
    for bad in (lambda: sim.ac_begin(np.zeros(7, np.float32), 4), lambda: sim.ac_begin(np.zeros((8, 2), np.float32), 4),
                lambda: sim.ac_radii(0), lambda: sim.ac_radii(8)):
        with pytest.raises(ValueError):
            bad()
    for call in (lambda: sim.ac_begin(0.1, 4), lambda: sim.ac_begin(np.zeros(8, np.float32), 4), lambda: sim.ac_steps(1.0, 1), sim.ac_end,
                 sim.ac_state, sim.ac_lists, sim.ac_forces):
        with pytest.raises(mh.MurbHipError) as e:
            call()
        assert e.value.code == E_INVALID


# ---------------------------------------------------------------------------------------------------- the restatement, pinned
def test_nirr_1_is_the_hermite_restatement():
    """ac_ref with n_irr = 1 equals hermite_ref.hermite_f64(state32=True) bit for bit, for h = 0, the cycling radii and a radius
    that takes in every body."""
    n = 300
    s = A.system(n)
    want = H.hermite_f64(s, 4, A.SOFT, DT, state32=True)
    for h in (0.0, A.radii(n), 2.0):
        got = A.run(s, h, 1, 4, A.SOFT, DT).state()
        for k in A.Q + A.V:
            assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def test_radius_zero_and_radius_of_everything():
    """h = 0: every list is empty, aI == +0 and aR == a0 bit for bit through regular and irregular steps.  A radius that takes in
    every body: the regular force is what rounding leaves, |aR| <= 2^-23 |a0| per component (a0 and aI are the roundings of two
    fp64 sums of the same terms in different orders), before and after steps."""
    n = 300
    s = A.system(n)
    zero = A.Scheme(s, 0.0, 3, A.SOFT)
    for _ in range(7):
        assert len(zero.lists[1]) == 0 and not zero.aI.view(np.uint32).any() and not zero.jI.view(np.uint32).any()
        if zero.m == 0:
            assert np.array_equal(zero.aR.view(np.uint32), zero.a0.view(np.uint32))
        zero.step(DT)
    full = A.Scheme(s, 2.0, 3, A.SOFT)
    for _ in range(4):
        assert len(full.lists[1]) == n * (n - 1)
        if full.m == 0:
            assert np.all(np.abs(full.aR) <= 2.0 ** -23 * np.abs(full.a0)) and np.all(np.abs(full.jR) <= 2.0 ** -23 * np.abs(full.j0))
        full.step(DT)


def test_derivative_update_on_a_cubic():
    """A(t) = c0 + c1 t + c2 t^2 / 2 + c3 t^3 / 6: from (A, A') at 0 and T the update returns A''(T) = c2 + c3 T and A''' = c3 to fp64
    rounding (1e-12 of the largest term: the differences cancel two digits), and the polynomial started from the END reproduces A
    at a later time to fp32 rounding."""
    rng = np.random.default_rng(5)
    c = rng.uniform(-2.0, 2.0, (4, 1000))
    for T in (0.25, 1.0, 3.0):
        A1 = c[0] + c[1] * T + c[2] * T * T / 2 + c[3] * T ** 3 / 6
        J1 = c[1] + c[2] * T + c[3] * T * T / 2
        a2, a3 = A.derivatives(c[0], c[1], A1, J1, T, exact=True)
        scale = np.abs(c).max() * max(1.0, T ** 3) / min(1.0, T ** 3)
        assert np.abs(a2 - (c[2] + c[3] * T)).max() <= 1e-12 * scale and np.abs(a3 - c[3]).max() <= 1e-12 * scale
        x2, _ = A.derivatives(c[0], c[1], A1, J1, T, keep_x2=True, exact=True)
        assert np.abs(x2 - c[2]).max() <= 1e-12 * scale
        tau = 0.5 * T
        at, jt = A.poly(A.f32(A1), A.f32(J1), A.f32(a2), A.f32(a3), tau)
        t = T + tau
        want = c[0] + c[1] * t + c[2] * t * t / 2 + c[3] * t ** 3 / 6
        terms = np.abs(A1) + np.abs(J1) * tau + np.abs(a2) * tau ** 2 / 2 + np.abs(a3) * tau ** 3 / 6
        assert at.dtype == np.float32 and np.all(np.abs(at - want) <= 2.0 ** -22 * terms)
        assert np.all(np.abs(jt - (c[1] + c[2] * t + c[3] * t * t / 2)) <= 2.0 ** -22 * (np.abs(J1) + np.abs(a2) * tau + np.abs(a3) * tau ** 2 / 2))


# ------------------------------------------------------------------------------------------------------------- wrong readings
@pytest.fixture(scope="module")
def gpu_case():
    """The GPU value test's own inputs at n = 1025: (state, radii, fp64-sum run, the bound on |dq| and |dv|)."""
    n = 1025
    s, h = A.system(n), A.radii(n)
    r64 = A.run(s, h, 4, 16, A.SOFT, DT).state()
    r32 = A.run(s, h, 4, 16, A.SOFT, DT, sums="f32").state()
    return s, h, r64, [4.0 * d for d in A.distance(r32, r64)]


@pytest.mark.parametrize("wrong", A.WRONG)
def test_wrong_readings_are_told_apart(gpu_case, wrong):
    """Each wrong reading of the definition moves positions and velocities of the GPU test's run (n_irr = 4, 16 steps) by more
    than 100 of the bounds that test applies."""
    s, h, r64, bound = gpu_case
    moved = A.distance(A.run(s, h, 4, 16, A.SOFT, DT, wrong=wrong).state(), r64)
    print(wrong, "moves |dq|, |dv| by", moved, "bounds", bound)
    assert bound[0] > 0 and bound[1] > 0
    assert moved[0] > 100 * bound[0] and moved[1] > 100 * bound[1]


# -------------------------------------------------------------------------------------------------------------------- physics
def galaxy_case(O):
    """Galaxy, n = 256, soft as in the Hermite host tests, n_irr = 4, 16 steps of dt = 16 h: per body the distance to its k-th
    nearest neighbour (times 1.0001) for k = 16 (the radius first tried) and k = 200."""
    s = O.init_bodies(256, "galaxy")
    q = H._stack(s, A.Q)
    d = np.sqrt(((q[:, None, :] - q[:, :, None]) ** 2).sum(0))
    d.sort(1)
    return s, np.float32(2e8), 57600.0, 16, {k: (d[:, k] * 1.0001).astype(np.float32) for k in (16, 200)}


def test_energy_error_order_and_placement(O):
    """ac_ref alone.  Order: halving dt over the same span divides the energy error by a factor that is at least half of what
    hermite_ref shows on the same problem and pair of step sizes.  Placement: the error at (dt, n_irr = 4) lies below plain
    Hermite's at 4 dt.
    Measured, k = 200 of 255 neighbours: AC 6.62e-4 at dt and 1.40e-4 at dt / 2 (factor 4.74); Hermite 3.23e-6 and 4.46e-7 (factor
    7.25); Hermite at 4 dt 2.64e-3.  With the radius first tried (k = 16) the order holds (2.97e-3 and 1.28e-4) and the placement
    does not (2.97e-3 against 2.64e-3): between regular steps the regular force is a cubic extrapolation over up to 3 dt, whose
    error enters the corrector with a far larger coefficient than the corrector's own; the radius was therefore chosen on the CPU
    so that the reference alone satisfies the placement."""
    s, soft, dt, steps, radii = galaxy_case(O)
    e0 = A.energy(s, soft)
    err = lambda st: abs((A.energy(st, soft) - e0) / e0)   # noqa: E731
    herm = [err(H.hermite_f64(s, steps * div, soft, np.float32(dt / div), state32=True)) for div in (1, 2)]
    herm4 = err(H.hermite_f64(s, steps // 4, soft, np.float32(4 * dt), state32=True))
    for k, h in radii.items():
        ac = [err(A.run(s, h, 4, steps * div, soft, np.float32(dt / div)).state()) for div in (1, 2)]
        print(f"k = {k}: AC {ac[0]:.3e} -> {ac[1]:.3e} (factor {ac[0] / ac[1]:.2f}); Hermite {herm[0]:.3e} -> {herm[1]:.3e} "
              f"(factor {herm[0] / herm[1]:.2f}); Hermite at 4 dt {herm4:.3e}")
        assert ac[0] / ac[1] >= 0.5 * herm[0] / herm[1], k
        if k == 200:
            assert ac[0] < herm4


# ----------------------------------------------------------------------------------------- the pure header, stand-alone programs
PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "murb_ac.h"
int main() {
    int ok = 1;
    // 1. the update returns a cubic's second and third derivative at the END, and the polynomial continues the cubic
    const double c0 = 0.75, c1 = -1.25, c2 = 0.5, c3 = 1.5;   // exact in fp32, as are T and what follows from them
    for (double T : {0.25, 0.5, 2.0}) {
        const float A1 = (float)(c0 + c1 * T + c2 * T * T / 2 + c3 * T * T * T / 6), J1 = (float)(c1 + c2 * T + c3 * T * T / 2);
        float a2 = 0.f, a3 = 0.f;
        murb_ac_derivatives((float)c0, (float)c1, A1, J1, T, a2, a3);
        ok &= std::fabs(a2 - (c2 + c3 * T)) <= 1e-5 && std::fabs(a3 - c3) <= 1e-5;
        const double tau = 0.125, t = T + tau;
        ok &= std::fabs(murb_ac_poly_a(A1, J1, a2, a3, tau) - (c0 + c1 * t + c2 * t * t / 2 + c3 * t * t * t / 6)) <= 1e-5;
        ok &= std::fabs(murb_ac_poly_j(J1, a2, a3, tau) - (c1 + c2 * t + c3 * t * t / 2)) <= 1e-5;
    }
    std::printf("%d", ok);
    // 2. tau and T at the largest n_irr: the product of an int and a float is exact in fp64
    const float dt = 0.1f;
    std::printf(" %d", (int)(murb_ac_elapsed(MURB_AC_NIRR_MAX, dt) == 4096.0 * (double)dt && murb_ac_elapsed(4095, dt) == 4095.0 * (double)dt));
    std::printf(" %d", (int)(murb_ac_elapsed(MURB_AC_NIRR_MAX, 3.0e38f) == 4096.0 * (double)3.0e38f));   // no fp32 overflow on the way
    std::printf(" %d %d %d %d", (int)murb_ac_nirr_valid(1), (int)murb_ac_nirr_valid(4096), (int)murb_ac_nirr_valid(0), (int)murb_ac_nirr_valid(4097));
    // 3. a zero polynomial stays +0, a constant stays itself
    std::printf(" %d\n", (int)(murb_ac_poly_a(0.f, 0.f, 0.f, 0.f, 7.0) == 0.f && !std::signbit(murb_ac_poly_a(0.f, 0.f, 0.f, 0.f, 7.0)) &&
                               murb_ac_poly_a(1.5f, 0.f, 0.f, 0.f, 7.0) == 1.5f && murb_ac_poly_j(-2.f, 0.f, 0.f, 7.0) == -2.f));
    return 0;
}
"""
WANT = ["1", "1", "1", "1", "1", "0", "0", "1"]


def build_and_run(tmp_path, flags):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr)
    return done.stdout.split()


def test_ac_header_is_plain_cpp(tmp_path):
    """csrc/murb_ac.h is plain C++: g++ compiles it on the CPU with every warning an error; polynomial and update agree with a cubic."""
    assert build_and_run(tmp_path, []) == WANT


def test_ac_header_program_under_sanitizers(tmp_path):
    """The same stand-alone program, with its own main, built with -fsanitize=address,undefined and run directly: no report, the
    same answers."""
    assert build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == WANT


# --------------------------------------------------------------------------------------------------------------- code object
def test_ac_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one of each of the four kernels, 0 bytes of scratch, no spilled
    register of either kind, at most 128 vector registers, no LDS, no atomic of any kind; the sweep is the list sweep's pair
    arithmetic (15 v_pk_fma_f32 and 2 v_rsq_f32 per packed pair, 7 lane steps in the three loop forms)."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    for kernel in ("murb_ac_predict_kernel", "murb_ac_sweep_kernel", "murb_ac_correct_kernel", "murb_ac_regular_kernel"):
        found = CO.metadata(kernel)
        assert len(found) == 1, kernel + " missing from the code object, or there twice"
        (name, num), = found.items()
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
        assert num["vgpr_count"] <= 128 and num["sgpr_count"] <= 106
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){0,12}?\s+\.name:\s+" + re.escape(name) + r"\n", CO.text()).group(1))
        assert lds == 0
        count = lambda pattern: len(CO.ops(name, pattern))      # noqa: E731
        assert not count(r"atomic") and not count(r"scratch_") and not count(r"^\s+ds_")
        if "sweep" in kernel:
            assert (count(r"^\s+v_pk_fma_f32"), count(r"^\s+v_rsq_f32")) == (15 * 7, 2 * 7)
            assert count(r"^\s+v_add_f32_dpp") == 4 * 7, "seven wave sums"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_ac_" in entry

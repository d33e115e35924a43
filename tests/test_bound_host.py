"""CPU: the bound-member read-out's entry points, its pure header under g++ alone, the host-only Lagrangian radii against
tests/helpers/bound_ref.py and known answers, their refusals, a stand-alone program under the address and undefined-behaviour
sanitizers, the conditions on the fixtures the GPU tests rely on, and the sweep kernel's code-object metadata."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bound_ref as R         # noqa: E402
import code_object as CO      # noqa: E402

E_INVALID = -2000
CSRC = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc")


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


@pytest.fixture(scope="module")
def runs():
    """{name: (state, reference run from all bodies)} of the two fixtures, computed once and left unchanged."""
    return {name: (fx(), R.unbind(fx())) for name, fx in (("A", R.fixture_a), ("B", R.fixture_b))}


# -------------------------------------------------------------------------------------------------------------- entry points
def test_bound_entry_points_are_exported(mh):
    """include/murbbound.h, the binding's list and the library's exports name the same three calls and one aid, disjoint from
    the other interfaces' lists; the version is unchanged; a NULL context is refused without a device."""
    header = open(os.path.join(ROOT, "include", "murbbound.h")).read()
    declared = sorted(re.findall(r"^int (murb(?:pot|bound)_\w+)\(", header, re.M))
    assert declared == sorted(mh.BOUND_EXPORTS) and len(declared) == 4
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murb(?:pot|bound)_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS) | \
        set(mh.NBR_EXPORTS) | set(mh.BIND_EXPORTS)
    assert not set(mh.BOUND_EXPORTS) & others
    assert mh.lib().murbhip_version() == 103
    L = mh.lib()
    assert L.murbpot_of(None, 1, None, None, None) == E_INVALID
    assert L.murbpot_at(None, 0, *([None] * 6)) == E_INVALID
    assert L.murbbound_members(None, None, None, 4, None, None, None) == E_INVALID
    for text in ("span_pot_ms_avg", "span_pot_count", "Not covered", "several shards", "block is open", "command line", "tracking CSV",
                 "re-admission", "Jacobi", "Zero-mass rule", "Field rule", "fma(gm_j * pm, inv, ph)", "v_rsq_f32", "NaN is dropped",
                 "Final pass", "block rows alone", "half a step behind", "radii in the velocity records"):
        assert text in header, text


def test_python_and_host_interfaces(mh):
    for method in ("potential_of", "potential_at", "bound_members"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.bound_members) and callable(mh.lagrangian_radii)
    assert hasattr(mh.host_lib(), "murbhost_sim_bound_members")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint boundMembers\(int maxIter", hpp)
    make = open(os.path.join(ROOT, "nbody-eurohpc_amd", "Makefile")).read()
    assert make.count("../include/murbbound.h") == 2
    assert len(R.OUT16) == len(mh.BOUND_KEYS) == 15 and tuple(mh.BOUND_KEYS) == R.OUT16


PROGRAM = r"""
#include <cstdio>
#include "murb_bound.h"
int main() {
    const double V[3] = {0.5, -0.25, 0.0};
    const double e = murb_bound_energy(1.5f, 0.75f, 2.f, V, 3.f);   // w = (1, 1, 2): 0.5 * 6 - 3
    const double mv[3] = {2.0, 4.0, -6.0};
    double F[3], Z[3];
    murb_bound_frame(4.0, mv, F);
    murb_bound_frame(0.0, mv, Z);
    const float qx[6] = {3.f, 1.f, 2.f, 1.f, 9.f, 0.5f}, qy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m[6] = {1.f, 1.f, 2.f, 1.f, 5.f, 0.f};
    const unsigned char member[6] = {1, 1, 1, 1, 0, 1};
    const double centre[3] = {0.0, 0.0, 0.0}, frac[4] = {0.2, 0.4, 0.8, 1.0};
    double r[4], none[1];
    murb_bound_radii(6, qx, qy, qy, m, member, centre, 4, frac, r);
    const unsigned char out[6] = {0, 0, 0, 0, 0, 1};
    murb_bound_radii(6, qx, qy, qy, m, out, centre, 1, frac, none);   // a massless member alone
    std::printf("%a %d %d %d %a %a %a %a %a %a %a %a %d\n", e, (int)murb_bound_stays(e), (int)murb_bound_stays(-1e-300),
                (int)murb_bound_stays(0.0 / V[2]), F[0], F[1], F[2], Z[0], r[0], r[1], r[2], r[3], (int)(none[0] != none[0]));
    return 0;
}
"""


def build_and_run(tmp_path, flags):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    return done.stdout.split()


def check_program(out):
    values = [float.fromhex(x) for x in out[:1] + out[4:12]]
    assert values[0] == 0.0 and out[1:4] == ["0", "1", "0"], "e = 0 leaves, e < 0 stays, NaN leaves"
    assert values[1:5] == [0.5, 1.0, -1.5, 0.0], "the frame, and 0 for a set without mass"
    # members in order: 0.5 (m 0), 1 (body 1), 1 (body 3), 2 (m 2), 3: running mass 0, 1, 2, 4, 5 of 5
    assert values[5:9] == [1.0, 1.0, 2.0, 3.0] and out[12] == "1"


def test_pure_header_compiles_without_a_device(tmp_path):
    """csrc/murb_bound.h holds the energy, the removal rule, the frame and the radii and is plain C++: g++ compiles it on the CPU
    with every warning an error, and a program built from it gives the known answers."""
    check_program(build_and_run(tmp_path, []))


def test_radii_program_under_sanitizers(tmp_path):
    """The same stand-alone program, with its own main, built with -fsanitize=address,undefined and run directly: no report, the
    same answers."""
    check_program(build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


# ---------------------------------------------------------------------------------------------------------------------- radii
def test_radii_against_the_restatement_bit_for_bit(mh):
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 100, 1664):
        q = rng.standard_normal((3, n)).astype(np.float32)
        q[:, n // 2:] = q[:, :n - n // 2]      # equal distances: the index decides
        m = rng.uniform(0.0, 2.0, n).astype(np.float32)
        member = rng.uniform(size=n) < 0.7
        member[0] = True
        centre = rng.standard_normal(3) * 0.1
        frac = np.concatenate([rng.uniform(1e-3, 1.0, 9), [1.0]])
        for mask in (None, member):
            got, want = mh.lagrangian_radii(q, m, frac, centre, mask), R.radii(q, m, frac, centre, mask)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, got, want)


def test_radii_known_answers(mh):
    """Equal masses on known shells: 10 bodies each at radius 1, 2, 3, 4 about (1, 2, 3): the quarter, half and whole radii are
    1, 2, 4, and a fraction just over a quarter reaches the second shell.  frac = 1 is the outermost member.  A mask removes the
    outer shells.  Members without mass, or no members: NaN."""
    rng = np.random.default_rng(9)
    d = rng.standard_normal((3, 40))
    d /= np.sqrt((d * d).sum(0))
    shell = np.repeat([1.0, 2.0, 3.0, 4.0], 10)
    centre = np.array([1.0, 2.0, 3.0])
    q = (d * shell + centre[:, None]).astype(np.float32)
    m = np.full(40, 0.03125, np.float32)
    got = mh.lagrangian_radii(q, m, [0.25, 0.5, 1.0, 0.2501, 0.75], centre)
    assert np.allclose(got, [1.0, 2.0, 4.0, 2.0, 3.0], rtol=1e-6, atol=0), got
    far = np.sqrt(((q.astype(np.float64) - centre[:, None]) ** 2).sum(0)).max()
    assert abs(got[2] - far) <= 1e-15 * far
    inner = shell <= 2.0
    got = mh.lagrangian_radii(q, m, [0.5, 1.0], centre, inner)
    assert np.allclose(got, [1.0, 2.0], rtol=1e-6, atol=0), got
    assert np.isnan(mh.lagrangian_radii(q, np.zeros(40, np.float32), [0.5, 1.0], centre)).all()
    assert np.isnan(mh.lagrangian_radii(q, m, [0.5], centre, np.zeros(40, bool))).all()
    one = mh.lagrangian_radii([[3.0], [4.0], [0.0]], [2.0], [1e-9, 1.0], [0, 0, 0])
    assert one.tolist() == [5.0, 5.0]
    assert len(mh.lagrangian_radii(q, m, [], centre)) == 0


def test_radii_refuse_bad_arguments(mh):
    fp, dp, bp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    L = mh.lib()
    q = [np.arange(5, dtype=np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32)]      # bodies at distance 0 .. 4
    m, centre, frac, out = np.ones(5, np.float32), np.zeros(3), np.array([0.5, 1.0]), np.full(2, 77.0)

    def call(arrays=None, mass=m, c=centre, fr=frac, nfrac=2, o=out, hole=None):
        a = [x.ctypes.data_as(fp) for x in (arrays or q)] + [mass.ctypes.data_as(fp)]
        if hole is not None:
            a[hole] = None
        return L.murbbound_radii(5, *a, None, c.ctypes.data_as(dp) if c is not None else None, nfrac,
                                 fr.ctypes.data_as(dp) if fr is not None else None, o.ctypes.data_as(dp) if o is not None else None)
    for hole in range(4):
        assert call(hole=hole) == E_INVALID
    assert call(c=None) == E_INVALID and call(fr=None) == E_INVALID and call(o=None) == E_INVALID and call(nfrac=-1) == E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            arrays = [x.copy() for x in q]
            arrays[k][2] = bad
            assert call(arrays=arrays) == E_INVALID
        mm = m.copy()
        mm[4] = bad
        assert call(mass=mm) == E_INVALID
        cc = centre.copy()
        cc[1] = bad
        assert call(c=cc) == E_INVALID
    mm = m.copy()
    mm[1] = -1.0
    assert call(mass=mm) == E_INVALID
    for bad in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert call(fr=np.array([0.5, bad])) == E_INVALID, bad
    assert (out == 77.0).all()
    assert call(nfrac=0) == 0 and (out == 77.0).all()
    assert call() == 0 and out.tolist() == [2.0, 4.0]
    with pytest.raises(ValueError):
        mh.lagrangian_radii(q[:2], m, [0.5], [0, 0, 0])
    with pytest.raises(ValueError):
        mh.lagrangian_radii(q, m, [0.5], [0, 0, 0], member=[1, 0])


# ------------------------------------------------------------------------------------------------------------------- fixtures
def test_fixtures_are_what_the_gpu_tests_need(runs):
    """Fixture A (n = 1664, a ragged fourth tile) converges in at least 3 rounds; the clump and all but a few of the fast bodies
    leave; started from the clump alone all 128 stay in a frame near (3, 0, 0).  Fixture B takes at least 3 rounds, every one
    but the last dropping bodies."""
    s, a = runs["A"]
    print("A:", a["dropped"], "fast bodies kept", int(a["member"][:R.A_FAST].sum()))
    assert len(s["m"]) == 1664 and abs(float(s["m"].astype(np.float64).sum()) - 1.0) < 1e-6
    assert a["converged"] and a["rounds"] >= 3 and a["dropped"][0] >= 150 and a["dropped"][1] >= 1 and a["dropped"][-1] == 0
    assert not a["member"][R.A_SPHERE:].any() and 1 <= a["member"][:R.A_FAST].sum() <= 10
    clump = R.unbind(s, start=R.clump_mask())
    assert clump["members"] == R.A_CLUMP and np.array_equal(clump["member"], R.clump_mask()) and clump["rounds"] == 1
    assert np.abs(clump["v"] - [3.0, 0.0, 0.0]).max() < 0.1
    s, b = runs["B"]
    print("B:", b["dropped"])
    assert len(s["m"]) == 1200 and b["converged"] and b["rounds"] >= 3 and all(d >= 1 for d in b["dropped"][:-1])


def test_wrong_rules_are_caught_on_the_fixtures(runs):
    """Each deliberately wrong rule ends with a different member set on fixture A or B: the self term kept, the frame not
    recomputed, dropped bodies re-admitted, the mask ignored."""
    for rule in ("self", "frame", "readmit", "nomask"):
        differs = {name: int((R.unbind(s, rule=rule)["member"] != right["member"]).sum()) for name, (s, right) in runs.items()}
        print(rule, differs)
        assert max(differs.values()) >= 1, rule


def test_no_body_of_the_reference_sits_in_the_band(runs):
    """The GPU test leaves bodies with |e| <= 2 * TOL_F64_MAX * phi out of a round's set comparison (only the fp32 phi can differ
    from the reference, by at most TOL_F64_MAX * phi) and allows two of them a round.  On the chosen seeds the reference has none
    in any round, so the comparison covers every body."""
    for name, (s, right) in runs.items():
        member = np.ones(len(s["m"]), bool)
        for t in range(right["rounds"]):
            new, e, _, phi = R.one_round(s, member)
            print(f"{name} round {t}: smallest |e| / phi = {(np.abs(e) / phi).min():.3e} (band {R.BAND:.0e})")
            assert R.in_band(e, phi).sum() == 0
            member = new
        assert np.array_equal(member, right["member"])


# --------------------------------------------------------------------------------------------------------------- code object
def test_pot_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one murb_pot_sweep_kernel, 0 bytes of scratch, no spilled register
    of either kind, at most 128 vector registers (4 waves per SIMD).  Per pair of interactions and point 3 packed subtractions,
    4 packed fmas, 1 packed multiply and 2 v_rsq_f32 in its loop (16 point steps unrolled), the four copies of the step behind
    the loop without the multiply; no atomics; the other sweeps are still there."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_pot_sweep_kernel")
    assert len(kernels) == 1, "murb_pot_sweep_kernel missing from the code object, or there twice"
    (name, num), = kernels.items()
    print(name, num)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128
    sub, fma = len(CO.ops(name, r"^\s+v_pk_add_f32 .*neg_lo")), len(CO.ops(name, r"^\s+v_pk_fma_f32"))
    mul, rsq = len(CO.ops(name, r"^\s+v_pk_mul_f32")), len(CO.ops(name, r"^\s+v_rsq_f32"))
    print("packed subtractions", sub, "fmas", fma, "multiplies", mul, "v_rsq_f32", rsq)
    assert (sub, fma, mul, rsq) == (3 * (16 + 4), 4 * (16 + 4), 16, 2 * (16 + 4))
    assert not CO.ops(name, r"atomic")
    for other in ("murb_pot_mask_kernel", "murb_pot_rows_kernel", "murb_bound_energy_kernel", "murb_bound_sums_kernel",
                  "murb_force_field_kernel", "murb_knn_sweep_kernel", "murb_bind_sweep_kernel"):
        assert len(CO.metadata(other)) == 1, other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_pot_sweep" in entry

"""CPU: the pair-separation read-out's entry points, the host-only bin and edge calls against tests/helpers/sep_ref.py, deliberately
wrong binning rules on the tie lattices, the launch cut that keeps every 32-bit counter from wrapping, the pure header under g++
alone and under the address and undefined-behaviour sanitizers, and the sweep kernels' code-object metadata."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import code_object as CO      # noqa: E402
import mst_ref as MR          # noqa: E402
import nearest_ref as NR      # noqa: E402
import sep_ref as R           # noqa: E402

E_INVALID = -2000
CSRC = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc")


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# -------------------------------------------------------------------------------------------------------------- entry points
def test_sep_entry_points_are_exported(mh):
    """include/murbsep.h, the binding's list and the library's exports name the same two calls and two aids, disjoint from the
    other interfaces' lists; the version is unchanged; a NULL context is refused without a device; the header states what the
    issue makes normative."""
    header = open(os.path.join(ROOT, "include", "murbsep.h")).read()
    declared = sorted(re.findall(r"^int (murbsep_\w+)\(", header, re.M))
    assert declared == sorted(mh.SEP_EXPORTS) and len(declared) == 4
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbsep_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS) | \
        set(mh.NBR_EXPORTS) | set(mh.BIND_EXPORTS) | set(mh.BOUND_EXPORTS) | set(mh.MST_EXPORTS)
    assert not set(mh.SEP_EXPORTS) & others
    assert mh.lib().murbhip_version() == 103
    L = mh.lib()
    total = (C.c_double * 1)()
    assert L.murbsep_of(None, 1, None, None, total, 0, 0, 0, None, None) == E_INVALID
    assert L.murbsep_at(None, 1, None, None, None, None, total, 0, 0, 0, None, None) == E_INVALID
    for text in ("span_sep_ms_avg", "span_sep_count", "Not covered", "several shards", "block is open", "command line",
                 "fma(dz,dz, fma(dy,dy, fma(dx,dx, +0.f)))", "softening never", "v_sqrt_f32", "adds +0", "chunks in ascending order", "(bits(d2) >> sh)",
                 "bin above that edge", "below + sum of hist + above == pairs", "no skip entry", "struck from", "x = +inf",
                 "no global atomic", "no 32-bit counter can wrap", "correctly rounded root"):
        assert text in header, text


def test_python_and_host_interfaces(mh):
    for method in ("separation_of", "separation_at", "mean_separation", "q_parameter"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.mean_separation) and callable(mh.separation_bin) and callable(mh.separation_edges)
    assert callable(mh.shell_density)
    assert hasattr(mh.host_lib(), "murbhost_sim_mean_separation")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint meanSeparation\(double \*mean\)", hpp)
    make = open(os.path.join(ROOT, "nbody-eurohpc_amd", "Makefile")).read()
    assert make.count("../include/murbsep.h") == 2
    assert "3-D" in mh.Simulation.q_parameter.__doc__ and "4/3 pi R^3" in mh.Simulation.q_parameter.__doc__


# ------------------------------------------------------------------------------------------------------ bins and edges, host only
def patterns(lo_exp, sub, bins):
    """float32 bit patterns from +0 to past +inf in steps of a prime, with every edge, its two neighbours, the subnormals' end,
    +inf and two NaNs."""
    e = R.bits(R.edges2(lo_exp, sub, bins)).astype(np.int64)
    near = np.concatenate([e - 1, e, e + 1])
    sweep = np.arange(0, 0x7FC00001, 40009, dtype=np.int64)
    extra = np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x7F800001, 0x7FC00000], np.int64)
    return np.unique(np.concatenate([near[(near >= 0) & (near <= 0x7FC00000)], sweep, extra])).astype(np.uint32)


@pytest.mark.parametrize("lo_exp,sub,bins", [(0, 0, 4), (0, 2, 8), (-10, 4, 1022), (3, 6, 500), (-126, 0, 1), (-126, 6, 1022), (127, 6, 63),
                                             (100, 0, 27), (20, 3, 17)])
def test_bin_against_the_restatement(mh, lo_exp, sub, bins):
    """murbsep_bin equals the restatement's bit rule and the same rule stated through the edges over a sweep of bit patterns, is
    monotone in the bits up to +inf, and puts +inf and NaN above."""
    assert R.valid(lo_exp, sub, bins)
    pat = patterns(lo_exp, sub, bins)
    d2 = pat.view(np.float32)
    L = mh.lib()
    got = np.array([L.murbsep_bin(lo_exp, sub, bins, float(v)) if v == v else mh.separation_bin(lo_exp, sub, bins, v) for v in d2], np.int64)
    assert np.array_equal(got, R.bin_of(d2, lo_exp, sub, bins))
    assert np.array_equal(got, R.bin_by_edges(d2, lo_exp, sub, bins))
    finite = pat <= 0x7F800000
    assert np.all(np.diff(got[finite]) >= 0) and got[finite][0] == -1 and got[finite][-1] == bins
    assert np.all(got[~finite] == bins) and mh.separation_bin(lo_exp, sub, bins, np.inf) == bins
    assert set(got) >= set(range(-1 if lo_exp > -126 else 0, bins + 1)), "every bin, below and above are met"


@pytest.mark.parametrize("lo_exp,sub,bins", [(0, 0, 4), (0, 2, 8), (-10, 4, 1022), (3, 6, 500), (-126, 0, 1), (-126, 6, 1022), (127, 6, 63)])
def test_edges_are_exact(mh, lo_exp, sub, bins):
    """murbsep_edges returns the restatement's floats bit for bit, 2^sub bins per octave, linear in d2 within an octave;
    bin(edge2[k]) == k and bin(nextafter(edge2[k], 0)) == k - 1; edge_r is the fp64 root."""
    edge2, edge_r = mh.separation_edges(lo_exp, sub, bins)
    assert edge2.dtype == np.float32 and edge_r.dtype == np.float64 and edge2.shape == edge_r.shape == (bins + 1,)
    assert np.array_equal(R.bits(edge2), R.bits(R.edges2(lo_exp, sub, bins)))
    assert edge2[0] == np.float32(2.0) ** np.float32(lo_exp) and np.all(np.isfinite(edge2)) and np.all(np.diff(edge2) > 0)
    assert np.array_equal(edge_r, np.sqrt(edge2.astype(np.float64)))
    per = 1 << sub
    for k in range(0, bins + 1 - per, per):
        assert edge2[k + per] == 2 * edge2[k], "an octave"
        assert np.all(np.diff(edge2[k:k + per + 1].astype(np.float64)) == float(edge2[k]) / per), "linear in d2"
    for k in range(bins + 1):
        assert mh.separation_bin(lo_exp, sub, bins, edge2[k]) == k
        assert mh.separation_bin(lo_exp, sub, bins, np.nextafter(edge2[k], np.float32(0))) == k - 1
    L = mh.lib()
    only2 = np.zeros(bins + 1, np.float32)
    assert L.murbsep_edges(lo_exp, sub, bins, only2.ctypes.data_as(C.POINTER(C.c_float)), None) == 0 and np.array_equal(only2, edge2)


def test_host_only_refusals(mh):
    """Parameters out of range and a top edge that is not finite, without a device; shell_density's shapes."""
    L = mh.lib()
    e2, er = np.zeros(2000, np.float32), np.zeros(2000, np.float64)
    p2, pr = e2.ctypes.data_as(C.POINTER(C.c_float)), er.ctypes.data_as(C.POINTER(C.c_double))
    for lo_exp, sub, bins in ((-127, 0, 1), (128, 0, 1), (0, -1, 1), (0, 7, 1), (0, 0, 0), (0, 0, -1), (0, 0, 1023), (0, 0, 128),
                              (127, 0, 1), (127, 6, 64), (-126, 0, 254), (126, 3, 16)):
        assert not R.valid(lo_exp, sub, bins)
        assert L.murbsep_bin(lo_exp, sub, bins, 1.0) == E_INVALID, (lo_exp, sub, bins)
        assert L.murbsep_edges(lo_exp, sub, bins, p2, pr) == E_INVALID, (lo_exp, sub, bins)
        with pytest.raises(mh.MurbHipError):
            mh.separation_bin(lo_exp, sub, bins, 1.0)
        with pytest.raises(mh.MurbHipError):
            mh.separation_edges(lo_exp, sub, bins)
    assert np.all(e2 == 0) and np.all(er == 0), "a refused call writes nothing"
    for lo_exp, sub, bins in ((0, 0, 127), (-126, 0, 253), (126, 3, 15), (127, 6, 63)):
        assert R.valid(lo_exp, sub, bins) and L.murbsep_edges(lo_exp, sub, bins, p2, pr) == 0 and np.isfinite(e2[bins])
    assert L.murbsep_edges(0, 0, 4, None, None) == E_INVALID
    with pytest.raises(ValueError):
        mh.shell_density([1, 2, 3], [1.0, 2.0, 3.0])
    rho = mh.shell_density([7, 0, 26], [0.0, 1.0, 2.0, 3.0])
    assert np.allclose(rho, np.array([7.0, 0.0, 26.0 / 19.0]) / (4.0 / 3.0 * np.pi), rtol=1e-15)


# ------------------------------------------------------------------------------------------------------------- wrong rules
@pytest.fixture(scope="module")
def tie_cases():
    """{name: (exact fp32 d2 matrix, mask or None)} of the tie lattices.  Left unchanged."""
    found = {"grid513": (R.d2_lattice(MR.tie_grid(513)[2]), None),
             "dense2049": (R.d2_lattice(NR.dense_lattice(2049)[2]), None)}
    found["grid513 masked"] = (found["grid513"][0], np.random.default_rng(6).random(513) < 0.4)
    return found


def library_histogram(mh, d2, lo_exp, sub, bins, member, own):
    """The restatement's counting with the LIBRARY's bin of every distinct d2 (murbsep_bin) in the place of its own rule."""
    keep = np.broadcast_to((np.ones(d2.shape[1], bool) if member is None else member)[None, :], d2.shape).copy()
    keep[np.arange(d2.shape[0]), own] = False
    values, inverse = np.unique(d2[keep], return_inverse=True)
    k = np.array([mh.separation_bin(lo_exp, sub, bins, v) for v in values], np.int64)[inverse]
    hist = np.bincount(k[(k >= 0) & (k < bins)], minlength=bins).astype(np.uint64)
    return hist, {"pairs": int(keep.sum()), "below": int((k < 0).sum()), "above": int((k >= bins).sum())}


def test_tie_lattices_sit_on_edges(mh, tie_cases):
    """With edges at the powers of two, a large share of the pairs of the tie lattices has d2 exactly on an edge."""
    for name, (d2, _) in tie_cases.items():
        on_edge = np.isin(d2, mh.separation_edges(0, 0, 12)[0])
        print(name, "pairs on an edge", int(on_edge.sum()), "of", d2.size)
        assert on_edge.sum() > d2.size // 100, "thousands of pairs decide the edge rule"


@pytest.mark.parametrize("rule", ["edge below", "steps in r", "own counted"])
def test_wrong_rules_are_caught(mh, tie_cases, rule):
    """The library's rule (murbsep_bin over the lattice's distinct d2) gives the restatement's histogram on the tie lattices, and
    each deliberately wrong rule gives another result: another histogram for the two binning rules, another below / pairs count
    for the own body."""
    for name, (d2, mask) in tie_cases.items():
        own = np.arange(d2.shape[0])
        for lo_exp, sub, bins in ((0, 0, 10), (0, 2, 40)):
            want = R.histogram(d2, lo_exp, sub, bins, member=mask, own=own)
            lib = library_histogram(mh, d2, lo_exp, sub, bins, mask, own)
            assert np.array_equal(lib[0], want[0]) and lib[1] == want[1], (name, lo_exp, sub, bins)
            got = R.histogram(d2, lo_exp, sub, bins, member=mask, own=own, rule=rule)
            assert want[1]["below"] + int(want[0].sum()) + want[1]["above"] == want[1]["pairs"]
            if rule == "own counted":
                members = d2.shape[0] if mask is None else int(mask.sum())
                assert got[1]["below"] == want[1]["below"] + members and got[1]["pairs"] == want[1]["pairs"] + members, name
            else:
                assert not np.array_equal(got[0], want[0]), (name, lo_exp, sub, bins)


# ----------------------------------------------------------------------------------------- the pure header, stand-alone programs
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "murb_sep.h"
int main() {
    // 1. the launch cut: for every layout the worst workgroup's pairs stay below 2^32, and one group more would not (or the
    //    batch binds)
    const unsigned long bodies[] = {1, 2, 511, 513, 2049, 4096, 65536, 200000, 1000000, 2500001, 3999999, 4000000};
    const long chunk_options[] = {0, 1, 2, 3, 7, 16, 61, 500, 7813};
    const long batch_options[] = {0, 16, 4096, 65536, 1l << 19, (1l << 20) - 16, 1l << 20};
    const long grids[] = {1, 4, 64, 416, 1024, 1216};
    unsigned long cases = 0, bound = 0, refused = 0, smallest = ~0ul;
    for (const unsigned long n : bodies)
        for (const long co : chunk_options)
            for (const long bo : batch_options)
                for (const long grid : grids) {
                    if (!murb_field_options_valid(co, bo)) return 2;
                    const MurbFieldLayout l = murb_field_layout(n, co, bo);
                    const unsigned long most = murb_sep_max_points(l, grid), cut = murb_sep_cut(l, grid);
                    ++cases;
                    if (most % MURB_FIELD_GROUP || cut % MURB_FIELD_GROUP || cut > l.batch || cut > most) return 3;
                    if (most == 0) { ++refused; if (murb_sep_worst_pairs(l, grid, MURB_FIELD_GROUP) <= 0xfffffffful) return 4; continue; }
                    // every launch size up to the cut, sampled, and the cut itself
                    for (unsigned long p = MURB_FIELD_GROUP; p <= cut; p += (cut / 7 / MURB_FIELD_GROUP + 1) * MURB_FIELD_GROUP)
                        if (murb_sep_worst_pairs(l, grid, p) > 0xfffffffful) return 5;
                    if (murb_sep_worst_pairs(l, grid, cut) > 0xfffffffful) return 6;
                    if (murb_sep_worst_pairs(l, grid, most) > 0xfffffffful) return 7;
                    if (murb_sep_worst_pairs(l, grid, most + MURB_FIELD_GROUP) <= 0xfffffffful) return 8;   // the largest such number
                    if (cut < l.batch) { ++bound; if (cut < smallest) smallest = cut; }
                }
    std::printf("%lu %lu %lu %lu", cases, bound, refused, smallest);
    // 2. the worst pairs restated: units by workgroup, counted one by one
    {
        const MurbFieldLayout l = murb_field_layout(2049, 3, 0);   // 5 tiles in 3 chunks: the longest holds 2
        const long grid = 7;
        const unsigned long points = 160;   // 10 groups: 30 units over 7 workgroups: 5 at the most
        unsigned long per[7] = {0};
        for (unsigned long u = 0; u < points / 16 * 3; ++u) per[u % grid] += 16ul * 2 * 512;
        unsigned long worst = 0;
        for (const unsigned long v : per) worst = v > worst ? v : worst;
        std::printf(" %d", (int)(worst == murb_sep_worst_pairs(l, grid, points) && worst == 5ul * 16 * 1024));
    }
    // 3. bins: the slot as an index and as a byte offset agree; the edges are the lowest members of their bins
    int ok = 1;
    for (int sub = 0; sub <= MURB_SEP_SUB_MAX; ++sub)
        for (int lo_exp = -126; lo_exp <= 127; lo_exp += 11) {
            const int sh = murb_sep_shift(sub), base1 = murb_sep_base(lo_exp, sub) - 1;
            for (uint64_t b = 0; b <= 0xffffffffull; b += 6700417ull)
                ok &= 4 * murb_sep_slot((unsigned int)b, sh, base1) == murb_sep_slot_bytes((unsigned int)b, sh, -4 * base1);
            for (int bins = 1; bins <= MURB_SEP_BINS_MAX; bins += 93) {
                if (!murb_sep_params_valid(lo_exp, sub, bins)) continue;
                for (int k = 0; k <= bins; ++k) {
                    const float e = murb_sep_edge2(lo_exp, sub, k);
                    ok &= murb_sep_bin(lo_exp, sub, bins, e) == k && murb_sep_bin(lo_exp, sub, bins, std::nextafter(e, 0.f)) == k - 1;
                }
            }
        }
    std::printf(" %d", ok);
    std::printf(" %d %d %d %d", murb_sep_bin(0, 0, 4, 0.f), murb_sep_bin(0, 0, 4, 3.f), murb_sep_bin(0, 0, 4, 16.f), murb_sep_bin(0, 0, 4, NAN));
    std::printf(" %d %d\n", (int)murb_sep_params_valid(127, 6, 63), (int)murb_sep_params_valid(127, 6, 64));
    return 0;
}
"""


def build_and_run(tmp_path, flags):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr)
    return done.stdout.split()


def check_program(out):
    cases, bound, refused, smallest = (int(v) for v in out[:4])
    print("layouts", cases, "where the counter bound cuts below the batch", bound, "refused", refused, "smallest cut", smallest)
    assert cases == 12 * 9 * 7 * 6 and bound > 0 and smallest >= 16
    assert out[4:6] == ["1", "1"]
    assert out[6:10] == ["-1", "1", "4", "4"] and out[10:12] == ["1", "0"]


def test_launch_cut_keeps_counters_below_2_32(tmp_path):
    """csrc/murb_sep.h is plain C++: g++ compiles it on the CPU with every warning an error.  Over body counts up to 4 000 000,
    batches up to 2^20, chunk options up to the tile count and grids from 1 to 1216 workgroups the cut keeps the worst
    workgroup's pairs below 2^32, is the largest number that does, and binds below the batch in some of them."""
    check_program(build_and_run(tmp_path, []))


def test_header_program_under_sanitizers(tmp_path):
    """The same stand-alone program, with its own main, built with -fsanitize=address,undefined and run directly: no report, the
    same answers."""
    check_program(build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


# --------------------------------------------------------------------------------------------------------------- code object
@pytest.mark.parametrize("hist", [False, True])
def test_sep_kernel_resources(hist):
    """Code-object metadata of a fresh gfx950 build: exactly one murb_sep_sweep_kernel of each form, 0 bytes of scratch, no
    spilled register of either kind, at most 128 vector registers (4 waves per SIMD); 16 384 bytes of LDS for the sum-only form
    and 4 096 more for the counters.  Per pair of interactions and point 3 packed subtractions, 3 packed fmas, 2 roots, 2 minima
    and one packed add in the loop (16 point steps unrolled); the histogram form adds 2 shifts, 2 shift-and-adds, 2 v_med3_i32
    and 2 LDS integer adds without return, and nothing else atomic anywhere."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_sep_sweep_kernel\w*Lb%d" % int(hist))
    assert len(kernels) == 1, "murb_sep_sweep_kernel missing from the code object, or there twice"
    (name, num), = kernels.items()
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){0,12}?\s+\.name:\s+" + re.escape(name) + r"\n", CO.text()).group(1))
    print(name, num, "lds", lds)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128 and num["sgpr_count"] <= 106
    assert lds == 16384 + (4096 if hist else 0)
    count = lambda pattern: len(CO.ops(name, pattern))      # noqa: E731
    sub, add, fma = count(r"^\s+v_pk_add_f32 .*neg_lo"), count(r"^\s+v_pk_add_f32"), count(r"^\s+v_pk_fma_f32")
    root, least = count(r"^\s+v_sqrt_f32"), count(r"^\s+v_min_f32")
    print("packed subtractions", sub, "packed adds", add - sub, "fmas", fma, "roots", root, "minima", least)
    assert (sub, fma, root, least) == (3 * 16, 3 * 16, 2 * 16, 2 * 16) and add - sub >= 16
    med3, shift, lds_add = count(r"^\s+v_med3_i32"), count(r"^\s+v_lshrrev_b32"), count(r"^\s+ds_add_u32")
    print("v_med3_i32", med3, "shifts", shift, "ds_add_u32", lds_add)
    assert (med3, lds_add) == ((2 * 16, 2 * 16) if hist else (0, 0))
    assert not hist or (shift >= 2 * 16 and count(r"^\s+v_lshl_add_u32") >= 2 * 16)
    assert not count(r"ds_add_rtn") and not count(r"global_atomic|flat_atomic|buffer_atomic") and not count(r"scratch_")
    assert not count(r"_f32.*atomic|atomic.*_f32|pk_add_f16"), "no float atomic"
    for other in ("murb_sep_mask_kernel", "murb_sep_rows_kernel", "murb_pot_sweep_kernel", "murb_foreign_sweep_kernel",
                  "murb_knn_sweep_kernel", "murb_bind_sweep_kernel", "murb_nbr_count_kernel"):
        assert len(CO.metadata(other)) == 1, other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_sep_sweep" in entry

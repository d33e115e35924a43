"""CPU: the listed-source read-out's entry points against include/murblist.h, complement_lists and the force split's composition
against tests/helpers/list_ref.py on synthetic arrays, the binding's argument checks, deliberately wrong readings of the definition
on the test inputs, the pure header under g++ alone and under the address and undefined-behaviour sanitizers, and the kernels'
code-object metadata."""
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
import field_ref as F         # noqa: E402
import list_ref as R          # noqa: E402

E_INVALID = -2000
CSRC = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc")


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# -------------------------------------------------------------------------------------------------------------- entry points
def test_list_entry_points_are_exported(mh):
    """include/murblist.h, the binding's list and the library's exports name the same three calls, disjoint from the other
    interfaces' lists; the version is unchanged; a NULL context is refused without a device; the header states what the issue
    makes normative and what is not covered."""
    header = open(os.path.join(ROOT, "include", "murblist.h")).read()
    declared = sorted(re.findall(r"^int (murb(?:list|split)_\w+)\(", header, re.M))
    assert declared == sorted(mh.LIST_EXPORTS) and len(declared) == 3
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murb(?:list|split)_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS) | \
        set(mh.NBR_EXPORTS) | set(mh.BIND_EXPORTS) | set(mh.BOUND_EXPORTS) | set(mh.MST_EXPORTS) | set(mh.SEP_EXPORTS)
    assert not set(mh.LIST_EXPORTS) & others
    L = mh.lib()
    assert L.murbhip_version() == 103
    assert L.murblist_of(None, 1, *[None] * 10) == E_INVALID
    assert L.murblist_at(None, 1, *[None] * 15) == E_INVALID
    assert L.murbsplit_of(None, 1, None, None, 0.0, *[None] * 8) == E_INVALID
    assert L.murblist_of(None, 0, *[None] * 10) == E_INVALID, "a NULL context is refused even with count 0"
    for text in ("(e >> 1) & 63", "half e & 1", "lane step e >> 7", "no skip machinery", "counts twice", "ORDER of the entries",
                 "murb_wave_sum", "no chunks", "+0.0f seven times", "LAST", "replaced by +0", "span_list_ms_avg", "span_list_count",
                 "\"field_batch\"", "\"list_entries\"", "offsets[0] != 0", "not non-decreasing", "outside [0, n)", "without a host round trip",
                 "bit for bit murblist_of's", "Not covered", "Ahmad-Cohen integrator", "resident across steps", "several shards",
                 "block-open", "fp64 sums", "very long lists", "weights per entry", "changes nothing"):
        assert text in header, text


def test_python_and_host_interfaces(mh):
    for method in ("list_field_of", "list_field_at", "irregular_field_of", "force_split"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.force_split) and callable(mh.complement_lists) and callable(mh.split_regular)
    assert hasattr(mh.host_lib(), "murbhost_sim_force_split")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint forceSplit\(float h,", hpp)
    make = open(os.path.join(ROOT, "nbody-eurohpc_amd", "Makefile")).read()
    assert make.count("../include/murblist.h") == 2


# ------------------------------------------------------------------------------------------------ complement and composition
def test_complement_lists_against_the_restatement(mh):
    """Every other body not in the list, ascending, the body itself left out: equal to the set difference written independently,
    for empty, full, unsorted and duplicate-holding lists, a body listed for itself, repeated bodies; list + complement holds
    every other body exactly once where the list had no duplicates and not the body."""
    n = 37
    rng = np.random.default_rng(3)
    bodies = np.array([0, 0, 36, 5, 17, 1, 2], np.int32)
    lists = [[], list(range(1, n)), rng.permutation(n)[:9], [4, 4, 9, 5], [17, 3], [0], list(rng.permutation(n))]
    o, j = R.csr(lists)
    got = mh.complement_lists(n, bodies, o, j)
    want = R.complement(n, bodies, o, j)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for p, (b, mine, rest) in enumerate(zip(bodies, lists, R.lists_of(*got))):
        assert np.all(np.diff(rest) > 0) and b not in rest and not set(rest) & set(mine), p
        assert set(rest) | (set(mine) - {int(b)}) == set(range(n)) - {int(b)}, p
    assert len(R.lists_of(*got)[0]) == n - 1 and len(R.lists_of(*got)[1]) == 0 and len(R.lists_of(*got)[6]) == 0
    empty = mh.complement_lists(5, np.zeros(0, np.int32), np.zeros(1, np.uint64), np.zeros(0, np.int32))
    assert empty[0].tolist() == [0] and empty[1].shape == (0,)
    for bad in (lambda: mh.complement_lists(n, [n], [0, 0], []), lambda: mh.complement_lists(n, [-1], [0, 0], []),
                lambda: mh.complement_lists(n, [0], [0, 1], [n]), lambda: mh.complement_lists(n, [0], [0, 1], [-1]),
                lambda: mh.complement_lists(n, [0], [0, 2], [1]), lambda: mh.complement_lists(n, [0, 1], [0, 1], [1]),
                lambda: mh.complement_lists(n, [0], [1, 1], [1]), lambda: mh.complement_lists(n, [0, 1], [0, 2, 1], [1, 2])):
        with pytest.raises(ValueError):
            bad()


def test_split_composition_against_the_restatement(mh):
    """On synthetic arrays: the listed sources and their complement together are the field of every other body (fp64 restatement
    against field_ref's, to rounding); split_regular is total - irregular formed in fp64 and rounded once, key by key."""
    n = 300
    s = R.system(n)
    bodies = np.array([0, 7, 299, 128, 7], np.int64)
    o, j = R.neighbours_f32(s, 0.2, R.SOFT)
    lists = [R.lists_of(o, j)[b] for b in bodies]
    assert min(len(x) for x in lists) >= 1
    lo, lj = R.csr(lists)
    co, cj = mh.complement_lists(n, bodies, lo, lj)
    p, v, skip = R.body_points(s, bodies)
    part = R.list_f64(p, v, lo, lj, s, R.SOFT)
    rest = R.list_f64(p, v, co, cj, s, R.SOFT)
    whole = F.field_f64(p, v, skip, s, R.SOFT)
    both = R.add_refs(part, rest)
    for k in range(3):
        scale = np.abs(whole[k]).max()
        assert np.abs(both[k] - whole[k]).max() <= 1e-12 * scale, k
    for name in ("a", "j", "phi"):
        assert np.allclose(both[3][name], whole[3][name], rtol=1e-12), name
    rng = np.random.default_rng(9)
    total = {k: rng.standard_normal(50).astype(np.float32) for k in R.KEYS}
    irregular = {k: (total[k] * rng.uniform(0.0, 1.0, 50)).astype(np.float32) for k in R.KEYS}
    irregular["ax"][:5] = total["ax"][:5]                 # exact cancellation: +0
    total["phi"][7], irregular["phi"][7] = np.float32(1.0), np.float32(2.0 ** -30)   # a difference fp32 cannot hold: rounded once
    regular = mh.split_regular(total, irregular)
    for k in R.KEYS:
        want = (total[k].astype(np.float64) - irregular[k].astype(np.float64)).astype(np.float32)
        assert regular[k].dtype == np.float32 and np.array_equal(F.bits(regular[k]), F.bits(want)), k
    assert np.all(F.bits(regular["ax"][:5]) == 0) and regular["phi"][7] == np.float32(1.0)


# --------------------------------------------------------------------------------------------------------- binding-side checks
def test_binding_argument_checks(mh):
    """The shapes the binding checks before it calls the library: offsets of count + 1 entries, idx of offsets[-1] entries, three
    point arrays of one length, velocities all three or none.  No device: the checks come first."""
    sim = object.__new__(mh.Simulation)
    sim.n, sim._h = 8, None
    ok_o, ok_j = np.array([0, 1, 2], np.uint64), np.array([1, 0], np.int32)
    pts = np.zeros((3, 2), np.float32)
    for bad in (lambda: sim.list_field_of([0, 1], [0, 1], [1]), lambda: sim.list_field_of([0, 1], ok_o, [1]),
                lambda: sim.list_field_of([0, 1], ok_o, [1, 0, 3]), lambda: sim.list_field_of(None, ok_o, ok_j),
                lambda: sim.list_field_at(pts[:2], None, ok_o, ok_j), lambda: sim.list_field_at(pts, pts[:2], ok_o, ok_j),
                lambda: sim.list_field_at([pts[0], pts[1], np.zeros(3, np.float32)], None, ok_o, ok_j),
                lambda: sim.list_field_at(pts, None, [0, 1], ok_j), lambda: sim.irregular_field_of([0, 1], h=[0.1, 0.2, 0.3])):
        with pytest.raises(ValueError):
            bad()
    # the library's answer to a NULL context through the binding's own calls: refused, never a crash
    for call in (lambda: sim.list_field_of([0, 1], ok_o, ok_j), lambda: sim.list_field_at(pts, None, ok_o, ok_j),
                 lambda: sim.irregular_field_of([0, 1], h=0.1)):
        with pytest.raises(mh.MurbHipError) as e:
            call()
        assert e.value.code == E_INVALID


# ------------------------------------------------------------------------------------------------------------- wrong rules
def rule_inputs(n=1025):
    """The GPU test's own inputs for the three properties: a list that holds the body itself, a list with a duplicate, lists whose
    lengths are no multiple of a lane step.  (state, points, velocities, own, offsets, idx)."""
    s = R.system(n)
    perm = R.permutation(n)
    bodies = np.array([perm[5], 3, 700], np.int64)
    lists = [perm[:40], np.concatenate([perm[100:130], perm[110:112]]), perm[:129]]   # perm[5] in its own list; two duplicates; 129
    assert bodies[0] in lists[0] and bodies[1] not in lists[1] and bodies[2] not in lists[2]
    p, v, _ = R.body_points(s, bodies)
    return (s, p, v, bodies) + R.csr(lists)


@pytest.mark.parametrize("rule", R.RULES)
def test_wrong_rules_are_told_apart(rule):
    """Each wrong reading of the definition moves the fp64 result of the point it concerns far beyond the bound the GPU tests
    apply, and leaves the other points alone."""
    s, p, v, own, o, j = rule_inputs()
    ref, c = R.bound_of(p, v, o, j, s, R.SOFT)
    wrong = R.list_f64(p, v, o, j, s, R.SOFT, rule=rule, own=own)
    e = R.scaled_errors(wrong[:3], ref)
    hit = {R.RULES[0]: [0], R.RULES[1]: [1], R.RULES[2]: [0, 1, 2]}[rule]
    print(rule, {k: (e[k] / R.U24).round(1).tolist() for k in e}, "bound", c)
    for point in range(3):
        for k in ("a", "j", "phi"):
            if point in hit and not (rule == R.RULES[0] and k != "phi"):   # the own term is G m / soft in phi and 0 in a and j
                assert e[k][point] > 100 * c[k] * R.U24, (rule, k, point)
            elif point not in hit:
                assert e[k][point] == 0.0, (rule, k, point)
    assert c["a"] > 0 and c["phi"] > 0 and max(c.values()) < 64, "the bound is a few units of 2^-24"


# ----------------------------------------------------------------------------------------- the pure header, stand-alone programs
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "murb_list.h"
int main() {
    // 1. every entry of a list has its own (lane, half, lane step); a lane step holds 128 of them; the steps cover the list
    int ok = 1;
    for (unsigned int L : {1u, 2u, 3u, 127u, 128u, 129u, 255u, 256u, 257u, 1024u, 100000u}) {
        std::vector<int> seen((size_t)murb_list_lane_steps(L) * MURB_LIST_STEP, 0);
        for (unsigned int e = 0; e < L; ++e) {
            const int at = murb_list_lane_step(e) * MURB_LIST_STEP + 2 * murb_list_lane(e) + murb_list_half(e);
            ok &= at == (int)e && murb_list_lane(e) < 64 && murb_list_lane_step(e) < murb_list_lane_steps(L);
            ++seen[(size_t)at];
        }
        for (size_t k = 0; k < seen.size(); ++k) ok &= seen[k] == (k < L ? 1 : 0);
        ok &= (unsigned long)murb_list_lane_steps(L) * MURB_LIST_STEP >= L && (unsigned long)(murb_list_lane_steps(L) - 1) * MURB_LIST_STEP < L;
    }
    ok &= murb_list_lane_steps(0) == 0;
    std::printf("%d", ok);
    // 2. the checks: exact-size arrays, so that a read past either end is a sanitizer report
    const unsigned long n = 10;
    std::vector<unsigned long> o = {0, 2, 2, 5};
    std::vector<int> j = {9, 0, 3, 3, 1};
    std::printf(" %d", (int)murb_list_valid(3, o.data(), j.data(), n));
    std::printf(" %d", (int)murb_list_valid(3, nullptr, j.data(), n));
    std::printf(" %d", (int)murb_list_valid(3, o.data(), nullptr, n));
    { auto b = o; b[0] = 1; std::printf(" %d", (int)murb_list_valid(3, b.data(), j.data(), n)); }
    { auto b = o; b[2] = 1; std::printf(" %d", (int)murb_list_valid(3, b.data(), j.data(), n)); }
    { auto b = j; b[4] = 10; std::printf(" %d", (int)murb_list_valid(3, o.data(), b.data(), n)); }
    { auto b = j; b[0] = -1; std::printf(" %d", (int)murb_list_valid(3, o.data(), b.data(), n)); }
    { std::vector<unsigned long> z = {0, 0, 0}; std::printf(" %d", (int)murb_list_valid(2, z.data(), nullptr, n)); }
    { std::vector<unsigned long> z = {0, MURB_LIST_MAX_LEN + 1}; std::printf(" %d", (int)murb_list_valid(1, z.data(), nullptr, n)); }
    { auto b = j; b[4] = 10; std::printf(" %d\n", (int)murb_list_valid(2, o.data(), b.data(), n)); }   // entry 4 belongs to no list of 2 points
    return 0;
}
"""


def build_and_run(tmp_path, flags):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr)
    return done.stdout.split()


WANT = ["1", "1", "0", "0", "0", "0", "0", "0", "1", "0", "1"]


def test_list_header_is_plain_cpp(tmp_path):
    """csrc/murb_list.h is plain C++: g++ compiles it on the CPU with every warning an error.  The lane mapping is a bijection
    onto the lane steps' slots; the checks accept a valid CSR pair and refuse each defect the header lists."""
    assert build_and_run(tmp_path, []) == WANT


def test_list_header_program_under_sanitizers(tmp_path):
    """The same stand-alone program, with its own main, built with -fsanitize=address,undefined and run directly: no report, the
    same answers."""
    assert build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == WANT


# --------------------------------------------------------------------------------------------------------------- code object
def test_list_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one murb_list_sweep_kernel and one murb_list_pack_kernel, 0 bytes of
    scratch, no spilled register of either kind, at most 128 vector registers (4 waves per SIMD at the least), no LDS; no atomic of
    any kind; 16-byte gathers; per packed pair of entries the pair function's 15 v_pk_fma_f32 and 2 v_rsq_f32, in the three loop
    forms of 4, 2 and 1 lane steps: 7 lane steps in all."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    for kernel in ("murb_list_sweep_kernel", "murb_list_pack_kernel"):
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
            fma, rsq, gather = count(r"^\s+v_pk_fma_f32"), count(r"^\s+v_rsq_f32"), count(r"^\s+global_load_dwordx[34]")
            print("v_pk_fma_f32", fma, "v_rsq_f32", rsq, "12- and 16-byte loads", gather)
            assert (fma, rsq) == (15 * 7, 2 * 7) and gather >= 4 * 7
            assert count(r"^\s+v_add_f32_dpp") == 4 * 7, "seven wave sums"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_list_" in entry

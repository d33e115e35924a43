"""CPU: the bound-pair read-out's entry points, its host-only aid (murbbind_elements: the inline function the device shares)
against tests/helpers/bind_ref.py bit for bit and against the closed form, the degenerate inputs, pins on the lattices the GPU
tests use, the argument checks that need no device, and the sweep kernel's code-object metadata."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bind_ref as B          # noqa: E402
import code_object as CO      # noqa: E402

E_INVALID = -2000


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


@pytest.fixture(scope="module")
def lattices():
    """{n: (q_int, v_int, lattice_stats)} of the two lattices the GPU tests use, computed once and left unchanged."""
    out = {}
    for n in (2049, 5121):
        _, _, _, q, v = B.bind_lattice(n)
        out[n] = (q, v, B.lattice_stats(q, v))
    return out


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# -------------------------------------------------------------------------------------------------------------- entry points
def test_bind_entry_points_are_exported(mh):
    """include/murbbind.h, the binding's list and the library's exports name the same three calls and one aid, disjoint from the
    other interfaces' lists; the version is unchanged; a NULL context is refused without a device."""
    header = open(os.path.join(ROOT, "include", "murbbind.h")).read()
    declared = sorted(re.findall(r"^int (murbbind_\w+)\(", header, re.M))
    assert declared == sorted(mh.BIND_EXPORTS) and len(declared) == 4
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbbind_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS) | set(mh.NBR_EXPORTS)
    assert not set(mh.BIND_EXPORTS) & others
    assert mh.lib().murbhip_version() == 103
    L = mh.lib()
    assert L.murbbind_of(None, 1, None, None, None) == E_INVALID
    assert L.murbbind_at(None, 0, *([None] * 10)) == E_INVALID
    assert L.murbbind_pairs(None, None, None, None, 0, None, None) == E_INVALID
    for text in ("span_bind_ms_avg", "span_bind_count", "Not covered", "several shards", "block is open", "binary stop", "regularisation",
                 "hierarchies", "perturber lists", "a <= 0", "softened problem", "half a step behind", "radii in the velocity records",
                 "h(i, j) == h(j, i)", "MUTUAL", "BOUND", "v_rsq_f32", "fma(-gs, inv, 0.5f * w2)", "no atomics"):
        assert text in header, text


def test_python_and_host_interfaces(mh):
    for method in ("bound_partner_of", "bound_partner_at", "binaries"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.binaries) and callable(mh.binary_elements)
    assert hasattr(mh.host_lib(), "murbhost_sim_binaries")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint binaries\(std::vector<int> &i", hpp)
    make = open(os.path.join(ROOT, "nbody-eurohpc_amd", "Makefile")).read()
    assert make.count("../include/murbbind.h") == 2


def test_pure_header_compiles_without_a_device(tmp_path):
    """csrc/murb_bind.h holds the order predicate and the elements and is plain C++: g++ compiles it on the CPU and a program
    built from it gives the library's bits."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include "murb_bind.h"\nint main() {\n'
                   '  const float qi[3] = {0.f, 0.f, 0.f}, vi[3] = {0.f, 0.f, 0.f}, qj[3] = {1.f, 0.f, 0.f}, vj[3] = {0.f, 1.f, 0.f};\n'
                   '  double e[MURB_BIND_ELEMS];\n  murb_bind_elements(0.f, qi, vi, 0.5f, 0.5f, qj, vj, 0.5f, 0.5f, e);\n'
                   '  std::printf("%a %a %a %d %d\\n", e[0], e[1], e[2], (int)murb_bind_before(-1.f, 7, -1.f, 9), (int)murb_bind_before(2.f, 1, 1.f, -1));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "nbody-eurohpc_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    a, e, p, first, second = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert float.fromhex(a) == 1.0 and float.fromhex(e) == 0.0 and float.fromhex(p) == B.TWO_PI
    assert (first, second) == ("1", "0")


# ---------------------------------------------------------------------------------------------------------------- elements
def element_cases():
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(200):
        scale = 10.0 ** rng.uniform(-3, 3)
        cases.append((np.float32(10.0 ** rng.uniform(-2, 2)), np.float32(10.0 ** rng.uniform(-6, -1) * scale),
                      rng.standard_normal(3) * scale, rng.standard_normal(3), np.float32(rng.uniform(0.1, 2.0)),
                      rng.standard_normal(3) * scale, rng.standard_normal(3), np.float32(rng.uniform(0.1, 2.0))))
    cases.append((np.float32(6.674e-11), np.float32(2e8), [1e11, 0, 0], [0, 3e4, 0], np.float32(6e24), [0, 0, 0], [0, 0, 0], np.float32(2e30)))   # SI
    cases.append((np.float32(1.0), np.float32(0.0), [0, 0, 0], [0, 0, 0], np.float32(0.5), [1, 0, 0], [0, 1, 0], np.float32(0.5)))      # circular
    cases.append((np.float32(1.0), np.float32(0.01), [0, 0, 0], [0, 0, 0], np.float32(0.0), [1, 0, 0], [0, 1, 0], np.float32(0.0)))     # two massless
    cases.append((np.float32(1.0), np.float32(0.01), [0, 0, 0], [0, 0, 0], np.float32(0.0), [1, 0, 0], [0, 0, 0], np.float32(0.0)))     # ... at rest
    cases.append((np.float32(1.0), np.float32(0.01), [0, 0, 0], [0, 0, 0], np.float32(1.0), [1, 0, 0], [0, 3, 0], np.float32(1.0)))     # h64 > 0
    cases.append((np.float32(1.0), np.float32(0.0), [0, 0, 0], [0, 0, 0], np.float32(1.0), [2, 0, 0], [0, 2, 0], np.float32(3.0)))      # ... 0 exactly
    cases.append((np.float32(1.0), np.float32(0.5), [3, 4, 5], [1, 0, 0], np.float32(1.0), [3, 4, 5], [0, 1, 0], np.float32(1.0)))      # coincident
    cases.append((np.float32(1.0), np.float32(0.0), [3, 4, 5], [1, 0, 0], np.float32(1.0), [3, 4, 5], [0, 1, 0], np.float32(1.0)))      # ... soft 0
    cases.append((np.float32(1.0), np.float32(0.5), [0, 0, 0], [0, 0, 0], np.float32(1.0), [1, 0, 0], [0, 0, 0], np.float32(0.0)))      # a probe
    return cases


def test_elements_against_the_restatement_bit_for_bit(mh):
    """murbbind_elements through ctypes against bind_ref.elements on random pairs over six decades of length, an SI pair, and the
    degenerate inputs: two massless bodies, h64 >= 0, coincident bodies with and without softening.  Every one of the six doubles
    has the restatement's bits (NaN where it has NaN)."""
    for k, (g, soft, qi, vi, mi, qj, vj, mj) in enumerate(element_cases()):
        got = mh.binary_elements(g, soft, qi, vi, mi, qj, vj, mj)
        want = B.elements(g, soft, np.float32(qi), np.float32(vi), mi, np.float32(qj), np.float32(vj), mj)[0]
        have = np.array([got[key] for key in B.ELEMENT_KEYS])
        same = (bits(have) == bits(want)) | (np.isnan(have) & np.isnan(want))
        assert same.all(), (k, have, want)


def test_elements_known_answers(mh):
    """Two bodies of mass 1/2 on a circular orbit of separation 1 with G = 1 and a softening of 1e-9: a = 1, e = 0, P = 2 pi,
    E_b = mu h = -1/8, to 1e-12.  An eccentric one: a = 2, e = 0.5 from its pericentre state.  Unbound: a < 0, P NaN.  Massless
    pairs: E_b = 0, P NaN.  Coincident bodies with softening: r = 0, finite h; without: h = -inf."""
    e = mh.binary_elements(1.0, 1e-9, [0, 0, 0], [0, 0, 0], 0.5, [1, 0, 0], [0, 1, 0], 0.5)
    for key, want in (("a", 1.0), ("period", 2 * math.pi), ("h", -0.5), ("energy", -0.125), ("r", 1.0)):      # e: closed form 0, below
        assert abs(e[key] - want) <= 1e-12 * abs(want), (key, e[key])
    assert e["e"] == 0.0      # soft2 = 1e-18 vanishes beside d2 = 1 in fp64: rs = 1, h64 = -1/2, L2 = 1, and 1 + 2 h L2 / GM^2 is exactly 0
    # pericentre of a = 2, e = 0.5, GM = 1: r = 1, v^2 = GM (2 / r - 1 / a) = 1.5; sqrt(1.5) is rounded to fp32 on the way in
    v = np.float32(math.sqrt(1.5))
    e = mh.binary_elements(1.0, 0.0, [0, 0, 0], [0, 0, 0], 0.25, [1, 0, 0], [0, v, 0], 0.75)
    a = 1.0 / (2.0 - float(v) ** 2)
    assert abs(e["a"] - a) <= 1e-12 * a and abs(e["a"] - 2.0) < 1e-6
    assert abs(e["e"] - (1.0 - 1.0 / a)) <= 1e-12 and abs(e["period"] - 2 * math.pi * a ** 1.5) <= 1e-11
    assert abs(e["energy"] - 0.1875 * (-0.5 / a)) <= 1e-14
    e = mh.binary_elements(1.0, 0.01, [0, 0, 0], [0, 0, 0], 1.0, [1, 0, 0], [0, 3, 0], 1.0)
    assert e["h"] > 0 and e["a"] < 0 and math.isnan(e["period"]) and e["e"] > 1 and e["energy"] > 0
    e = mh.binary_elements(1.0, 0.01, [0, 0, 0], [0, 0, 0], 0.0, [1, 0, 0], [0, 1, 0], 0.0)
    assert e["energy"] == 0.0 and e["e"] == math.inf and e["h"] == 0.5 and e["a"] == 0.0 and math.isnan(e["period"])
    e = mh.binary_elements(1.0, 0.01, [0, 0, 0], [0, 0, 0], 0.0, [1, 0, 0], [0, 0, 0], 0.0)
    assert e["energy"] == 0.0 and e["e"] == 0.0 and e["h"] == 0.0 and math.isnan(e["a"]) and math.isnan(e["period"])
    e = mh.binary_elements(1.0, 0.5, [3, 4, 5], [1, 0, 0], 1.0, [3, 4, 5], [0, 1, 0], 1.0)
    assert e["r"] == 0.0 and e["h"] == 1.0 - 2.0 / 0.5 and e["a"] == 2.0 / 6.0 and e["e"] == 1.0
    e = mh.binary_elements(1.0, 0.0, [3, 4, 5], [1, 0, 0], 1.0, [3, 4, 5], [0, 1, 0], 1.0)
    assert e["h"] == -math.inf and e["a"] == 0.0 and e["r"] == 0.0


def test_elements_refuse_bad_arguments(mh):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    q = [np.zeros(3, np.float32), np.zeros(3, np.float32), np.ones(3, np.float32), np.zeros(3, np.float32)]
    out = np.full(6, 77.0)
    L = mh.lib()

    def call(g=1.0, soft=0.1, mi=1.0, mj=1.0, hole=None, arrays=q):
        a = [x.ctypes.data_as(fp) for x in arrays]
        o = out.ctypes.data_as(dp)
        if hole is not None and hole < 4:
            a[hole] = None
        if hole == 4:
            o = None
        return L.murbbind_elements(g, soft, a[0], a[1], mi, a[2], a[3], mj, o)
    for hole in range(5):
        assert call(hole=hole) == E_INVALID
    for bad in (-1.0, math.nan, math.inf):
        assert call(g=bad) == E_INVALID and call(soft=bad) == E_INVALID and call(mi=bad) == E_INVALID and call(mj=bad) == E_INVALID
    for k in range(4):
        arrays = [x.copy() for x in q]
        arrays[k][1] = np.nan
        assert call(arrays=arrays) == E_INVALID
    assert (out == 77.0).all()
    assert call() == 0 and (out != 77.0).all()
    with pytest.raises(ValueError):
        mh.binary_elements(1.0, 0.1, [0, 0], [0, 0, 0], 1.0, [1, 0, 0], [0, 0, 0], 1.0)


# ---------------------------------------------------------------------------------------------------------------- the lattices
@pytest.mark.parametrize("n", (2049, 5121))
def test_lattices_exercise_the_rule(lattices, n):
    """Conditions on the inputs of the GPU tests, so that a lattice that exercises nothing fails here: every body's minimal class
    lies at least 1e-3 of w2 / 2 + gs / rs below the next class (500 times the force bound 2e-6: the partner index is determined
    for EVERY body), at least 15 % of the bodies have candidates of the minimal class in several layout tiles, at least 40 % are
    in mutual pairs, and body 0 at the corner next to the origin, where the padding lies, is among them all."""
    q, v, st = lattices[n]
    mutual, bound = B.pair_lists(st["idx"], st["key"])
    print(f"n={n}: smallest class gap {st['gap'].min():.4f}, ties {(st['cnt'] > 1).mean():.3f}, across tiles {(st['span'] > 1).mean():.3f}, "
          f"mutual {2 * len(mutual) / n:.3f}, bound pairs {len(bound)}")
    assert st["gap"].min() >= 1e-3
    assert (st["cnt"] > 1).mean() >= 0.20 and (st["span"] > 1).mean() >= 0.15
    assert 2 * len(mutual) / n >= 0.40 and len(bound) == len(mutual)
    assert (q[:, 0] == 1).all() and st["idx"][0] > 0
    # A probe of G m = 100 at rest on the origin, where the padding lies at rest: a padding slot's h = -100 / 0.5 would be the
    # smallest by far if it were a candidate (the GPU test asks for the real partner).
    real = 0.5 * (v.astype(np.float64) ** 2).sum(0) - 101.0 / np.sqrt((q.astype(np.float64) ** 2).sum(0) + 0.25)
    assert real.min() > -100.0 / 0.5


@pytest.mark.parametrize("n", (2049, 5121))
def test_wrong_rules_are_caught_on_the_lattices(lattices, n):
    """The deliberately wrong rules differ from the rule on the lattices: the nearest neighbour for most bodies (a fast neighbour
    is not the partner), the highest index of the minimal class for every body with a tie, a later tile's win for every body
    whose ties span tiles."""
    _, _, st = lattices[n]
    near, high, later = ((st[k] != st["idx"]).mean() for k in ("nearest", "high", "later"))
    print(f"n={n}: nearest neighbour differs for {near:.3f}, highest index for {high:.3f}, later tile for {later:.3f}")
    assert near > 0.8 and high >= 0.20 and later >= 0.15
    assert np.array_equal(st["high"] != st["idx"], st["cnt"] > 1) and np.array_equal(st["later"] != st["idx"], st["span"] > 1)


def test_planted_systems_are_what_the_gpu_test_needs():
    """bind_ref.planted(): in fp64 the binary's members and the triple's inner pair are each other's partners with h < 0, the
    triple's outer body picks an inner one with h < 0 and is not picked back, and the binary has a = 0.01, e = 0.5 up to the
    fp32 rounding of its coordinates."""
    s, soft, g, info = B.planted()
    key, _ = B.key_matrix(s, g, soft)
    p = key.argmin(1)
    h = key[np.arange(len(p)), p]
    for i, j in (info["binary"], info["inner"]):
        assert p[i] == j and p[j] == i and h[i] < 0
    assert p[info["outer"]] in info["inner"] and h[info["outer"]] < 0 and p[p[info["outer"]]] != info["outer"]
    e = B.state_elements(s, g, soft, [info["binary"]])[0]
    assert abs(e[0] - 0.01) < 1e-3 and abs(e[1] - 0.5) < 0.05 and e[5] > 5 * float(soft)


# --------------------------------------------------------------------------------------------------------------- code object
def test_bind_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one murb_bind_sweep_kernel, 0 bytes of scratch, no spilled register
    of either kind, at most 128 vector registers (4 waves per SIMD); 15 packed instructions and 2 v_rsq_f32 per pair of
    interactions in its plain loop (16 point steps unrolled), plus the rolled exact arm and the 4 steps behind the loop; the other
    sweeps are still there."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_bind_sweep_kernel")
    assert len(kernels) == 1, "murb_bind_sweep_kernel missing from the code object, or there twice"
    (name, num), = kernels.items()
    print(name, num)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128
    packed, rsq = len(CO.ops(name, r"^\s+v_pk_(?:add|mul|fma)_f32")), len(CO.ops(name, r"^\s+v_rsq_f32"))
    print("packed", packed, "v_rsq_f32", rsq)
    assert packed == 15 * (16 + 4 + 4) and rsq == 2 * (16 + 4 + 4)
    assert len(CO.ops(name, r"^\s+v_min3_f32")) == 16 + 4
    for other in ("murb_bind_pack_kernel", "murb_bind_rows_kernel", "murb_bind_pairs_kernel", "murb_force_field_kernel", "murb_knn_sweep_kernel"):
        assert len(CO.metadata(other)) == 1, other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_bind_sweep" in entry

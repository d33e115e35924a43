"""CPU: the k-nearest-neighbour read-out's entry points, its two host-only aids (murbknn_merge: the chunk fold's function;
murbknn_density: the estimator) against tests/helpers/knn_ref.py on the dense tie lattice, the argument checks that need no
device, and the sweep kernel's code-object metadata."""
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
import knn_ref as K           # noqa: E402
import nearest_ref as NR      # noqa: E402

E_INVALID = -2000
N = 2049
TILES = 5


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


@pytest.fixture(scope="module")
def dense():
    """(q_int, soft2, masses, {k: per-tile lists}, {k: full lists}) of dense_lattice(2049), computed once and left unchanged."""
    s, soft, q = NR.dense_lattice(N)
    soft2 = np.float32(soft) * np.float32(soft)
    tiles = {k: [K.knn(q, soft2, k, t * K.TILE, (t + 1) * K.TILE) for t in range(TILES)] for k in (6, 8)}
    full = {k: K.knn(q, soft2, k) for k in (6, 8)}
    return q, soft2, s["m"], tiles, full


# -------------------------------------------------------------------------------------------------------------- entry points
def test_knn_entry_points_are_exported(mh):
    """include/murbknn.h, the binding's list and the library's exports name the same four calls and two aids, disjoint from the
    other interfaces' lists; the version is unchanged; a NULL context is refused without a device."""
    header = open(os.path.join(ROOT, "include", "murbknn.h")).read()
    declared = sorted(re.findall(r"^int (murb(?:knn|density)_\w+)\(", header, re.M))
    assert declared == sorted(mh.KNN_EXPORTS) and len(declared) == 6
    assert '#include "murbhip.h"' in header and "#define MURBKNN_KMAX 32" in header and mh.KNN_KMAX == 32
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murb(?:knn|density)_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    assert not set(mh.KNN_EXPORTS) & (set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS))
    assert mh.lib().murbhip_version() == 103
    assert mh.lib().murbknn_of(None, 6, 1, None, None, None) == E_INVALID
    assert mh.lib().murbknn_at(None, 6, 0, *([None] * 6)) == E_INVALID
    assert mh.lib().murbdensity_of(None, 6, 1, None, None) == E_INVALID
    assert mh.lib().murbdensity_centre(None, 6, None) == E_INVALID
    for text in ("span_knn_ms_avg", "span_knn_count", "Not covered", "several shards", "block is open", "k > 32", "integrator input"):
        assert text in header, text


def test_python_and_host_interfaces(mh):
    for method in ("knn_of", "knn_at", "density", "density_centre"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.density_centre) and callable(mh.knn_merge) and callable(mh.knn_density)
    assert hasattr(mh.host_lib(), "murbhost_sim_density_centre") and hasattr(mh.host_lib(), "murbhost_sim_set_density_centre")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint densityCentre\(int k", hpp)
    main = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "murb", "main.cpp")).read()
    assert '"hip+tracking+density"' in main


def test_aids_refuse_bad_arguments(mh):
    """k outside [1, 32] (density: [2, 32]) and NULL pointers: MURBHIP_E_INVALID, and the outputs untouched."""
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    i, r = np.arange(40, dtype=np.int32), np.arange(40, dtype=np.float32)
    io, ro = np.full(40, 77, np.int32), np.full(40, 77, np.float32)
    a = lambda x: x.ctypes.data_as(ip if x.dtype == np.int32 else fp)      # noqa: E731
    L = mh.lib()
    for k in (0, -1, 33):
        assert L.murbknn_merge(k, a(i), a(r), a(i), a(r), a(io), a(ro)) == E_INVALID
        assert L.murbknn_density(k, a(i), a(r), a(r), 0.5, a(ro)) == E_INVALID
    assert L.murbknn_density(1, a(i), a(r), a(r), 0.5, a(ro)) == E_INVALID
    for hole in range(6):
        args = [a(i), a(r), a(i), a(r), a(io), a(ro)]
        args[hole] = None
        assert L.murbknn_merge(6, *args) == E_INVALID
    for hole in (0, 1, 2, 4):
        args = [a(i), a(r), a(r), 0.5, a(ro)]
        args[hole] = None
        assert L.murbknn_density(6, *args) == E_INVALID
    assert (io == 77).all() and (ro == 77).all()
    assert L.murbknn_merge(32, a(i), a(r), a(i), a(r), a(io), a(ro)) == 0


# ----------------------------------------------------------------------------------------------------------------- the merge
def test_lattice_has_the_ties_the_merge_is_tested_on(dense):
    """The figures the tests below rest on: the share of bodies whose k-th and (k + 1)-th candidates have the same r2 (61 % at
    k = 6, 97 % at k = 8), and that nearly every list spans at least two tiles."""
    q, soft2, _, _, full = dense
    for k, share in ((6, 0.61), (8, 0.97)):
        _, r2 = K.knn(q, soft2, k + 1)
        tied = float((r2[:, k - 1] == r2[:, k]).mean())
        span = np.array([len(set(row // K.TILE)) for row in full[k][0]])
        print(f"k={k}: {tied:.3f} of the bodies tie across the k-th place; {float((span >= 2).mean()):.3f} of the lists span >= 2 tiles")
        assert abs(tied - share) < 0.01 and (span >= 2).mean() > 0.95


@pytest.mark.parametrize("k", (6, 8))
def test_merge_of_tile_lists_is_the_full_list(mh, dense, k):
    """Lists cut at every tile boundary of dense_lattice(2049), folded left to right with murbknn_merge: the restatement's full
    lists, bit for bit, for every body."""
    _, _, _, tiles, full = dense
    lists = tiles[k]
    for b in range(N):
        idx, r2 = lists[0][0][b], lists[0][1][b]
        for t in range(1, TILES):
            idx, r2 = mh.knn_merge(idx, r2, lists[t][0][b], lists[t][1][b])
        assert np.array_equal(idx, full[k][0][b]) and np.array_equal(r2, full[k][1][b]), b


def test_merge_fold_is_associative(mh, dense):
    """Any grouping of the tiles into chunks gives the same list: ((01)(234)), (0(1(2(34)))), ((04)(13))2 in shuffled order."""
    _, _, _, tiles, full = dense
    L = tiles[6]

    def m(x, y):
        return mh.knn_merge(x[0], x[1], y[0], y[1])
    for b in range(0, N, 7):
        t = [(L[c][0][b], L[c][1][b]) for c in range(TILES)]
        for got in (m(m(t[0], t[1]), m(m(t[2], t[3]), t[4])), m(t[0], m(t[1], m(t[2], m(t[3], t[4])))), m(m(m(t[4], t[0]), m(t[3], t[1])), t[2])):
            assert np.array_equal(got[0], full[6][0][b]) and np.array_equal(got[1], full[6][1][b]), b


def test_merge_takes_an_entry_listed_twice_once_and_fills_tails(mh):
    idx, r2 = mh.knn_merge([3, 9, -1], [1.0, 2.0, np.inf], [3, 5, -1], [1.0, 2.0, np.inf])
    assert idx.tolist() == [3, 5, 9] and r2.tolist() == [1.0, 2.0, 2.0]
    idx, r2 = mh.knn_merge([4, -1, -1], [1.0, np.inf, np.inf], [-1, -1, -1], [np.inf] * 3)
    assert idx.tolist() == [4, -1, -1] and r2.tolist() == [1.0, np.inf, np.inf]


def test_wrong_tie_rule_is_caught(dense):
    """The deliberately wrong rule "higher index wins a tie" in the fold changes the k = 6 set of 1 259 of the 2 049 bodies."""
    _, _, _, tiles, full = dense
    L = tiles[6]
    changed = 0
    for b in range(N):
        idx, r2 = L[0][0][b], L[0][1][b]
        for t in range(1, TILES):
            idx, r2 = K.merge(idx, r2, L[t][0][b], L[t][1][b], high_wins=True)
        changed += set(idx.tolist()) != set(full[6][0][b].tolist())
    print(f"higher index wins: {changed} of {N} sets differ")
    assert changed == 1259


def test_reference_merge_agrees_with_the_library(mh, dense):
    _, _, _, tiles, _ = dense
    L = tiles[8]
    for b in range(0, N, 11):
        want = K.merge(L[1][0][b], L[1][1][b], L[3][0][b], L[3][1][b])
        got = mh.knn_merge(L[1][0][b], L[1][1][b], L[3][0][b], L[3][1][b])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# --------------------------------------------------------------------------------------------------------------- the density
def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(same, 0, d)


def test_density_against_the_restatement(mh, dense):
    """murbknn_density against numpy fp64, to 1 ulp of fp32 (the fp64 steps are the same; the only freedom is sqrt), on the dense
    lattice's lists: bodies on one point (d2 == 0: +inf), massless neighbours (bodies 12 and 700)."""
    q, soft2, m, _, full = dense
    soft = np.float32(0.5)
    for k in (6, 8):
        idx, r2 = full[k]
        want = K.density(idx, r2, m, soft2)
        got = np.array([mh.knn_density(idx[b], r2[b], m, soft) for b in range(N)], np.float32)
        assert ulps(got, want).max() <= 1
        assert np.isfinite(got).sum() > 2000 and (got[np.isfinite(got)] > 0).all()
    idx, r2 = K.knn(q, soft2, 2)
    got = np.array([mh.knn_density(idx[b], r2[b], m, soft) for b in NR.DENSE_TRIPLE])      # both others on the body's own point
    assert np.isinf(got).all() and (got > 0).all(), "k bodies on one point"
    assert np.isfinite([mh.knn_density(idx[b], r2[b], m, soft) for b in (10, 11)]).all(), "one other on the point: the 2nd is not"
    assert any(12 in row[:5] or 700 in row[:5] for row in full[6][0]), "no massless neighbour in any list"


def test_density_edge_cases(mh):
    """Fewer than k candidates: +0.  One massless neighbour: its mass is not counted.  d2 == 0 with massless neighbours: +inf, not
    NaN.  The k-th neighbour's mass is not counted.  A known answer: M = 3 inside r = 2: 3 / (4/3 pi 8)."""
    m = np.array([1.0, 2.0, 0.0, 8.0], np.float32)
    soft = np.float32(0.5)
    s2 = float(soft * soft)
    assert mh.knn_density([1, -1], [1.0, np.inf], m, soft) == 0.0 and not np.signbit(mh.knn_density([1, -1], [1.0, np.inf], m, soft))
    got = mh.knn_density([0, 1, 3], np.array([1.0, 2.0, 4.0]) + s2, m, soft)
    assert ulps(got, np.float32(3.0 / (K.FOUR_THIRDS_PI * 8.0))) <= 1
    assert mh.knn_density([2, 3], np.array([1.0, 1.0]) + s2, m, soft) == 0.0
    assert mh.knn_density([2, 3], [s2, s2], m, soft) == np.inf
    assert mh.knn_density([0, 3], [s2, s2], m, soft) == np.inf
    for args in (([1, -1], [1.0, np.inf]), ([0, 1, 3], np.array([1.0, 2.0, 4.0]) + s2), ([2, 3], [s2, s2])):
        assert ulps(mh.knn_density(*args, m, soft), K.density(np.array(args[0]), np.array(args[1], np.float32), m, soft * soft)[0]) <= 1


# --------------------------------------------------------------------------------------------------------------- code object
def test_knn_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one murb_knn_sweep_kernel, 0 bytes of scratch, 0 spilled registers,
    at most 128 vector registers (4 waves per SIMD); its loop forms r2 in packed arithmetic; the field sweep is still there."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_knn_sweep_kernel")
    assert len(kernels) == 1, "murb_knn_sweep_kernel missing from the code object, or there twice"
    (name, num), = kernels.items()
    print(name, num)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128
    assert len(CO.ops(name, r"^\s+v_pk_fma_f32")) >= 12 and len(CO.ops(name, r"wave_shr:1")) >= 2
    assert len(CO.metadata(r"murb_force_field_kernel")) == 1
    for other in ("murb_knn_rows_kernel", "murb_knn_density_kernel", "murb_knn_centre_kernel"):
        assert len(CO.metadata(other)) == 1, other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_knn_sweep" in entry

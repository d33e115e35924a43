"""CPU: the neighbours-within-a-radius read-out's entry points, its host-only aids (murbnbr_threshold, murbnbr_cut,
murbhip.fof_groups) against tests/helpers/nbr_ref.py, the known answers of the dense lattice the GPU tests rest on, and the two
sweep kernels' code-object metadata."""
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
import nbr_ref as NB          # noqa: E402
import nearest_ref as NR      # noqa: E402

E_INVALID = -2000
N = 2500
TOTALS = {0: 12, 1: 12678, 2: 62386, 3: 213992}      # dense_lattice(2500), soft 0.5: entries of all bodies' lists at h
MAXIMA = {0: 2, 1: 7, 2: 33, 3: 118}                 # ... and the longest list


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


@pytest.fixture(scope="module")
def dense():
    """(q_int, soft2, {h: lists of all bodies}) of dense_lattice(2500), computed once and left unchanged."""
    _, soft, q = NR.dense_lattice(N)
    soft2 = np.float32(soft) * np.float32(soft)
    return q, soft2, {h: NB.neighbours(q, soft2, h) for h in TOTALS}


# -------------------------------------------------------------------------------------------------------------- entry points
def test_nbr_entry_points_are_exported(mh):
    """include/murbnbr.h, the binding's list and the library's exports name the same six calls, disjoint from the other
    interfaces' lists; the version is unchanged; a NULL context is refused without a device."""
    header = open(os.path.join(ROOT, "include", "murbnbr.h")).read()
    declared = sorted(re.findall(r"^int (murbnbr_\w+)\(", header, re.M))
    assert declared == sorted(mh.NBR_EXPORTS) and len(declared) == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbnbr_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    others = set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS) | set(mh.TRACER_EXPORTS) | set(mh.KNN_EXPORTS)
    assert not set(mh.NBR_EXPORTS) & others
    assert mh.lib().murbhip_version() == 103
    off = (C.c_ulong * 2)()
    assert mh.lib().murbnbr_of(None, 1, None, None, 1.0, off, None, None, 0) == E_INVALID
    assert mh.lib().murbnbr_at(None, 0, None, None, None, None, None, 1.0, off, None, None, 0) == E_INVALID
    assert mh.lib().murbnbr_set_option(None, b"list_entries", 0) == E_INVALID
    assert mh.lib().murbnbr_get_option(None, b"list_entries", C.byref(C.c_long())) == E_INVALID


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "murbnbr.h")).read()
    for text in ('#include "murbhip.h"', "r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))", "thr = (float)((double)h * h + (double)soft2)",
                 "r2 <= thr", "ASCENDING BODY INDEX", "offsets[0] = 0", "Massless bodies are candidates", "padding slots", "Count-only",
                 "idx and r2 are untouched", '"list_entries"', "1 << 26", "span_nbr_ms_avg", "span_nbr_count", "Not covered",
                 "several shards", "block is open", "sums over the sphere", "integrator's input", "sorted by distance"):
        assert text in header, text
    for name, phrase in (("murbknn.h", "neighbours within a radius"), ("murbhip.h", "full neighbour lists")):
        text = open(os.path.join(ROOT, "include", name)).read()
        at = text.index(phrase)
        assert "murbnbr.h" in text[at:at + 200], name + " does not point at murbnbr.h"


def test_python_and_host_interfaces(mh):
    for method in ("neighbours_of", "neighbours_at", "set_neighbour_option", "neighbour_option"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.neighbours_of) and callable(mh.neighbour_threshold) and callable(mh.fof_groups)
    assert mh.NBR_OPTIONS == ("list_entries",)
    assert hasattr(mh.host_lib(), "murbhost_sim_neighbours_of")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint neighboursOf\(float h, std::vector<unsigned long> ?&offsets, std::vector<int> ?&idx\)", hpp)


# ------------------------------------------------------------------------------------------------------------- the threshold
def test_threshold_is_the_encounter_rule(mh):
    """murbnbr_threshold against nearest_ref.threshold: h = 0 gives soft2 itself, a square beyond fp32 gives +inf, and a sweep of
    radii and softenings whose sums need both roundings."""
    rng = np.random.default_rng(5)
    soft = np.float32(0.5)
    assert mh.neighbour_threshold(0.0, soft) == np.float32(0.25)
    assert mh.neighbour_threshold(1.0, soft) == np.float32(1.25)
    assert np.isposinf(mh.neighbour_threshold(3e19, soft)) and np.isposinf(NR.threshold(3e19, soft * soft))
    assert np.isfinite(mh.neighbour_threshold(1.8e19, soft))
    for h, s in zip(rng.uniform(0, 3, 200).astype(np.float32), rng.uniform(0, 1, 200).astype(np.float32)):
        assert mh.neighbour_threshold(h, s) == NR.threshold(h, s * s), (h, s)
    for h, s in ((1e-3, 2e8), (7.3e9, 2e8), (1e-20, 1e-20)):
        assert mh.neighbour_threshold(h, s) == NR.threshold(h, np.float32(s) * np.float32(s))
    out = np.full(1, 77, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    for h, s in ((-1.0, 0.5), (np.nan, 0.5), (np.inf, 0.5), (1.0, -0.5), (1.0, np.nan), (1.0, np.inf)):
        assert mh.lib().murbnbr_threshold(h, s, fp) == E_INVALID
    assert mh.lib().murbnbr_threshold(1.0, 0.5, None) == E_INVALID and out[0] == 77


# -------------------------------------------------------------------------------------------------------------------- the cut
def test_cut_on_hand_made_offsets(mh):
    """offsets of lists of 3, 0, 5, 5, 2, 0, 0, 9 and 1 entries."""
    off = np.cumsum([0, 3, 0, 5, 5, 2, 0, 0, 9, 1]).astype(np.uint64)
    cut = lambda first, entries: mh.neighbour_cut(off, first, entries)      # noqa: E731
    assert cut(0, 2) == 1, "a budget smaller than one list: that list alone"
    assert cut(7, 8) == 8 and cut(7, 0) == 8
    assert cut(0, 3) == 2, "an exact fit, and the empty list behind it comes along"
    assert cut(0, 8) == 3 and cut(0, 7) == 2 and cut(0, 13) == 4 and cut(0, 12) == 3, "exact fits and one short of them"
    assert cut(4, 2) == 7, "empty lists cost nothing"
    assert cut(0, 23) == 7 and cut(0, 24) == 8 and cut(0, 25) == 9 and cut(0, 10 ** 9) == 9, "the last range ends at count"
    assert cut(8, 0) == 9 and cut(8, 1) == 9
    assert cut(1, 0) == 2, "an empty first list, and nothing fits behind it"
    # walking the ranges covers every point once, whatever the budget
    for entries in (0, 1, 4, 5, 9, 10, 30):
        first, seen = 0, []
        while first < 9:
            last = cut(first, entries)
            assert first < last <= 9
            assert last == first + 1 or off[last] - off[first] <= entries
            assert last == 9 or off[last + 1] - off[first] > entries, "not the furthest point"
            seen += list(range(first, last))
            first = last
        assert seen == list(range(9))
    up = C.POINTER(C.c_ulong)
    last = C.c_ulong(77)
    assert mh.lib().murbnbr_cut(9, off.ctypes.data_as(up), 9, 5, C.byref(last)) == E_INVALID, "first >= count"
    assert mh.lib().murbnbr_cut(9, None, 0, 5, C.byref(last)) == E_INVALID
    assert mh.lib().murbnbr_cut(9, off.ctypes.data_as(up), 0, 5, None) == E_INVALID and last.value == 77


# ---------------------------------------------------------------------------------------------------------- the dense lattice
def test_dense_lattice_known_answers_and_teeth(dense):
    """The totals and maxima the GPU test asserts, from the restatement.  The fixture has teeth: face neighbours sit exactly at
    r2 = 1.25 = thr(h = 1), so the deliberately wrong rule `<` changes the h = 1 total; bodies on one point sit at r2 = soft2 =
    thr(h = 0)."""
    q, soft2, lists = dense
    for h, (offsets, idx, r2) in lists.items():
        counts = np.diff(offsets.astype(np.int64))
        print(f"h={h}: total {int(offsets[-1])}, longest list {counts.max()}")
        assert int(offsets[-1]) == TOTALS[h] and counts.max() == MAXIMA[h]
        own = np.repeat(np.arange(N), counts)
        assert (idx != own).all() and (idx >= 0).all() and (idx < N).all()
        assert (r2 <= NR.threshold(h, soft2)).all()
        for p in (0, 14, 600, N - 1):
            row = idx[int(offsets[p]):int(offsets[p + 1])]
            assert (np.diff(row) > 0).all(), "not ascending in index"
    assert NR.threshold(1, soft2) == np.float32(1.25)
    wrong = NB.neighbours(q, soft2, 1, strict=True)
    print(f"h=1 with `<`: total {int(wrong[0][-1])} instead of {TOTALS[1]}")
    assert int(wrong[0][-1]) == TOTALS[0] < TOTALS[1], "with `<` only the bodies on one point are left"
    assert int(NB.neighbours(q, soft2, 0, strict=True)[0][-1]) == 0
    # bodies on one point list each other at h = 0: the pairs and the triple of nearest_ref.dense_lattice
    offsets, idx, _ = lists[0]
    row = lambda p: idx[int(offsets[p]):int(offsets[p + 1])].tolist()      # noqa: E731
    assert row(10) == [11] and row(11) == [10] and row(12) == [1500] and row(13) == [N - 2]
    assert row(14) == [600, 1100] and row(600) == [14, 1100] and row(1100) == [14, 600] and row(0) == []


def test_reference_subsets_radii_and_points(dense):
    """The restatement's own consistency: a subset's lists are the rows of the full ones; per-point radii pick the rows of the
    common-h lists; points on the bodies with the body skipped are the bodies' lists."""
    q, soft2, lists = dense
    sub = np.array([7, 7, N - 1, 0, 14, 600], np.int64)
    h = np.array([0, 1, 2, 3, 0, 1], np.float32)
    got = NB.neighbours(q, soft2, h, bodies=sub)
    at = NB.neighbours_at(q, soft2, h, q[:, sub], skip=sub)
    assert NB.same(got, at)
    for e, (b, hh) in enumerate(zip(sub, h)):
        o, i, r = lists[int(hh)]
        want = i[int(o[b]):int(o[b + 1])]
        assert np.array_equal(got[1][int(got[0][e]):int(got[0][e + 1])], want)
    none = NB.neighbours_at(q, soft2, 0, q[:, sub])
    assert np.diff(none[0].astype(np.int64)).tolist() == [1, 1, 1, 1, 3, 3], "without a skip the body itself is listed"


def test_fof_groups_against_bfs(mh, dense):
    """murbhip.fof_groups on the h = 1 lists of the dense lattice against a breadth-first search on its r2 matrix: the same
    labels, each the smallest index of its component; the lattice is one big group and some small ones."""
    q, soft2, lists = dense
    offsets, idx, _ = lists[1]
    got = mh.fof_groups(offsets, idx)
    inside = NR.r2_matrix(q, soft2) <= NR.threshold(1, soft2)
    assert np.array_equal(inside, inside.T)
    want = NB.fof_bfs(inside)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    sizes = np.bincount(got)
    print(f"h=1: {int((sizes > 0).sum())} groups, the largest of {sizes.max()} bodies")
    assert (sizes > 0).sum() > 1 and sizes.max() > N // 2
    assert (got <= np.arange(N)).all() and (got[got] == got).all()
    assert got[NR.DENSE_PARTNER] == NR.DENSE_PARTNER and got[N - 1] == NR.DENSE_PARTNER, "the far pair is a group of two"
    h0 = mh.fof_groups(*lists[0][:2])
    assert h0[11] == 10 and h0[1500] == 12 and h0[600] == 14 and h0[1100] == 14 and (h0 != np.arange(N)).sum() == 5
    assert np.array_equal(mh.fof_groups(np.zeros(4, np.uint64), np.zeros(0, np.int32)), np.arange(3))
    with pytest.raises(ValueError):
        mh.fof_groups(offsets, idx[:-1])


# --------------------------------------------------------------------------------------------------------------- code object
def test_nbr_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one count and one fill kernel, 0 bytes of scratch, 0 spilled
    registers, at most 128 vector registers (4 waves per SIMD); both loops form r2 in packed arithmetic; the knn and field
    sweeps are still there once each."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    for kernel in ("murb_nbr_count_kernel", "murb_nbr_fill_kernel"):
        kernels = CO.metadata(kernel)
        assert len(kernels) == 1, kernel + " missing from the code object, or there twice"
        (name, num), = kernels.items()
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
        assert num["vgpr_count"] <= 128
        assert len(CO.ops(name, r"^\s+v_pk_fma_f32")) >= 12
    assert len(CO.metadata(r"murb_knn_sweep_kernel")) == 1 and len(CO.metadata(r"murb_force_field_kernel")) == 1
    for other in ("murb_nbr_pack_kernel", "murb_nbr_rows_kernel", "murb_field_pack_kernel"):
        assert len(CO.metadata(other)) == 1, other
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "murb_nbr_" in entry

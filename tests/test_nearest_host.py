"""CPU: nearest neighbours from the Hermite sweeps (option "nearest") and the encounter stop.  The library, the binding and the
header carry the entry points; the numpy restatement (tests/helpers/nearest_ref.py, written from include/murbhip.h) gives the
same answer however the j range is cut; the two nearest-neighbour kernels of a fresh gfx950 build use no scratch, spill
nothing, keep the plain sweep's packed arithmetic, and leave the plain kernels' registers as they were."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import code_object as CO   # noqa: E402
import nearest_ref as N   # noqa: E402

E_INVALID = -2000


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


def test_nearest_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_download_nearest", "murbhip_set_encounter", "murbhip_encounters"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    for method in ("nearest", "set_encounter", "encounters"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.encounters)
    for name in ("murbhost_sim_set_encounter", "murbhost_sim_encounters"):
        assert hasattr(mh.host_lib(), name)
    # the argument checks that need no device: no context
    count, time = C.c_ulong(), C.c_double()
    assert mh.lib().murbhip_download_nearest(None, None, None) == E_INVALID
    assert mh.lib().murbhip_set_encounter(None, 1.0) == E_INVALID
    assert mh.lib().murbhip_encounters(None, None, None, None, 0, C.byref(count), C.byref(time)) == E_INVALID


@pytest.mark.parametrize("n", [2, 513, 2049, 3072])
def test_chunked_fold_equals_brute_force(n):
    """6 layout tiles cut into 1, 3 and 6 chunks (and the device's own tile count): the lexicographic fold over the chunks
    is the brute-force answer, on a lattice with deliberate ties (equal distances inside a tile and across tiles, two bodies
    on one point, a body on the origin where the padding lies)."""
    s, soft = N.lattice(n)
    q = np.stack([s[k] for k in ("qx", "qy", "qz")])
    idx, r2 = N.nearest(q, 0.25, exact=True)
    assert (idx != np.arange(n)).all() and (idx >= 0).all() and (idx < n).all()
    if n >= 513:
        assert idx[8] == 7 and idx[20] == 21 and idx[30] == 100 and idx[5] == 400 and idx[400] == 5
        assert r2[5] == np.float32(0.25) and r2[20] == np.float32(4.25) and r2[30] == np.float32(9.25)
    for chunks in (1, 3, 6):
        got_idx, got_r2 = N.chunked(q, 0.25, n, 6, chunks)
        assert np.array_equal(got_idx, idx) and np.array_equal(got_r2.view(np.uint32), r2.view(np.uint32)), chunks
    # the fp64 form agrees on a lattice: the exact index is a candidate, the minimum is the exact r2
    best, cand = N.nearest(q, 0.25)
    assert cand[np.arange(n), idx].all() and np.array_equal(best, r2.astype(np.float64))


def test_lone_body_and_threshold():
    idx, r2 = N.nearest(np.zeros((3, 1)), 0.25, exact=True)
    assert idx[0] == -1 and np.isinf(r2[0])
    idx, r2 = N.chunked(np.zeros((3, 1)), 0.25, 1, 2, 2)
    assert idx[0] == -1 and np.isinf(r2[0])
    assert N.threshold(3.0, 0.25) == np.float32(9.25)
    r = float(np.float32(3e10))      # the radius is an fp32 argument; the square and the sum are fp64, one rounding at the end
    assert N.threshold(3e10, np.float32(1e6) ** 2) == np.float32(r * r + float(np.float32(1e6) ** 2))
    a, b = N.lex_min(np.float32([1, 2, 2]), np.int32([5, 5, 9]), np.float32([1, 3, 2]), np.int32([3, 1, 4]))
    assert a.tolist() == [1, 2, 2] and b.tolist() == [3, 5, 4]


PARENT_VGPRS = {"murb_force_jerk_kernel": 96, "murb_force_jerk_adaptive_kernel": 96, "murb_force_jerk_block_kernel": 95}


def test_nearest_kernels_use_no_scratch():
    """Code-object metadata of a fresh gfx950 build (the method of test_hermite_block_host.py): both nearest-neighbour sweeps are
    there with 0 bytes of scratch and 0 spilled registers, their packed fp32 instructions, reciprocal square roots and LDS
    reads are exactly the plain sweep's, and they fit 4 waves per SIMD (at most 128 vector registers; DESIGN.md 4.9 records
    that decision and what it costs).  The plain kernels keep the register counts they had before the option existed."""
    hipcc = CO.hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed: no code object to inspect")
    seen = {}
    for name, num in CO.metadata(r"murb_nn_|murb_force_jerk_").items():
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0, name
        short = re.search(r"(murb_[a-z_]+_kernel)", name).group(1)
        seen[short] = num["vgpr_count"]
    for want in ("murb_nn_sweep_kernel", "murb_nn_active_sweep_kernel"):
        assert want in seen, want + " missing from the code object"
        assert seen[want] <= 128, want + " no longer fits 4 waves per SIMD"
    for name, vgprs in PARENT_VGPRS.items():
        assert seen[name] == vgprs, f"{name}: {seen[name]} vector registers, {vgprs} before the option existed"
    assert sum("DESIGN" in f for f in os.listdir(ROOT)) and "4 waves per SIMD" in open(os.path.join(ROOT, "DESIGN.md")).read()

    def packed(kernel):
        return sorted(CO.ops(kernel, r"^\s*(v_pk_\w+|v_rsq_f32\w*|ds_read_b128)\b"))

    plain = packed("murb_force_jerk_kernel")
    assert len(plain) > 100
    for want in ("murb_nn_sweep_kernel", "murb_nn_active_sweep_kernel"):
        assert packed(want) == plain, want


# ------------------------------------------------------------------------------------------------------ the dense tie lattice
DENSE_N = (2049, 2561, 4609)


@lru_cache(maxsize=None)
def dense(n):
    """(state, q, q2, k, r2 matrix of q, of q2): conditions on the inputs of tests/test_tie_lattice_gpu.py, not measurements."""
    s, soft, q = N.dense_lattice(n)
    assert soft == np.float32(0.5)
    q2, k = N.shifted(q)
    return s, q, q2, k, N.r2_matrix(q, 0.25), N.r2_matrix(q2, 0.25)


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_lattice_ties(n):
    """Nearly every row of the dense lattice is a tie, most ties span tiles and cross the border of the body's own tile, and a
    wrong tie rule changes the answer almost everywhere."""
    s, q, q2, k, r2m, r2m2 = dense(n)
    idx, r2 = N.nearest(q, 0.25, exact=True)
    assert np.array_equal(idx, r2m.argmin(1)) and np.array_equal(r2, r2m.min(1))
    cnt, span, own = N.tie_stats(r2m)
    high, later = N.highest_index_wins(r2m), N.later_tile_wins(r2m)
    idx2 = N.nearest(q2, 0.25, exact=True)[0]
    print(f"n = {n}: ties {np.mean(cnt >= 2):.3f}, over >= 2 tiles {np.mean(span >= 2):.3f}, own tile and outside {np.mean(own):.3f}; "
          f"highest index changes {np.mean(high != idx):.3f}, later tile {np.mean(later != idx):.3f}; shift changes {np.mean(idx2 != idx):.3f}")
    assert np.mean(cnt >= 2) >= 0.90 and np.mean(span >= 2) >= 0.80
    # A tie mate lies in the body's own tile with probability 511 / (n - 1) under the random order: with the 4 to 5 mates of a
    # grid body that is 1 - (1 - 511 / (n - 1))^c = 0.68 ... 0.76 of the rows at 2 049 (5 tiles), 0.59 ... 0.67 at 2 561 (6) and
    # 0.38 ... 0.44 at 4 609 (10).  The tie tests on the device run at the first two sizes, where the floor is one half; the
    # third only fills the hit lists, and its floor keeps the same distance from what the order can give.
    assert np.mean(own) >= (0.50 if n < 4609 else 0.30)
    assert np.mean(high != idx) >= 0.90 and np.mean(later != idx) >= 0.80
    assert np.mean(idx2 != idx) >= 0.90, "a refresh that does nothing would not show"
    assert (idx >= 0).all() and (idx < n).all() and (idx != np.arange(n)).all()


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_lattice_specials(n):
    s, q, q2, k, r2m, r2m2 = dense(n)
    idx, r2 = N.nearest(q, 0.25, exact=True)
    assert q.min() >= 1 and q2.min() >= 1 and (q[:, 0] == 1).all() and r2[0] > 3.25 and 0 < idx[0] < n
    assert np.flatnonzero(idx == n - 1).tolist() == [N.DENSE_PARTNER] and idx[n - 1] == N.DENSE_PARTNER
    assert (r2m[n - 1] == r2[n - 1]).sum() == 1 and (r2m[N.DENSE_PARTNER] == r2[N.DENSE_PARTNER]).sum() == 1
    assert N.DENSE_PARTNER // N.TILE == 1 and (n - 1) // N.TILE == (n - 1) // 512 and (n - 1) % N.TILE < N.TILE - 1
    for a, b in N.DENSE_PAIRS + ((13, n - 2),):
        assert idx[a] == b and idx[b] == a and r2[a] == r2[b] == np.float32(0.25)
    assert N.DENSE_PAIRS[0][0] // 2 == N.DENSE_PAIRS[0][1] // 2 and N.DENSE_PAIRS[1][0] // N.TILE != N.DENSE_PAIRS[1][1] // N.TILE
    t = N.DENSE_TRIPLE
    assert len({b // N.TILE for b in t}) == 3 and (r2[list(t)] == np.float32(0.25)).all()
    assert idx[t[0]] == t[1] and idx[t[1]] == t[0] and idx[t[2]] == t[0]
    for b in N.DENSE_MASSLESS:
        assert s["m"][b] == 0.0 and (idx == b).any()
    assert (s["m"] == 0.0).sum() == 2 and s["m"].max() < 2.0 and s["m"][s["m"] > 0].min() >= 1.0
    # the shift: the same points held by other bodies, and velocities that carry every body there in one step of 2^-30
    assert np.array_equal(np.sort(q2.T.tolist(), 0), np.sort(q.T.tolist(), 0)) and np.array_equal(q + k, q2)
    v = np.stack([s[f] for f in ("vx", "vy", "vz")]).astype(np.float64)
    assert np.array_equal(v * 2.0 ** -30, k) and np.abs(v).max() <= 2.0 ** 35
    assert np.array_equal(np.stack([s[f] for f in ("qx", "qy", "qz")]).astype(np.int64), q)


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_lattice_chunked(n):
    """However the tiles are cut into chunks, the fold gives the brute force, before and after the shift."""
    s, q, q2, k, r2m, r2m2 = dense(n)
    tiles = -(-n // 1024) * 2
    for pos, m in ((q, r2m), (q2, r2m2)):
        idx, r2 = m.argmin(1).astype(np.int32), m.min(1)
        for chunks in (1, 2, 3, 4, 6, 8):
            got_idx, got_r2 = N.chunked(pos, 0.25, n, tiles, chunks)
            assert np.array_equal(got_idx, idx) and np.array_equal(got_r2.view(np.uint32), r2.view(np.uint32)), chunks

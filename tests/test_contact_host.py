"""CPU: contacts by radii from the Hermite sweeps (option "contact") and the contact stop.  The library, the binding and the
header carry the entry points; the numpy restatement (tests/helpers/contact_ref.py, written from include/murbhip.h) gives the
same answer however the j range is cut; murbhip.merge_contacts conserves what a merger conserves; the two contact kernels of a
fresh gfx950 build use no scratch, spill nothing and add only packed adds and fused multiply-adds to the plain sweep."""
import collections
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
import contact_ref as CR   # noqa: E402
import nearest_ref as N    # noqa: E402

E_INVALID = -2000
Q = ("qx", "qy", "qz")


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_contact_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_upload_radii", "murbhip_download_contact", "murbhip_contacts"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    for method in ("upload_radii", "contact", "contacts"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.contacts) and callable(mh.merge_contacts)
    for name in ("murbhost_sim_set_contact", "murbhost_sim_contacts"):
        assert hasattr(mh.host_lib(), name)
    # the argument checks that need no device: no context
    count, time = C.c_ulong(), C.c_double()
    radii = np.zeros(4, np.float32)
    assert mh.lib().murbhip_upload_radii(None, radii.ctypes.data_as(C.POINTER(C.c_float))) == E_INVALID
    assert mh.lib().murbhip_download_contact(None, None, None) == E_INVALID
    assert mh.lib().murbhip_contacts(None, None, None, None, 0, C.byref(count), C.byref(time)) == E_INVALID


@pytest.mark.parametrize("n", [2, 513, 2049, 3072])
def test_chunked_fold_equals_brute_force(n):
    """6 layout tiles cut into 1, 3 and 6 chunks: the lexicographic fold over the chunks is the brute-force answer on the
    lattice, whose radii give an exact touch with a tie, partners in other tiles and a large body that covers dozens."""
    s, soft, radii = CR.lattice(n)
    q = np.stack([s[k] for k in Q])
    idx, gap2 = CR.contact(q, radii, 0.25)
    assert (idx != np.arange(n)).all() and (idx >= 0).all() and (idx < n).all()
    if n >= 513:
        assert idx[5] == 400 and idx[400] == 5 and gap2[5] == -1.0 and gap2[400] == -1.0
        assert idx[7] == 8 and idx[8] == 7 and gap2[7] == 0.75 and gap2[8] == 0.75 and s["m"][7] == 0.0 and radii[7] == 0.0
        assert gap2[20] == 0.0 and gap2[21] == 0.0 and gap2[300] == 0.0 and idx[20] == 21 and not np.signbit(gap2[20])
        assert idx[30] == n - 1 and gap2[30] == -3.25 and N.nearest(q, 0.25, exact=True)[0][30] == 100
        assert idx[100] == n - 1 and gap2[100] == 5.75
        other = int((idx != N.nearest(q, 0.25, exact=True)[0]).sum())
        print(f"n = {n}: {other} bodies have a contact partner that is not their nearest neighbour, {(gap2 <= 0).sum()} touch")
        assert 26 <= other <= 200
    assert (gap2[idx] <= gap2).all()      # gap2 is symmetric: a body's partner has a partner at most as far
    for chunks in (1, 3, 6):
        got_idx, got_gap2 = CR.chunked(q, radii, 0.25, n, 6, chunks)
        assert np.array_equal(got_idx, idx) and np.array_equal(bits(got_gap2), bits(gap2)), chunks
    # all radii 0: the geometrically nearest body
    zero_idx, zero_gap2 = CR.contact(q, np.zeros(n, np.float32), 0.25)
    nn_idx, nn_r2 = N.nearest(q, 0.25, exact=True)
    assert np.array_equal(zero_idx, nn_idx) and np.array_equal(zero_gap2, nn_r2 - np.float32(0.25))
    # the fp64 form agrees on a lattice
    ok, err = CR.check_candidates(idx, gap2, q, radii, 0.25)
    assert ok and err == 0.0


def test_lone_body():
    idx, gap2 = CR.contact(np.zeros((3, 1)), np.float32([0.5]), 0.25)
    assert idx[0] == -1 and np.isinf(gap2[0]) and gap2[0] > 0
    idx, gap2 = CR.chunked(np.zeros((3, 1)), np.float32([0.5]), 0.25, 1, 2, 2)
    assert idx[0] == -1 and np.isinf(gap2[0])


def test_merge_contacts(mh):
    """A chain 3-9, 9-4 and a separate pair 6-1 merge into two bodies at places 3 and 1; mass, momentum, mass-weighted position
    and the sum of R^3 are conserved; survivors keep their order; an all-massless group takes the plain means."""
    rng = np.random.default_rng(5)
    n = 12
    s = {k: rng.standard_normal(n).astype(np.float32) * np.float32(1e9) for k in Q + ("vx", "vy", "vz")}
    s["m"] = rng.uniform(1e20, 2e20, n).astype(np.float32)
    radii = rng.uniform(1e7, 2e7, n).astype(np.float32)
    out, new_r, where = mh.merge_contacts(s, radii, [3, 9, 6], [9, 4, 1])
    assert len(new_r) == n - 3 and all(len(out[k]) == n - 3 for k in out)
    assert where.tolist() == [0, 1, 2, 3, 3, 4, 1, 5, 6, 3, 7, 8]
    m64 = s["m"].astype(np.float64)
    assert abs(out["m"].astype(np.float64).sum() - m64.sum()) <= 1e-6 * m64.sum()
    for k in Q + ("vx", "vy", "vz"):
        want = (m64 * s[k].astype(np.float64)).sum()
        got = (out["m"].astype(np.float64) * out[k].astype(np.float64)).sum()
        scale = (m64 * np.abs(s[k].astype(np.float64))).sum()
        assert abs(got - want) <= 1e-6 * scale, k
    r3 = (radii.astype(np.float64) ** 3).sum()
    assert abs((new_r.astype(np.float64) ** 3).sum() - r3) <= 1e-6 * r3
    for old in (0, 2, 5, 7, 8, 10, 11):      # untouched bodies: the same values, in the same order
        assert all(out[k][where[old]] == s[k][old] for k in s) and new_r[where[old]] == radii[old]
    assert out["m"][3] == np.float32(m64[[3, 4, 9]].sum()) and out["m"][1] == np.float32(m64[[1, 6]].sum())
    assert new_r[3] == np.float32(np.cbrt((radii[[3, 4, 9]].astype(np.float64) ** 3).sum()))
    # an all-massless group: the plain means
    s0 = {k: v.copy() for k, v in s.items()}
    s0["m"][[2, 5]] = 0.0
    out0, _, where0 = mh.merge_contacts(s0, radii, [5], [2])
    assert where0[5] == where0[2] == 2 and out0["m"][2] == 0.0
    for k in Q + ("vx", "vy", "vz"):
        assert out0[k][2] == np.float32((float(s[k][2]) + float(s[k][5])) / 2.0), k
    # no pairs: nothing changes
    same, same_r, ident = mh.merge_contacts(s, radii, [], [])
    assert ident.tolist() == list(range(n)) and all(np.array_equal(same[k], s[k]) for k in s) and np.array_equal(same_r, radii)


def test_contact_kernels_use_no_scratch():
    """Code-object metadata of a fresh gfx950 build (the method of test_nearest_host.py): both contact sweeps are there with 0
    bytes of scratch and 0 spilled registers and fit 4 waves per SIMD (at most 128 vector registers; 168 would need the sentence
    "3 waves per SIMD" in DESIGN.md 4.10).  Their reciprocal square roots are the plain sweep's, and their packed fp32
    instructions are the plain sweep's plus only v_pk_add_f32 and v_pk_fma_f32.

    LDS reads.  A tile is consumed in 4 lane steps of 4 records each (position A and B, velocity A and B): 16 records of 16
    bytes per lane.  The plain sweep uses two of the four lanes of the velocity B record {vz0, vz1, 0, 0}, so the compiler
    narrows those 4 reads to 8 bytes and pairs them (12 ds_read_b128 + 2 ds_read2st64_b64 as built today); the radii sit in the
    other two lanes, so the contact sweeps read that record whole.  The bound is the layout's: at most one LDS read
    instruction per record, 16, none of them beside the 16-byte reads, and no 16-byte read of the plain sweep missing.  (The
    plain sweep's own ds_read_b128 count, 12, is therefore NOT the contact sweeps': 4 reads are wider, none is added to the 16
    records.)"""
    hipcc = CO.hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed: no code object to inspect")
    seen = {}
    for name, num in CO.metadata(r"murb_contact_").items():
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0, name
        seen[re.search(r"(murb_[a-z_]+_kernel)", name).group(1)] = num["vgpr_count"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4.10"):] if "4.10" in design else ""
    for want in ("murb_contact_sweep_kernel", "murb_contact_active_sweep_kernel"):
        assert want in seen, want + " missing from the code object"
        assert seen[want] <= 128 or (seen[want] <= 168 and "3 waves per SIMD" in section), f"{want}: {seen[want]} vector registers"

    def counted(kernel, pattern):
        return collections.Counter(CO.ops(kernel, pattern))

    symbol = CO.symbol

    arith, lds = r"^\s*(v_pk_\w+|v_rsq_f32\w*)\b", r"^\s*(ds_read\w+)\b"
    plain, plain_lds = counted(symbol("murb_force_jerk_kernel"), arith), counted(symbol("murb_force_jerk_kernel"), lds)
    assert sum(plain.values()) > 100
    for want in ("murb_contact_sweep_kernel", "murb_contact_active_sweep_kernel"):
        got, got_lds = counted(symbol(want), arith), counted(symbol(want), lds)
        print(want, dict(got), dict(got_lds), "plain", dict(plain_lds))
        extra = got - plain
        assert not (plain - got), want + ": a packed instruction of the plain sweep is missing"
        assert set(extra) <= {"v_pk_add_f32", "v_pk_fma_f32"}, f"{want}: {dict(extra)}"
        assert sum(v for k, v in got.items() if k.startswith("v_rsq_f32")) == sum(v for k, v in plain.items() if k.startswith("v_rsq_f32"))
        records = 4 * 4      # lane steps of a tile x records of a lane step
        assert plain_lds["ds_read_b128"] <= got_lds["ds_read_b128"] <= records, f"{want}: {dict(got_lds)}, plain sweep {dict(plain_lds)}"
        assert sum(got_lds.values()) <= records, f"{want}: LDS reads {dict(got_lds)}: more than one per record"


# ------------------------------------------------------------------------------------------------------ the dense tie lattice
DENSE_N = (2049, 2561, 4609)


@lru_cache(maxsize=None)
def dense(n):
    """(q, q2, radii, gap2 matrix of q, of q2): conditions on the inputs of tests/test_tie_lattice_gpu.py, not measurements.
    Forming the matrices runs _exact_gap2's asserts on every pair: r2, e, s and gap2 are exact in fp32."""
    s, soft, q = CR.dense_lattice(n)
    q2, _ = CR.shifted(q)
    radii = CR.dense_radii(n)
    assert set(np.unique(radii)) <= {0.0, 0.5, 1.0, 1.5}
    return q, q2, radii, CR.gap2_matrix(q, radii, 0.25), CR.gap2_matrix(q2, radii, 0.25)


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_lattice_contacts(n):
    """Overlaps, exact touches and misses all occur, many rows are ties, most partners are not the nearest body, and the wrong
    tie rule changes the answer."""
    q, q2, radii, gm, gm2 = dense(n)
    idx, gap2 = CR.contact(q, radii, 0.25)
    assert np.array_equal(idx, gm.argmin(1)) and np.array_equal(bits(gap2), bits(gm.min(1))) and not np.signbit(gap2[gap2 == 0]).any()
    cnt, span, own = N.tie_stats(gm)
    high = N.highest_index_wins(gm)
    nn = N.nearest(q, 0.25, exact=True)[0]
    idx2 = CR.contact(q2, radii, 0.25)[0]
    frac = [float(np.mean(c)) for c in (gap2 < 0, gap2 == 0, gap2 > 0)]
    print(f"n = {n}: gap2 < 0 / == 0 / > 0: {frac[0]:.3f} / {frac[1]:.3f} / {frac[2]:.3f}; ties {np.mean(cnt >= 2):.3f} (over >= 2 "
          f"tiles {np.mean(span >= 2):.3f}); partner is not the nearest {np.mean(idx != nn):.3f}; highest index changes "
          f"{np.mean(high != idx):.3f}; shift changes {np.mean(idx2 != idx):.3f}")
    assert min(frac) >= 0.05
    assert np.mean(cnt >= 2) >= 0.20 and np.mean(idx != nn) >= 0.50 and np.mean(high != idx) >= 0.20
    assert np.mean(idx2 != idx) >= 0.90, "a refresh that does nothing would not show"
    assert (gap2[idx] <= gap2).all()
    for a, b in N.DENSE_PAIRS + ((13, n - 2),) + tuple(zip(N.DENSE_TRIPLE, N.DENSE_TRIPLE[1:])):      # on one point: e = 0
        assert gm[a, b] == -np.float32(radii[a] + radii[b]) ** 2


@pytest.mark.parametrize("n", DENSE_N)
def test_dense_lattice_chunked(n):
    q, q2, radii, gm, gm2 = dense(n)
    tiles = -(-n // 1024) * 2
    for pos, m in ((q, gm), (q2, gm2)):
        idx, gap2 = m.argmin(1).astype(np.int32), m.min(1)
        for chunks in (1, 2, 3, 4, 6, 8):
            got_idx, got_gap2 = CR.chunked(pos, radii, 0.25, n, tiles, chunks)
            assert np.array_equal(got_idx, idx) and np.array_equal(bits(got_gap2), bits(gap2)), chunks

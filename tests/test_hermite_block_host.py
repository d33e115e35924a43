"""CPU: individual block time steps of the Hermite integrator (murbhip_evolve_block).  The numpy restatement of the scheme
(tests/helpers/hermite_block_ref.py, written from include/murbhip.h) does on a binary inside a cluster what block steps are
for, its level rule has the edges the header states, a run keeps the tick invariants; the library, the binding and the
header carry the entry points, and the new kernels of a fresh gfx950 build use no scratch."""
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
import code_object as CO           # noqa: E402
import hermite_adaptive_ref as A   # noqa: E402
import hermite_block_ref as B      # noqa: E402

ETA, ETA_START, BLOCKS = 0.02, 0.01, 4


@lru_cache(maxsize=None)
def shared_run(n):
    """(steps, relative energy error) of the shared adaptive scheme over 2 binary periods, dt_max = period / 2."""
    s, period = B.cluster(n)
    e0 = A.energy(s, B.SOFT)
    out, dts, t, _ = A.evolve(s, 2.0 * period, B.SOFT, eta=ETA, eta_start=ETA_START, dt_max=period / 2.0)
    assert t == 2.0 * period
    return len(dts), abs(A.energy(out, B.SOFT) - e0) / abs(e0)


@lru_cache(maxsize=None)
def block_run(n, kmax):
    """(Run, relative energy error) of 4 blocks of period / 2; the tick invariants are checked after every block step."""
    s, period = B.cluster(n)
    e0 = A.energy(s, B.SOFT)

    def invariants(r, act):
        step = r.T >> r.levels.astype(np.int64)
        assert (r.ticks % step == 0).all(), "a body's time is no multiple of its step"
        assert (r.ticks < r.T).all() and (r.levels >= 0).all() and (r.levels <= r.kmax).all()
        if r.clock == 0:
            assert act.all() and (r.ticks == 0).all(), "not every body was active at the block boundary"

    r = B.Run(s, B.SOFT, period / 2.0, kmax=kmax, eta=ETA, eta_start=ETA_START).run(BLOCKS, check=invariants)
    assert r.clock == 0 and r.ticks_done == BLOCKS * r.T
    return r, abs(A.energy(r.state(), B.SOFT) - e0) / abs(e0)


@pytest.mark.parametrize("n,ratio", [(32, 5), (256, 20)])
def test_block_steps_on_a_binary_in_a_cluster(n, ratio):
    """hermite_adaptive_ref.binary(0.9) with n - 2 field bodies of 1e26 kg on circular orbits at 2e12 ... 8e12 m, softening
    1e6 m, 2 binary periods in 4 blocks of period / 2, eta 0.02, eta_start 0.01, kmax 12: no step is clamped, the energy error at
    the synchronised end is at most the shared scheme's, and the body-steps are at most 1/5 (n = 32) and 1/20 (n = 256) of
    the shared scheme's.  Measured: n = 32: shared 341 steps = 10 912 body-steps, error 6.5e-5; block 483 block steps, 1 176
    body-steps (1/9.3), error 2.5e-5.  n = 256: shared 340 steps = 87 040, 4.9e-5; block 483, 2 724 (1/32), 1.4e-5."""
    steps, err_shared = shared_run(n)
    r, err = block_run(n, 12)
    print(f"n = {n}: shared {steps} steps = {steps * n} body-steps, error {err_shared:.3e}; block {r.steps} block steps, "
          f"{r.body_steps} body-steps, largest active set {r.max_active}, levels {r.k_lo} ... {r.k_hi}, error {err:.3e}")
    assert r.clamped == 0
    assert err <= err_shared
    assert r.body_steps * ratio <= steps * n
    assert r.max_active == n and r.k_lo == 0 and r.time() == BLOCKS * float(np.float32(B.cluster(n)[1] / 2.0))


def test_a_cap_too_coarse_is_reported():
    """kmax 8 on the same system (n = 256): the pericentre passages ask for less than dt_max / 256, the steps taken there count
    as clamped (measured 170 of 330) and the energy error shows it (0.13)."""
    r, err = block_run(256, 8)
    print(f"kmax 8: {r.steps} block steps, {r.clamped} clamped, error {err:.3e}")
    assert r.clamped > 0 and r.k_hi == 8
    assert err > 100.0 * block_run(256, 12)[1]


def test_level_rule_edges():
    dt_max, kmax = np.float32(4096.0), 4     # levels 4096, 2048, 1024, 512, 256
    assert B.k_req(np.float32(np.inf), dt_max, kmax) == (0, False)
    assert B.k_req(np.float32(5000.0), dt_max, kmax) == (0, False)
    assert B.k_req(np.float32(4096.0), dt_max, kmax) == (0, False)          # exactly on a level: that level
    assert B.k_req(np.nextafter(np.float32(4096.0), np.float32(0.0)), dt_max, kmax) == (1, False)
    assert B.k_req(np.float32(1024.0), dt_max, kmax) == (2, False)
    assert B.k_req(np.float32(300.0), dt_max, kmax) == (4, False)
    assert B.k_req(np.float32(256.0), dt_max, kmax) == (4, False)           # the cap itself still qualifies
    assert B.k_req(np.float32(255.0), dt_max, kmax) == (4, True)            # below the cap: clamped
    assert B.k_req(np.float32(1.0), np.float32(1.0), 0) == (0, False) and B.k_req(np.float32(0.5), np.float32(1.0), 0) == (0, True)
    T = 1 << kmax
    # several halvings at once
    assert B.new_level(1, 4, 8, kmax) == 4
    # a doubling needs the coarser grid to have a point at t_next: level 3 has steps of 2 ticks, level 2 of 4
    assert B.new_level(3, 0, 6, kmax) == 3          # 6 is no multiple of 4: refused
    assert B.new_level(3, 0, 8, kmax) == 2          # allowed, and one level only
    assert B.new_level(3, 2, 4, kmax) == 2
    assert B.new_level(3, 3, 4, kmax) == 3
    assert B.new_level(1, 0, T, kmax) == 0 and B.new_level(1, 0, T // 2, kmax) == 1
    assert B.new_level(0, 0, T, kmax) == 0
    # the criterion's +inf (a lone body: 0 / 0) starts at level 0
    z = np.zeros((3, 1))
    assert B.start_levels(z, z, 0.01, dt_max, kmax)[0] == 0
    # seconds are exact products of ticks
    assert B.tick_seconds(np.float32(3600.0), 12) * 4096 == 3600.0 and B.level_dt(3600.0, 3) == np.float32(450.0)


def test_next_time_and_active_set():
    kmax = 3
    ticks, levels = np.array([0, 0, 4, 6, 7]), np.array([0, 1, 2, 3, 3])
    t, act = B.next_time(ticks, levels, kmax)     # 8, 4, 6, 7, 8
    assert t == 4 and act.tolist() == [False, True, False, False, False]
    t, act = B.next_time(np.array([0, 4, 6, 7, 7]), np.array([0, 1, 2, 3, 3]), kmax)
    assert t == 8 and act.all()


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


def test_block_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_evolve_block", "murbhip_block_state", "murbhip_block_set_levels"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    for method in ("evolve_block", "block_state", "set_block_levels"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.block_counts) and hasattr(mh.host_lib(), "murbhost_sim_block_counts")
    # the argument checks that need no device: no context
    out = (C.c_double * 8)()
    assert mh.lib().murbhip_evolve_block(None, 1.0, 1, 0.02, 0.01, 12, 1, out) == -2000
    assert mh.lib().murbhip_block_state(None, None, None) == -2000
    assert mh.lib().murbhip_block_set_levels(None, None, 0) == -2000


def test_block_kernels_use_no_scratch():
    """Code-object metadata of a fresh gfx950 build: the eight kernels of a block step are there, with 0 bytes of scratch and
    0 spilled registers; the active sweep has the fixed-step sweep's LDS and arithmetic and fits 5 waves per SIMD (at most
    96 vector registers: 512 / 5 rounded down to the allocation unit of 8).  The two potential kernels, likewise free of
    scratch and spills, fit 4 waves per SIMD (128 vector registers)."""
    hipcc = CO.hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed: no code object to inspect")
    kernels = CO.metadata(r"murb_block_|murb_force_jerk_block_|murb_force_jerk_pot_")
    for want in ("murb_block_begin_kernel", "murb_block_start_kernel", "murb_block_min_kernel", "murb_block_predict_kernel",
                 "murb_block_plan_kernel", "murb_force_jerk_block_kernel", "murb_block_correct_kernel", "murb_block_book_kernel",
                 "murb_force_jerk_pot_kernel", "murb_force_jerk_pot_block_kernel"):
        assert any(want in k for k in kernels), want + " missing from the code object"
    for name, num in kernels.items():
        print(name, num)
        assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0, name
        if "murb_force_jerk_block_kernel" in name:
            assert num["vgpr_count"] <= 96, "the active sweep no longer fits 5 waves per SIMD"
        if "murb_force_jerk_pot_" in name:      # the potential forms, fixed and active (per-body multipliers): 4 waves per SIMD
            assert num["vgpr_count"] <= 128, name + " no longer fits 4 waves per SIMD"

    def packed(kernel):   # the packed fp32 instructions, reciprocal square roots and LDS reads of a kernel's body
        return sorted(CO.ops(kernel, r"^\s*(v_pk_\w+|v_rsq_f32\w*|ds_read_b128)\b"))

    fixed, block = "murb_force_jerk_kernel", "murb_force_jerk_block_kernel"
    assert packed(fixed) == packed(block) and len(packed(fixed)) > 100


# ------------------------------------------------------------------------------- the shapes tests/test_block_wrap_gpu.py relies on
def test_wrap_case_shapes(mh):
    """Every (n, active count, "block_units") of tests/test_block_wrap_gpu.py: the rows the sweep writes fit ensure_block's
    buffer (slots + 16 U), and on 256 CUs the cases hold units equal to the plain grid exactly, two passes, and at least 3 passes
    of the plain grid with 4 of the option forms' grid."""
    import block_wrap as W
    for n in W.CUTS:
        assert W.slots_of(n) == mh.slice_slots(n, 1), n
    assert (W.GRID_PLAIN, W.GRID_OPTION) == (1280, 1024)
    seen = []
    for n, active, units in W.cases():
        slots = W.slots_of(n)
        groups, chunks, walked = W.plan(active, units, slots // W.TILE)
        assert 1 <= chunks <= slots // W.TILE and walked == groups * chunks
        assert W.GROUP * walked <= slots + W.GROUP * units, (n, active, units, walked)
        seen.append((n, active, units, walked, W.passes(walked, W.GRID_PLAIN), W.passes(walked, W.GRID_OPTION)))
    for line in sorted(set(x for x in seen if x[1] >= x[0] // 2)):
        print("n=%d active=%d U=%d: %d units, %d passes of 1280, %d of 1024" % line)
    walked = [x[3] for x in seen]
    assert W.GRID_PLAIN in walked, "no case fills the plain grid exactly"
    assert any(x[4] == 2 for x in seen) and any(x[5] == 2 for x in seen)
    assert any(x[4] >= 3 and x[5] >= 4 for x in seen if x[0] == W.MAIN)
    deep = max(x[3] for x in seen if x[0] == W.DEEP)
    assert deep == 577 * 20 == 11540 and W.passes(deep, W.GRID_PLAIN) == 10 and W.passes(deep, W.GRID_OPTION) == 12
    # the cut of 10 tiles into 7 chunks, and the small sets stay inside one pass of either grid
    assert W.cut(10, 7) == [1, 1, 2, 1, 2, 1, 2] and W.cut(10, 4) == [2, 3, 2, 3] and W.cut(10, 10) == [1] * 10
    for n in W.CUTS:
        d = W.depth_set(n)
        assert 64 <= len(d) <= 72 and 4 <= -(-len(d) // W.GROUP) <= 5
        assert -(-len(d) // W.GROUP) * (W.slots_of(n) // W.TILE) <= W.GRID_OPTION


def test_tightest_row_sizing():
    """n = 5 120 (10 tiles, no padding, 320 groups) with U = 320 x 9 + 1 = 2 881: 10 chunks, 51 200 row entries written of
    51 216 allocated.  One unit less and the plan gives 9 chunks."""
    import block_wrap as W
    assert W.TIGHT_U == 2881 and W.slots_of(W.MAIN) == 5120
    groups, chunks, walked = W.plan(W.MAIN, W.TIGHT_U, 10)
    assert (groups, chunks, walked) == (320, 10, 3200)
    assert W.GROUP * walked == 51200 and W.slots_of(W.MAIN) + W.GROUP * W.TIGHT_U == 51216
    assert W.plan(W.MAIN, W.TIGHT_U - 1, 10)[1] == 9
    # no (active, U) at all can pass the buffer: units <= max(U + groups - 1, groups) and 16 groups <= slots
    for n in (W.MAIN, W.PADDED, W.DEEP, 17, 1024, 1025):
        slots = W.slots_of(n)
        for active in (1, 15, 16, 17, n // 2, n - 1, n):
            for units in (1, 2, 15, 16, 17, 1279, 1280, 1281, W.TIGHT_U, 65536):
                walked = W.plan(active, units, slots // W.TILE)[2]
                assert W.GROUP * walked <= slots + W.GROUP * units, (n, active, units)


def test_phi_lane_sums_depend_on_the_tile_order():
    """numpy float32 emulation of a wave's phi sums on the dense system of tests/test_potential_gpu.py (n = 2 049, 5 tiles that
    hold bodies): "tiles 1, 2, 3, 4, then the own tile 0" (a wave whose bodies all lie in tile 0) against "tile 4, then 0, 1, 2,
    3" (a wave with one body each in tiles 0 ... 3: all four masked in the loop and added behind it).  The folded totals differ
    for several probe bodies: a sweep whose mask is per wave gives a body's phi other bits in other company."""
    import potential_ref as PR
    s, soft = PR.dense()
    probes = PR.dense_probes(64)
    assert len(probes) == 64 and (probes < PR.TILE).all()
    lanes = folded = 0
    for b in probes:
        acc_a, tot_a = PR.lane_sums_f32(s, soft, int(b), (1, 2, 3, 4, 0))
        acc_b, tot_b = PR.lane_sums_f32(s, soft, int(b), (4, 0, 1, 2, 3))
        lanes += int(not np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32)))
        folded += int(np.float32(tot_a).view(np.uint32) != np.float32(tot_b).view(np.uint32))
        want = PR.phi_of(s, soft, rows=[int(b)])[0]
        assert abs(float(tot_a) - want) <= PR.TOL_F64_MAX * want and abs(float(tot_b) - want) <= PR.TOL_F64_MAX * want
    print(f"{lanes} of {len(probes)} probe bodies differ in a lane accumulator, {folded} in the folded total")
    assert folded >= 4

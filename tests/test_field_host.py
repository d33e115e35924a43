"""CPU: the yardstick of the field read-out (tests/helpers/field_ref.py) against the yardsticks of the sweeps, the planning
behind murbfield_layout, the launch cut of csrc/murb_field.h under g++ alone and under the sanitizers, the new entry points of the built libraries and the Python interface, the sweep kernel's code
object, and why a skipped body must never enter an fp32 sum."""
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
import hermite_ref as H       # noqa: E402
import potential_ref as PR    # noqa: E402

E_INVALID = -2000
G = float(H.G)


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("n", [1, 2, 63, 513])
def test_field_at_the_bodies_is_the_sweeps(n):
    """At the bodies' own state with every body skipping itself, the field is the Hermite sweep's (a, j) and the "potential"
    option's phi: the three fp64 yardsticks agree to 1e-12 of the sums of the terms' magnitudes."""
    s = F.system(n)
    p, v, skip = F.body_points(s, np.arange(n))
    a, j, phi, ab = F.field_f64(p, v, skip, s, F.SOFT)
    ha, hj, habs = H.acc_jerk_f64(s, F.SOFT, want_abs=True)
    hphi = PR.phi_of(s, F.SOFT)
    tiny = np.finfo(np.float64).tiny
    assert (np.abs(a - ha).max(0) <= 1e-12 * np.maximum(ab["a"], tiny)).all()
    assert (np.abs(j - hj).max(0) <= 1e-12 * np.maximum(ab["j"], tiny)).all()
    assert np.allclose(ab["j"], habs, rtol=1e-12, atol=0.0)
    assert (np.abs(phi - hphi) <= 1e-12 * np.maximum(hphi, tiny)).all() and np.array_equal(ab["phi"], phi)
    if n == 1:
        assert not a.any() and not j.any() and phi[0] == 0.0 and not np.signbit(phi[0])


def test_known_answers():
    """One body of G m = 1 at the origin at rest, soft 0: a point at (2, 0, 0) moving with (0, 1, 0) sees a = (-1/4, 0, 0),
    j = -v / r^3 (d.w = 0) = (0, -1/8, 0) and phi = 1/2; with the body skipped, nothing; a second body on the first counts."""
    m = 1.0 / G
    s = PR.state([[0.0], [0.0], [0.0]], [m])
    p, v = np.array([[2.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]])
    a, j, phi, ab = F.field_f64(p, v, None, s, 0.0)
    assert np.allclose(a[:, 0], [-0.25, 0, 0], rtol=1e-6) and np.allclose(j[:, 0], [0, -0.125, 0], rtol=1e-6) and np.isclose(phi[0], 0.5, rtol=1e-6)
    a, j, phi, ab = F.field_f64(p, v, [0], s, 0.0)
    assert not a.any() and not j.any() and phi[0] == 0.0 and ab["a"][0] == 0.0
    two = PR.state([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [m, m])
    a, j, phi, ab = F.field_f64(p, v, [0], two, 0.0)
    assert np.allclose(a[:, 0], [-0.25, 0, 0], rtol=1e-6) and np.isclose(phi[0], 0.5, rtol=1e-6)
    # the radial part of the jerk: a point moving outwards with speed 1 has d.w = -r for a body at rest: j = w/r^3 - 3 (d.w) d / r^5
    a, j, phi, ab = F.field_f64(p, np.array([[1.0], [0.0], [0.0]]), None, s, 0.0)
    assert np.allclose(j[:, 0], [-1.0 / 8.0 + 3.0 * 2.0 * 2.0 / 32.0, 0, 0], rtol=1e-6)


def test_float32_emulation_and_bound():
    """The float32 emulation attains a few 2^-24 on the dense system, for all three quantities, and far points cancel worse than
    bodies: the bound follows the inputs."""
    s = F.system(513)
    for name, (p, v, skip) in (("bodies", F.body_points(s, np.arange(33))), ("midpoints", F.midpoints(s, 33)), ("far", F.far_points(33))):
        ref, c = F.bound_of(p, v, skip, s, F.SOFT)
        print(name, {k: round(x, 2) for k, x in c.items()})
        assert all(0.0 < c[k] < 200.0 for k in c), (name, c)
        assert F.check(F.field_f32(p, v, skip, s, F.SOFT), ref, c, name)      # a quarter of the bound by construction
        wrong = F.field_f64(p, v, None if skip is not None else np.zeros(33, np.int64), s, F.SOFT)[:3]      # one body's term off
        e = F.scaled_errors(wrong, ref)
        assert max(e[k].max() for k in e) > 100 * max(c.values()) * F.U24


def test_sparse_probe_has_power():
    """With every source alone massive a point's sum IS that source's term; with all 16 the smallest source term is 10 x the
    bound of the point's sums at every point: a dropped or doubled j slot shows."""
    s, soft, src = F.sparse_sources()
    assert tuple(src) == PR.SPARSE_SOURCES and {int(x) % F.TILE for x in src} >= {0, 511}
    p, v, skip = F.midpoints(s, 64, stride=11)
    ref, c = F.bound_of(p, v, skip, s, soft)
    q = H._stack(s, F.Q)
    gm = H._gm(s)[src]
    d = q[:, None, src] - p.astype(np.float64)[:, :, None]
    r2 = (d ** 2).sum(0) + float(soft) ** 2
    tphi, ta = gm / np.sqrt(r2), gm / r2 ** 1.5 * np.sqrt((d ** 2).sum(0))
    share_phi, share_a = tphi.min(1) / ref[3]["phi"], ta.min(1) / ref[3]["a"]
    need = F.POWER_FACTOR * max(c.values()) * F.U24
    print(f"sparse probe: smallest share phi {share_phi.min():.2e}, a {share_a.min():.2e}; needs {need:.1e}")
    assert (share_phi >= need).all() and (share_a >= need).all()
    one = F.only_source(s, src[3])
    assert np.flatnonzero(one["m"]).tolist() == [src[3]]
    r1 = F.field_f64(p, v, skip, one, soft)
    assert np.allclose(r1[2], tphi[:, 3], rtol=1e-12)


def test_skipped_body_must_never_enter_the_sum():
    """potential_ref.own_term_pair: the own term G m / soft is 1e4 x the pair term.  A float32 sum that took the skipped body's term
    and gave it back has lost the pair term's low 13 bits — 1e-4 of it, fifty times what DESIGN.md §4.11 allows phi — where the
    sum that never held it is exact to fp32."""
    s, soft, (a, b) = PR.own_term_pair(2)
    f = np.float32
    pair, own = f(G * PR.OWN_MASS / np.sqrt(PR.OWN_SEP ** 2 + float(soft) ** 2)), f(G * PR.OWN_MASS / float(soft))
    there_and_back = (own + pair) - own
    lost = abs(float(there_and_back) - float(pair)) / float(pair)
    p, v, skip = F.body_points(s, [a])
    by_index = F.field_f32(p, v, skip, s, soft)[2][0]
    kept = abs(float(by_index) - float(pair)) / float(pair)
    print(f"own / pair = {float(own) / float(pair):.3e}: through the sum {lost:.2e}, by index {kept:.2e}")
    assert lost > 10 * PR.TOL_F64_MAX and kept <= 2.0 ** -23
    assert F.field_f32(p, v, None, s, soft)[2][0] == own + pair        # without a skip entry the own term counts


# ------------------------------------------------------------------------------------------------------------------ planning
@pytest.mark.parametrize("n", [1, 512, 513, 1025, 2049, 30000])
@pytest.mark.parametrize("option", [0, 1, 2, 7, 10 ** 6])
def test_field_layout(mh, n, option):
    tiles = -(-n // 512)
    base = mh.field_layout(n, chunks=option)
    k = base["chunks"]
    assert 1 <= k <= tiles and base["tiles"] == tiles
    assert k == (min(tiles, option) if option else min(16, max(1, tiles // 8)))      # the default: chunks of 8 tiles or more
    flat = [t for lo, hi in base["ranges"] for t in range(lo, hi)]
    assert flat == list(range(tiles)), "the chunks cover every tile once, in order"
    assert all(hi > lo for lo, hi in base["ranges"])
    for batch in (0, 16, 32, 4096):
        per = batch if batch else 16384
        for count in (0, 1, 16, 17, 33, per, per + 1, 10 ** 6):
            lay = mh.field_layout(n, chunks=option, batch=batch, count=count)
            assert lay["chunks"] == k and lay["ranges"] == base["ranges"], "the chunk cut is no function of the count or the batch"
            assert lay["groups"] * 16 == per and lay["rows"] >= per * k
            assert lay["batches"] == -(-count // per)


def test_field_layout_refusals(mh):
    out = (C.c_ulong * 4)()
    L = mh.lib()
    assert L.murbfield_layout(0, 0, 0, out) == E_INVALID
    assert L.murbfield_layout(100, 0, 0, None) == E_INVALID
    assert L.murbfield_layout(100, -1, 0, out) == E_INVALID
    for batch in (-16, 8, 17, (1 << 20) + 16):
        assert L.murbfield_layout(100, 0, batch, out) == E_INVALID, batch
    assert L.murbfield_layout(100, 0, 1 << 20, out) == 0


# ---------------------------------------------------------------------------------- the launch cut, a stand-alone program
CSRC = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc")

CUT_PROGRAM = r"""
#include <cstdio>
#include "murb_field.h"
static bool same(const MurbFieldCut& k, int chunks, int tiles_each, int tiles_more, long grid)
{
    return k.chunks == chunks && k.tiles_each == tiles_each && k.tiles_more == tiles_more && k.grid == grid;
}
int main() {
    const unsigned long bodies[] = {1, 2, 511, 513, 2049, 4096, 65536, 200000, 1000000, 4000000};
    const long chunk_options[] = {0, 1, 2, 3, 7, 16, 61, 500, 7813};
    const long grids[] = {1, 4, 64, 416, 1024, 1216};
    const unsigned long paddeds[] = {16, 32, 1008, 4096, 16384, 1ul << 20};   // ascending
    unsigned long cases = 0, cut_less = 0, uncut = 0;
    for (const unsigned long n : bodies)
        for (const long co : chunk_options)
            for (const long grid_full : grids) {
                if (!murb_field_options_valid(co, 0)) return 2;
                const MurbFieldLayout l = murb_field_layout(n, co, 0);
                if (l.chunks < 1 || l.chunks > l.tiles) return 3;
                int before = l.chunks;
                for (const unsigned long padded : paddeds) {
                    if (murb_field_padded(padded) != padded || murb_field_padded(padded - 15) != padded || murb_field_padded(padded + 1) != padded + 16)
                        return 4;
                    for (const bool fill : {false, true}) {
                        const MurbFieldCut k = murb_field_cut(l, padded, grid_full, fill);
                        ++cases;
                        if (k.chunks < 1 || k.chunks > l.chunks) return 10;
                        if (k.tiles_each < 1) return 11;
                        if (k.tiles_more < 0 || k.tiles_more >= k.chunks) return 12;
                        if (k.tiles_each * k.chunks + k.tiles_more != l.tiles) return 13;
                        if (k.grid < 1 || k.grid > grid_full) return 14;
                        if (k.grid > (long)k.groups * k.chunks) return 15;
                        if ((unsigned long)k.groups * 16 != padded) return 16;
                        if (!fill) {
                            if (k.chunks != l.chunks) return 20;   // a sum's bits do not depend on how many points were asked for
                            continue;
                        }
                        if (k.chunks > before) return 21;          // non-increasing in padded
                        before = k.chunks;
                        if (k.groups >= grid_full && k.chunks != 1) return 22;
                        const long most = (long)k.groups * l.chunks;
                        if ((long)k.groups * k.chunks < (grid_full < most ? grid_full : most)) return 23;   // fills the grid where the layout allows
                        cut_less += k.chunks < l.chunks;
                        uncut += k.chunks == 1 && l.chunks > 1;
                    }
                }
            }
    std::printf("%lu %lu %lu", cases, cut_less, uncut);
    // known answers: tiles of 512 bodies, 256 CUs x 4 workgroups
    const MurbFieldLayout five = murb_field_layout(2049, 3, 0), many = murb_field_layout(200000, 0, 0);
    std::printf(" %d %d %d %d", five.tiles, five.chunks, many.tiles, many.chunks);
    std::printf(" %d", (int)same(murb_field_cut(five, 16, 1024, true), 3, 1, 2, 3));
    std::printf(" %d", (int)same(murb_field_cut(five, 16384, 1024, true), 1, 5, 0, 1024));
    std::printf(" %d", (int)same(murb_field_cut(many, 4096, 1024, true), 4, 97, 3, 1024));
    std::printf(" %d\n", (int)same(murb_field_cut(many, 4096, 1024, false), 16, 24, 7, 1024));
    return 0;
}
"""


def build_and_run_cut(tmp_path, flags):
    src, exe = tmp_path / "cut.cpp", tmp_path / "cut"
    src.write_text(CUT_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr)
    return done.stdout.split()


def check_cut_program(out):
    cases, cut_less, uncut = (int(v) for v in out[:3])
    print("cuts", cases, "fill mode below the layout's chunks", cut_less, "not cut at all", uncut)
    assert cases == 10 * 9 * 6 * 6 * 2 and cut_less > 0 and uncut > 0
    assert out[3:7] == ["5", "3", "391", "16"], "the layouts of the known answers"
    assert out[7:] == ["1", "1", "1", "1"], "the known answers"


def test_launch_cut(tmp_path):
    """csrc/murb_field.h is plain C++: g++ compiles it on the CPU with every warning an error.  murb_field_cut over body counts
    up to 4 000 000, chunk options up to the tile count, grids from 1 to 1216 workgroups and launches from one group to 2^20
    points: in both modes the chunks cover every tile once (tiles_each * chunks + tiles_more == tiles, tiles_each >= 1), lie in
    [1, the layout's], and the grid in [1, min(grid_full, groups * chunks)]; the fixed mode keeps the layout's chunks whatever the
    launch holds; the fill mode's chunks never grow with the launch, are 1 once the groups fill the grid, and fill the grid
    wherever the layout allows.  Four known answers."""
    check_cut_program(build_and_run_cut(tmp_path, []))


def test_launch_cut_under_sanitizers(tmp_path):
    """The same stand-alone program, with its own main, built with -fsanitize=address,undefined and run directly: no report, the
    same answers."""
    check_cut_program(build_and_run_cut(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


# -------------------------------------------------------------------------------------------------------------- entry points
def test_field_entry_points_are_exported(mh):
    """include/murbfield.h, the binding's list and the library's exports name the same entry points; the options are documented
    where they are set; the interface of include/murbhip.h is what it was."""
    header = open(os.path.join(ROOT, "include", "murbfield.h")).read()
    declared = sorted(re.findall(r"^int (murbfield_\w+)\(", header, re.M))
    assert declared == sorted(mh.FIELD_EXPORTS) and len(declared) == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbfield_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    for name in declared:
        assert hasattr(mh.lib(), name)
    for key in mh.FIELD_OPTIONS:
        assert re.search(r'^ \*   "%s" ' % key, header, re.M), key
    assert not set(mh.FIELD_EXPORTS) & set(mh.EXPORTS)
    # the argument checks that need no device: no context
    v = C.c_long()
    assert mh.lib().murbfield_at(None, 0, *([None] * 14)) == E_INVALID
    assert mh.lib().murbfield_of(None, 0, *([None] * 8)) == E_INVALID
    assert mh.lib().murbfield_set_option(None, b"field_chunks", 1) == E_INVALID
    assert mh.lib().murbfield_get_option(None, b"field_chunks", C.byref(v)) == E_INVALID


def test_python_interface_has_the_methods(mh):
    for method in ("field_at", "field_of"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.field_at) and callable(mh.field_layout)
    assert hasattr(mh.host_lib(), "murbhost_sim_field_at")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint fieldAt\(", hpp)


# --------------------------------------------------------------------------------------------------------------- code object
def test_field_kernel_uses_no_scratch():
    """Code-object metadata of a fresh gfx950 build (the method of test_nearest_host.py): murb_force_field_kernel is there with 0
    bytes of scratch and 0 spilled registers and fits 4 waves per SIMD (at most 128 vector registers); its inner loop is the
    plain sweep's packed arithmetic plus one packed multiply (the mask) and one packed add (phi) per pair of interactions."""
    hipcc = CO.hipcc()
    assert hipcc, "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_force_field_kernel")
    assert len(kernels) == 1, "murb_force_field_kernel missing from the code object"
    (name, num), = kernels.items()
    print(name, num)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128, "no longer fits 4 waves per SIMD"

    def counts(kernel):
        ops = [re.sub(r"_e(32|64)$", "", op) for op in CO.ops(kernel, r"^\s*(v_pk_\w+|v_rsq_f32\w*)\b")]
        return {k: ops.count(k) for k in set(ops)}, CO.body(kernel)

    plain, _ = counts("murb_force_jerk_kernel")
    mine, body = counts(name)
    print("plain sweep", plain, "field sweep", mine)
    pairs = plain["v_rsq_f32"] // 2          # pairs of interactions of the unrolled tile: 4 lane steps x 4 points
    assert pairs == 16
    # the loop's copy, and four copies of one pair of interactions behind it (one per point: the tile of its skipped slot)
    assert mine["v_rsq_f32"] == 2 * (pairs + 4)
    # per pair of interactions the sweep's own packed arithmetic (its multiplies and fused multiply-adds all lie in its loop, and
    # six packed subtractions), one packed instruction for the mask and one for phi; the folds add 10 packed additions per point
    per_pair = (plain["v_pk_mul_f32"] + plain["v_pk_fma_f32"]) // pairs + 6
    assert per_pair == 26
    total = mine["v_pk_fma_f32"] + mine["v_pk_mul_f32"] + mine["v_pk_add_f32"]
    assert total <= (per_pair + 2) * (pairs + 4) + 4 * 10, "more than one packed instruction each for the mask and phi beside the sweep's"
    assert not re.search(r"\bscratch_|\bbuffer_", body)


# ------------------------------------------------------------------------------------------- the walk beyond one grid pass
import field_wrap as FW      # noqa: E402

CASE_NAMES = ("A", "B", "C", "D", "E")


def test_wrap_helper_plans_like_the_library(mh):
    """field_wrap's chunk count, chunk cut and launches are murbfield_layout's, for every case and both grids."""
    for grid in (FW.GRID, FW.SMALL_GRID):
        for name, case in FW.cases(grid).items():
            lay = mh.field_layout(case.n, chunks=case.chunks_option, batch=case.batch, count=case.count)
            assert lay["chunks"] == case.chunks and lay["ranges"] == FW.cut(case.n, case.chunks), name
            assert lay["batches"] == len(FW.launches(case.count, case.batch)) and lay["groups"] * 16 == (case.batch or FW.BATCH_DEFAULT), name
            assert lay["rows"] >= max(g for _, _, g in FW.launches(case.count, case.batch)) * 16 * case.chunks, name


def test_wrap_walk_visits_every_unit_once():
    """unit_of over every workgroup and every k is each (group, chunk) once; a workgroup has no unit behind its first missing one."""
    for groups, chunks, grid in ((3, 3, 1024), (7, 5, 8), (622, 5, 1024), (2, 2, 4), (5, 1, 2)):
        units, blocks, passes = FW.walk(groups, chunks, grid)
        seen = [FW.unit_of(b, k, groups, chunks, grid) for b in range(grid) for k in range(passes + 1)]
        got = sorted(x for x in seen if x is not None)
        assert got == sorted((g, c) for c in range(chunks) for g in range(groups)), (groups, chunks, grid)
        assert blocks == min(units, grid) and passes == -(-units // grid) and FW.unit_of(0, passes, groups, chunks, grid) is None
        late = FW.late_units(groups, chunks, grid)
        assert late.sum() == units - blocks and all(late[c, g] == (k > 0) for b in range(blocks) for k in range(passes)
                                                    for g, c in [FW.unit_of(b, k, groups, chunks, grid) or (None, None)] if g is not None)


@pytest.mark.parametrize("grid", [FW.GRID, FW.SMALL_GRID])
def test_wrap_cases_make_their_passes(grid):
    """On 256 CUs (1 024 workgroups) and on a chip of 64, every case of tests/test_field_wrap_gpu.py makes the passes it claims,
    a workgroup's second unit is what the case says it is, and the points claimed to have a row written in a later pass have one."""
    table = FW.cases(grid)
    for name, case in table.items():
        walks = case.walks(grid)
        print(name, case.n, case.chunks, FW.cut(case.n, case.chunks), walks)
        assert case.passes(grid) >= case.passes_min, name
        late, claimed = case.late_points(grid), case.claimed_late(grid)
        assert (late >= claimed).all(), name
        assert claimed.any() == (name != "E")
        for sl in FW.one_pass_slices(case.count, case.chunks, grid):
            assert FW.walk(-(-(sl.stop - sl.start) // 16), case.chunks, grid)[2] == 1, name
        assert sum(sl.stop - sl.start for sl in FW.one_pass_slices(case.count, case.chunks, grid)) == case.count
    a, b, c, d, e = (table[k] for k in CASE_NAMES)
    # A: 3 passes or more, all points late, the last group padded, the next unit in another group AND another chunk
    _, bn, groups, units, blocks, passes = a.walks(grid)[0]
    assert len(a.walks(grid)) == 1 and passes >= 3 and blocks == grid and grid % groups != 0 and bn % 16 == 13 and a.claimed_late(grid).all()
    assert a.chunks == 5 and FW.cut(a.n, 5) == [(k, k + 1) for k in range(5)] and a.n % 512 == 1
    for blk in range(grid):
        (g0, c0), (g1, c1) = FW.unit_of(blk, 0, groups, 5, grid), FW.unit_of(blk, 1, groups, 5, grid)
        assert g0 != g1 and c0 != c1
    # B: one launch under its own batch, one chunk: the next unit is another group of the same chunk
    _, bn, groups, units, blocks, passes = b.walks(grid)[0]
    assert len(b.walks(grid)) == 1 and b.chunks == 1 and passes == 3 and units == groups and bn % 16 == 7
    assert FW.unit_of(3, 1, groups, 1, grid) == (3 + grid, 0) and FW.unit_of(3, 2, groups, 1, grid) == (3 + 2 * grid, 0) and units == 2 * grid + 5
    assert not b.claimed_late(grid)[:16 * grid].any() and b.claimed_late(grid)[16 * grid:].all() and (b.late_points(grid) == b.claimed_late(grid)).all()
    # C: the rule's two chunks, three launches, the last of 17 points and one pass; at 1 024 workgroups the next unit is the same group's next chunk
    assert c.chunks == 2 and FW.cut(c.n, 2) == [(0, 8), (8, 17)] and c.chunks_option == 0 and c.batch == 0
    assert [(first, bn, groups) for first, bn, groups, *_ in c.walks(grid)] == [(0, 16384, 1024), (16384, 16384, 1024), (32768, 17, 2)]
    assert [w[5] for w in c.walks(grid)] == [2048 // grid, 2048 // grid, 1] and c.walks(grid)[2][3:5] == (4, 4)
    assert c.claimed_late(grid)[:32768].all() and not c.late_points(grid)[32768:].any()
    if grid == FW.GRID:
        assert all(FW.unit_of(blk, 1, 1024, 2, grid) == (blk, 1) and FW.unit_of(blk, 0, 1024, 2, grid) == (blk, 0) for blk in range(grid))
    # D: the cap of 16 chunks, 8 or 9 tiles each; the call of 64 makes one pass, the call of 3 200 points 3 200 units
    assert d.chunks == 16 and FW.chunks_of(d.n + 512 * 40) == 16 and {hi - lo for lo, hi in FW.cut(d.n, 16)} == {8, 9}
    assert d.walks(grid, 64)[0][3:] == (64, 64, 1) and d.walks(grid)[0][3] == 3200 and d.passes(grid) == -(-3200 // grid) and d.claimed_late(grid).all()
    # E: three chunks of 8, 8 and 9 tiles (with two tiles a stage: an odd tail stage), one pass at every count
    assert e.chunks == 3 and [hi - lo for lo, hi in FW.cut(e.n, 3)] == [8, 8, 9] and e.counts == (1, 16, 17, 33)
    assert all(w[5] == 1 for count in e.counts for w in e.walks(grid, count))


@pytest.mark.parametrize("grid", [FW.GRID, FW.SMALL_GRID])
def test_wrap_subsets_and_points(grid):
    """The rows compared with fp64 hold points of the first group, of a group in the middle and of the last, padded group, both
    sides of every launch boundary and rows written in a later pass; the points hold all four kinds and the skip entries the
    cases need: slot 0, a tile's last slot, the last real slot, a slot in the second and in the last tile of every chunk, and -1."""
    for name, case in FW.cases(grid).items():
        for count in (case.counts if name != "E" else case.counts[-1:]):
            rows = FW.subset(case, grid, count)
            groups = -(-count // 16)
            assert len(rows) == len(set(rows.tolist())) and rows.min() == 0 and rows.max() == count - 1 and len(rows) * case.n <= 1.05 * FW.PAIRS_LIMIT
            assert len(rows) >= min(count, 100)
            for first, bn, launch_groups in FW.launches(count, case.batch):
                for g in (0, launch_groups // 2, launch_groups - 1):
                    assert (((rows - first) // 16 == g) & (rows >= first) & (rows < first + bn)).any(), (name, first, g)
            assert ((rows // 16) == groups - 1).sum() == count - 16 * (groups - 1), "the last group: all its real points"
            for first, bn, _ in FW.launches(count, case.batch)[1:]:
                assert {first - 1, first}.issubset(rows.tolist())
            if count == case.count and name != "E":
                late = case.late_points(grid)
                assert late[rows].sum() >= len(rows) // 2, name
            s = F.system(min(case.n, 2049)) if case.n > 20000 else F.system(case.n)      # the largest case: the slots alone matter here
            slots = FW.special_slots(case.n, case.chunks)
            assert {0, 511, case.n - 1} <= set(slots.tolist()) and len(slots) <= min(case.counts[-1], 64)
            for lo, hi in FW.cut(case.n, case.chunks):
                tiles = set((slots // 512).tolist())
                assert min(lo + 1, hi - 1) in tiles and hi - 1 in tiles
            if case.n <= 20000:
                p, v, skip = FW.mixed_points(s, count, case.chunks, 100)
                assert p.shape == v.shape == (3, count) and skip.shape == (count,) and p.dtype == v.dtype == np.float32 and skip.dtype == np.int32
                assert set(slots.tolist()) <= set(skip.tolist()) and (skip == -1).any() and skip.min() == -1 and skip.max() == case.n - 1
                assert set(FW.special_rows(count, len(slots)).tolist()) <= set(rows.tolist())
                own = skip >= 0
                on_body = own & (p[0] == s["qx"][np.maximum(skip, 0)])
                far = np.abs(p).max(0) > 100
                assert on_body.sum() > count // 8 and far.sum() > count // 8 and (own & ~on_body).sum() > count // 16
                assert not v[:, far].any() and np.isfinite(FW.doubled(p)).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_wrap_stale_rows_have_power(name):
    """What a unit left out leaves in its rows is the call before: the same count at the doubled points.  The fp64 field there,
    in the place of the measured call's, misses field_ref's bound on EVERY row of the subset by three orders of magnitude: the
    largest of a row's three scaled errors, each over its own bound C * 2^-24, is 1 000 or more."""
    grid = FW.GRID
    case = FW.cases(grid)[name]
    s = F.system(case.n)
    p, v, skip = FW.mixed_points(s, case.count, case.chunks, 100)
    rows = FW.subset(case, grid)
    ref, c = FW.reference(case, s, p, v, skip, rows)
    power = FW.stale_power(case, s, p, v, skip, rows, ref, c)
    print(f"case {name}: {len(rows)} rows, C = " + ", ".join(f"{k} {c[k]:.1f}" for k in c) + f"; stale rows miss by {power.min():.3g} x the bound or more")
    assert all(0.0 < c[k] < 200.0 for k in c)
    assert (power >= 1000.0).all()

"""GPU: the field read-out (murbfield_at / murbfield_of) beyond one pass of its fixed grid, beyond one launch, under the chunk
cut of the rule itself, and across growth of its buffers.  murb_force_field_kernel walks units u = blockIdx.x, += grid;
everything made again inside that loop (the kernel argument, tid and lane, the points' scalar values and skip entries, the
tile range, the zeroed sums, the LDS stage behind the barrier "of the unit before", the row index) matters from a workgroup's
second unit on, and tests/test_field_gpu.py has at most 20 units.  tests/helpers/field_wrap.py restates the walk and lists
the cases; tests/test_field_host.py pins their arithmetic and the power of the stale-row probe on the CPU.

Yardsticks: field_ref's fp64 field within field_ref.bound_of's bound (computed on the CPU from the inputs) on a subset of rows;
and bits against bits on every row: a point carries the bits it has in calls so short that no workgroup takes a second unit
(the same context, the same chunk count, consecutive slices of the same points), in a second run and in a fresh context.

The partial rows are not cleared between calls.  Immediately before every measured call the same context makes a call of the
same count at the doubled points 2p, which writes the same rows: a unit left out leaves those, three orders of magnitude beyond
the bound (tests/test_field_host.py::test_wrap_stale_rows_have_power)."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import field_ref as F         # noqa: E402
import field_wrap as FW       # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 100


@pytest.fixture(scope="module")
def grid(gpu):
    """Workgroups of the field sweep on the device at hand: 4 per CU."""
    with gpu.Simulation(16, soft=F.SOFT) as sim:
        return FW.grid_of(sim.info("block_grid"))


def open_sim(gpu, s, **options):
    sim = gpu.Simulation(len(s["m"]), soft=F.SOFT)
    for k, v in options.items():
        sim.set_field_option(k, v)
    sim.upload(s)
    return sim


@lru_cache(maxsize=None)
def system(n):
    return F.system(n)


@lru_cache(maxsize=None)
def points(name, grid, count):
    """The case's points of a call of `count` points; case E: the first `count` of its 33."""
    case = FW.cases(grid)[name]
    s = system(case.n)
    if name == "E":
        return tuple(x[..., :count] for x in FW.mixed_points(s, case.count, case.chunks, SEED))
    return FW.mixed_points(s, count, case.chunks, SEED + count % 89)


@lru_cache(maxsize=None)
def truth(name, grid, count, kind="mixed"):
    """(rows, fp64 reference, C) of a call: the case's points, the same at rest, or the repeated bodies' own values."""
    case = FW.cases(grid)[name]
    s = system(case.n)
    p, v, skip = points(name, grid, count) if kind != "bodies" else F.body_points(s, FW.repeated_bodies(count, case.n))
    rows = FW.subset(case, grid, count)
    return (rows,) + FW.reference(case, s, p, None if kind == "at rest" else v, skip, rows)


def measured(sim, p, v, skip, bodies=None):
    """The call behind a call of the same count at the doubled points, which writes the same rows."""
    sim.field_at(FW.doubled(p), v, skip)
    return sim.field_at(p, v, skip) if bodies is None else sim.field_of(bodies)


def check_rows(got, rows, ref, c, what):
    return F.check({k: got[k][rows] for k in F.KEYS}, ref, c, f"{what}, {len(rows)} rows")


def describe(case, grid, count=None):
    return "; ".join(f"{bn} points = {groups} groups x {case.chunks} chunks = {units} units on {blocks} of {grid} workgroups: {passes} passes"
                     for _, bn, groups, units, blocks, passes in case.walks(grid, count))


# ------------------------------------------------------------------------------------------------------------- 0. pass counts
def test_pass_counts(gpu, grid):
    """The device's own grid: units and passes of every case, and case A makes at least 3 passes, so that this file cannot go
    blind on another chip."""
    table = FW.cases(grid)
    for name, case in table.items():
        with gpu.Simulation(case.n, soft=F.SOFT) as sim:
            for k, v in case.options().items():
                sim.set_field_option(k, v)
            assert sim.field_option("field_chunks") == case.chunks, name
            assert sim.field_option("field_batch") == (case.batch or FW.BATCH_DEFAULT), name
        for count in case.counts:
            print(f"case {name}, n={case.n}, chunks {FW.cut(case.n, case.chunks)}: {describe(case, grid, count)}")
        assert case.passes(grid) >= case.passes_min, (name, grid)
        assert (case.late_points(grid) >= case.claimed_late(grid)).all(), name
    assert table["A"].passes(grid) >= 3


# --------------------------------------------------------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_past_one_pass(gpu, grid, name):
    """Per call of the case: fp64 on the subset of rows behind the stale call; every row's bits against calls of one pass each;
    the same call again; a fresh context.  B also at rest; A and C also field_of of a long list with repeats."""
    case = FW.cases(grid)[name]
    assert case.passes(grid) >= case.passes_min, f"case {name} makes {case.passes(grid)} passes on {grid} workgroups, not {case.passes_min}"
    s = system(case.n)
    kept = {}
    with open_sim(gpu, s, **case.options()) as sim:
        assert sim.field_option("field_chunks") == case.chunks
        for count in case.counts:
            what = f"case {name} ({describe(case, grid, count)})"
            p, v, skip = points(name, grid, count)
            if count == case.count or name != "E":
                assert set(FW.special_slots(case.n, case.chunks).tolist()) <= set(skip.tolist()), "slot 0, a tile's last, the last real one, every chunk"
            big = measured(sim, p, v, skip)
            check_rows(big, *truth(name, grid, count), what)
            for sl in FW.one_pass_slices(count, case.chunks, grid):
                assert FW.walk(-(-(sl.stop - sl.start) // FW.GROUP), case.chunks, grid)[2] == 1
                part = sim.field_at(p[:, sl], v[:, sl], skip[sl])
                for k in F.KEYS:
                    bad = np.flatnonzero(F.bits(part[k]) != F.bits(big[k][sl]))
                    assert len(bad) == 0, f"{what}: {k} of {len(bad)} points from {sl.start + bad[0]} on differs from the call of points {sl.start} ... {sl.stop}"
            assert F.same_bits(measured(sim, p, v, skip), big), what + ": the same call again"
            kept[count] = big
            if name == "B":
                rest = measured(sim, p, None, skip)
                check_rows(rest, *truth(name, grid, count, "at rest"), what + ", at rest")
                parts = [sim.field_at(p[:, sl], None, skip[sl]) for sl in FW.one_pass_slices(count, case.chunks, grid)]
                assert all(np.array_equal(F.bits(np.concatenate([x[k] for x in parts])), F.bits(rest[k])) for k in F.KEYS), what + ", at rest: bits"
                assert all(np.array_equal(F.bits(rest[k]), F.bits(big[k])) for k in ("ax", "ay", "az", "phi")), "a and phi do not see the velocities"
            if name in ("A", "C"):
                bodies = FW.repeated_bodies(count, case.n)
                bp, bv, bskip = F.body_points(s, bodies)
                of = measured(sim, bp, bv, bskip, bodies)
                check_rows(of, *truth(name, grid, count, "bodies"), what + ", field_of")
                assert F.same_bits(of, measured(sim, bp, bv, bskip)), what + ": field_of is field_at at the bodies' own values"
                first = {k: of[k][:case.n] for k in F.KEYS}
                for lo in range(case.n, count, case.n):
                    assert all(np.array_equal(F.bits(of[k][lo:lo + case.n]), F.bits(first[k][:count - lo])) for k in F.KEYS), "a body listed again"
    with open_sim(gpu, s, **case.options()) as fresh:
        for count in case.counts[::-1]:
            assert F.same_bits(fresh.field_at(*points(name, grid, count)), kept[count]), f"case {name}, {count} points: a fresh context"


# ------------------------------------------------------------------------------------------------------------ 2. buffer growth
def test_buffer_growth(gpu, grid):
    """One context: 16 points, case A's count (the points' buffers grow), "field_chunks" 1 to 5 at that count (the rows alone
    grow), 16 points again in the grown buffers.  Every call gives the bits of the same call in a fresh context."""
    case = FW.cases(grid)["A"]
    s = system(case.n)
    p, v, skip = points("A", grid, case.count)
    small = (p[:, :16], v[:, :16], skip[:16])
    calls = [(0, small), (0, (p, v, skip))] + [(k, (p, v, skip)) for k in range(1, 6)] + [(5, small)]
    with open_sim(gpu, s) as sim:
        for chunks, (pp, pv, ps) in calls:
            sim.set_field_option("field_chunks", chunks)
            got = sim.field_at(pp, pv, ps)
            with open_sim(gpu, s, field_chunks=chunks) as fresh:
                assert fresh.field_option("field_chunks") == sim.field_option("field_chunks") == FW.chunks_of(case.n, chunks)
                assert F.same_bits(fresh.field_at(pp, pv, ps), got), f"{len(ps)} points, field_chunks {chunks}"

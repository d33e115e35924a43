"""The walk of the field sweep (murb_force_field_kernel, launched by field_run) restated, and the cases that
tests/test_field_wrap_gpu.py runs beyond one pass of its fixed grid, shared with tests/test_field_host.py, which pins their
arithmetic.  numpy only; nothing here touches a device.

A call of `count` points is cut into launches of at most "field_batch" points.  A launch of bn points has groups =
ceil(bn / 16) groups (the last filled up with copies of its first point) and walks groups x chunks units on a grid of
min(units, 4 workgroups per CU): workgroup b takes the units u = b, b + grid, ...; unit u is (group, chunk) =
(u % groups, u / groups) and writes the rows chunk * stride + 16 group ... + 15 with stride = 16 groups.  The rows are not
cleared between launches or calls, so a unit that is left out leaves what the launch before wrote there."""
import numpy as np

import field_ref as F

GROUP, TILE = 16, F.TILE
CUS = 256                              # an MI355X
GRID = 4 * CUS                         # 1 024 workgroups: info("block_grid") / 5 * 4
SMALL_GRID = 4 * 64                    # a chip of 64 CUs
TILES_PER_CHUNK, CHUNKS_MAX, BATCH_DEFAULT = 8, 16, 16384      # csrc/murb_field.h
Q, V = F.Q, F.V


def grid_of(block_grid):
    """The field sweep's workgroups from info("block_grid") (5 per CU): 4 per CU."""
    return int(block_grid) // 5 * 4


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def tiles_of(n):
    return -(-n // TILE)


def chunks_of(n, option=0):
    """murb_field_layout: "field_chunks" k > 0 = k, 0 = tiles / 8 within [1, 16]; never more than the tiles."""
    tiles = tiles_of(n)
    return min(option if option > 0 else min(max(tiles // TILES_PER_CHUNK, 1), CHUNKS_MAX), tiles)


def cut(n, chunks):
    """[(first tile, end tile)] of the chunks."""
    tiles = tiles_of(n)
    return [(tiles * c // chunks, tiles * (c + 1) // chunks) for c in range(chunks)]


def launches(count, batch=0):
    """[(first point, points, groups)] of a call."""
    batch = batch or BATCH_DEFAULT
    return [(first, min(batch, count - first), -(-min(batch, count - first) // GROUP)) for first in range(0, count, batch)]


def walk(groups, chunks, grid):
    """(units, workgroups, passes) of one launch."""
    units = groups * chunks
    blocks = max(1, min(units, grid))
    return units, blocks, -(-units // blocks)


def unit_of(block, k, groups, chunks, grid):
    """(group, chunk) of workgroup `block`'s k-th unit (k = 0: its first), or None where it has none."""
    units, blocks, _ = walk(groups, chunks, grid)
    u = block + k * blocks
    return (u % groups, u // groups) if block < blocks and u < units else None


def late_units(groups, chunks, grid):
    """bool (chunks, groups): the units that are some workgroup's second or later one."""
    units, blocks, _ = walk(groups, chunks, grid)
    return (np.arange(units) >= blocks).reshape(chunks, groups)


def late_points(count, chunks, grid, batch=0):
    """bool (count): the points of a call with at least one chunk row written in a workgroup's second or later unit."""
    out = np.zeros(count, bool)
    for first, bn, groups in launches(count, batch):
        out[first:first + bn] = np.repeat(late_units(groups, chunks, grid).any(0), GROUP)[:bn]
    return out


def one_pass_slices(count, chunks, grid):
    """Consecutive slices of a call's points, each so short that groups x chunks <= grid: no workgroup takes a second unit."""
    per = GROUP * max(grid // chunks, 1)
    return [slice(lo, min(count, lo + per)) for lo in range(0, count, per)]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """n bodies, the two field options (0: the default), the counts of its calls (the last one is the big call), the passes
    the big call's first launch claims, and the points it claims a late row for (claimed_late)."""

    def __init__(self, name, n, chunks_option, batch, counts, passes_min, late, what):
        self.name, self.n, self.chunks_option, self.batch, self.counts = name, n, chunks_option, batch, tuple(counts)
        self.passes_min, self.late, self.what = passes_min, late, what
        self.chunks = chunks_of(n, chunks_option)
        self.count = self.counts[-1]

    def options(self):
        return {k: v for k, v in (("field_chunks", self.chunks_option), ("field_batch", self.batch)) if v}

    def walks(self, grid, count=None):
        """[(first, points, groups, units, workgroups, passes)] of the launches of a call (the big call by default)."""
        return [(first, bn, groups) + walk(groups, self.chunks, grid)
                for first, bn, groups in launches(self.count if count is None else count, self.batch)]

    def passes(self, grid):
        return self.walks(grid)[0][5]

    def late_points(self, grid):
        return late_points(self.count, self.chunks, grid, self.batch)

    def claimed_late(self, grid):
        """bool (count): the points the case says have a row written in a second or later pass.  "all": every chunk but the
        first ones lies wholly beyond the grid, so every group has a late row; "groups beyond the grid": one chunk, the first
        `grid` groups are the workgroups' first units and all later ones are late; "full launches": every point of a launch of a
        full batch (the last, short launch makes one pass); "none"."""
        want = np.zeros(self.count, bool)
        if self.late == "all":
            want[:] = True
        elif self.late == "groups beyond the grid":
            want[GROUP * grid:] = True
        elif self.late == "full launches":
            for first, bn, _ in launches(self.count, self.batch):
                want[first:first + bn] = bn == (self.batch or BATCH_DEFAULT)
        return want


def cases(grid=GRID):
    """The case table of tests/test_field_wrap_gpu.py for a grid of `grid` workgroups."""
    return {
        "A": Case("A", 2049, 5, 0, (GROUP * (-(-3 * grid // 5) + 7) - 3,), 3, "all",
                  "5 tiles, the last padded, one chunk a tile; the groups do not divide the grid: a workgroup's next unit is another "
                  "group and another chunk; the last group is filled with copies"),
        "B": Case("B", 513, 1, GROUP * (2 * grid + 16), (GROUP * (2 * grid + 5) - 9,), 3, "groups beyond the grid",
                  "one chunk: a workgroup's next unit is another group of the same chunk; one of two tiles padded"),
        "C": Case("C", 8193, 0, 0, (2 * BATCH_DEFAULT + 17,), 2, "full launches",
                  "the rule's 2 chunks [0, 8) [8, 17), three launches at the default batch, the last of 17 points with a stride of "
                  "its own on the same rows; a workgroup's next unit is the same group's next chunk"),
        "D": Case("D", 65537, 0, 0, (64, GROUP * 200), 2, "all",
                  "129 tiles: the cap of 16 chunks, 8 or 9 tiles each"),
        "E": Case("E", 12289, 0, 0, (1, 16, 17, 33), 1, "none",
                  "25 tiles: the rule's 3 chunks of 8, 8 and 9 tiles, an odd tail stage; one pass"),
    }


# ---- points ------------------------------------------------------------------------------------------------------------------
def special_slots(n, chunks):
    """Skip entries every call must hold: slot 0, a tile's last slot, the last real slot (in the padded tile), and per chunk a slot
    of its second tile (the second tile of an LDS stage) and of its last tile (the tail stage)."""
    slots = [0, min(TILE, n) - 1, n - 1]
    for lo, hi in cut(n, chunks):
        slots += [min(n - 1, min(lo + 1, hi - 1) * TILE + 5), min(n - 1, (hi - 1) * TILE + TILE - 2)]
    return np.array(sorted(set(slots)), np.int32)


def special_rows(count, specials):
    """The points of a call that take the special skip entries: spread evenly, the first and the last point among them."""
    return np.unique(np.round(np.linspace(0, count - 1, min(specials, count))).astype(np.int64))


def mixed_points(s, count, chunks, seed):
    """(points (3, count), velocities (3, count), skip (count)) float32 / int32: a seeded mix of field_ref's three kinds — bodies'
    own values with themselves skipped, midpoints of body pairs with nobody skipped, far points at rest — and random points in the
    box with random skip entries, -1 among them; special_slots' entries sit on random points at special_rows (as many as the count
    has room for)."""
    n = len(s["m"])
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, count)
    b = rng.integers(0, n, count)
    bp, bv, _ = F.body_points(s, b)
    o = (b + 7) % n
    mp = np.stack([(s[c][b].astype(np.float64) + s[c][o]) * 0.5 for c in Q]).astype(np.float32)
    mv = np.stack([(s[c][b].astype(np.float64) + s[c][o]) * 0.5 for c in V]).astype(np.float32)
    u = rng.standard_normal((3, count))
    fp = (0.5 + 1e3 * u / np.linalg.norm(u, axis=0)).astype(np.float32)
    rp = rng.uniform(0.0, 1.0, (3, count)).astype(np.float32)
    rv = (1e-3 * rng.standard_normal((3, count))).astype(np.float32)
    rskip = np.where(rng.random(count) < 0.5, rng.integers(0, n, count), -1)
    which = [kind[None] == 0, kind[None] == 1, kind[None] == 2]
    p = np.select(which, [bp, mp, fp], rp).astype(np.float32)
    v = np.select(which, [bv, mv, np.zeros_like(fp)], rv).astype(np.float32)
    skip = np.select([kind == 0, kind == 3], [b, rskip], -1).astype(np.int32)
    at = special_rows(count, len(special_slots(n, chunks)))
    p[:, at], v[:, at], skip[at] = rp[:, at], rv[:, at], special_slots(n, chunks)[:len(at)]
    return np.ascontiguousarray(p), np.ascontiguousarray(v), skip


def doubled(p):
    """The points of the call that runs before every measured one, on the same rows."""
    return (np.float32(2.0) * p).astype(np.float32)


def repeated_bodies(count, n):
    return (np.arange(count) % n).astype(np.int32)


# ---- the rows compared with fp64 -----------------------------------------------------------------------------------------------
PAIRS_LIMIT = 8_000_000      # rows x bodies of one fp64 comparison: about a second of numpy


def subset(case, grid, count=None):
    """Rows of a call compared with fp64: of every launch the first group, the one in the middle and the last (padded) one, 8 points either side of every launch boundary, the rows of the special skip entries, and an even spread over
    the points with a late row — about 1 000 rows, fewer where the bodies are many (rows x bodies <= PAIRS_LIMIT; the rows named
    here and 16 of the spread always)."""
    count = case.count if count is None else count
    limit = max(64, min(1000, PAIRS_LIMIT // case.n))
    if count <= limit:
        return np.arange(count, dtype=np.int64)
    rows = []
    for k, (first, bn, groups) in enumerate(launches(count, case.batch)):
        mid = first + groups // 2 * GROUP
        rows += list(range(first, first + min(GROUP, bn))) + list(range(mid, min(mid + GROUP, first + bn))) + \
            list(range(first + (groups - 1) * GROUP, first + bn))
        if k > 0:
            rows += list(range(first - 8, min(count, first + 8)))
    rows += list(special_rows(count, len(special_slots(case.n, case.chunks))))
    late = np.flatnonzero(late_points(count, case.chunks, grid, case.batch))
    spread = late if len(late) else np.arange(count)
    rows += list(spread[np.linspace(0, len(spread) - 1, max(limit - len(set(rows)), 16)).astype(np.int64)])
    return np.array(sorted(set(int(r) for r in rows)), np.int64)


def eval_block(n):
    """Points per block of field_ref's evaluation, so that a block's arrays stay at some ten MB."""
    return int(max(8, min(256, (1 << 21) // n)))


def take(p, v, skip, rows):
    return p[:, rows], None if v is None else v[:, rows], None if skip is None else skip[rows]


def reference(case, s, p, v, skip, rows):
    """(ref, C) of field_ref.bound_of on the rows `rows` of the call."""
    return F.bound_of(*take(p, v, skip, rows), s, F.SOFT, block=eval_block(case.n))


def stale_power(case, s, p, v, skip, rows, ref, c):
    """Per row: the fp64 field at the doubled points (what a unit left out leaves in its rows) in the place of the call's own:
    the largest of its three scaled errors, each in units of its own bound C * 2^-24."""
    pp, pv, sk = take(p, v, skip, rows)
    stale = F.field_f64(doubled(pp), pv, sk, s, F.SOFT, want_abs=False, block=eval_block(case.n))[:3]
    e = F.scaled_errors(stale, ref)
    return np.max([e[k] / (c[k] * F.U24) for k in ("a", "j", "phi")], axis=0)

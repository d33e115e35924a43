"""The shapes of the active sweep's unit loop that tests/test_block_wrap_gpu.py runs, and the arithmetic of
murb_block_plan_kernel and ensure_block restated, shared with tests/test_hermite_block_host.py.  numpy only; nothing here
touches a device.

A block step of `active` bodies has groups = ceil(active / 16) i groups; murb_block_plan_kernel cuts the j range into
chunks = clamp(ceil(U / groups), 1, tiles) chunks for "block_units" U, and the active sweep walks groups x chunks units with a
fixed grid: 5 workgroups per CU in the plain form, 4 in the nearest, contact and potential forms.  The rows of the partial sums
are sized slots + 16 U by ensure_block; the sweep writes 16 x units of them."""
import numpy as np

from active_sets import active_sets

GROUP, TILE, SLOT_STEP = 16, 512, 1024
CUS = 256                                   # an MI355X
GRID_PLAIN, GRID_OPTION = 5 * CUS, 4 * CUS  # 1 280 and 1 024 workgroups
MAIN, PADDED, DEEP = 5120, 4609, 9217       # 10 tiles without padding, 10 tiles with one body in the last, 20 tiles
CUTS = {MAIN: (1, 4, 5, 7, 10), PADDED: (1, 10), DEEP: (20,)}
TIGHT_U = 320 * 9 + 1                       # n = 5 120: the smallest U that gives 320 groups 10 chunks


def slots_of(n):
    """Body slots of one shard (multiples of 1 024; asserted against murbhip_slice_slots on the host)."""
    return -(-n // SLOT_STEP) * SLOT_STEP


def plan(active, units, tiles):
    """(groups, chunks, units walked) of murb_block_plan_kernel."""
    groups = -(-active // GROUP)
    chunks = min(max(-(-units // groups), 1), tiles)
    return groups, chunks, groups * chunks


def passes(units, grid):
    return -(-units // grid)


def cut(tiles, chunks):
    """Tiles per chunk: [tiles c / chunks, tiles (c + 1) / chunks) like the sweep."""
    return [tiles * (c + 1) // chunks - tiles * c // chunks for c in range(chunks)]


def wrap_sets(n):
    """The active sets of a case, the largest first: all n, range(1, n), every second body, then active_sets(n)'s small ones."""
    small = [a for a in active_sets(n) if len(a) < n - 1]
    return [np.arange(n, dtype=np.int64), np.arange(1, n, dtype=np.int64), np.arange(0, n, 2, dtype=np.int64)] + small


def depth_set(n):
    """64 spread bodies and active_sets' specials: 4 to 5 groups, which run in the sweep's first pass at any cut."""
    special = [0, n - 1, 511, 512, 1022, 1023, 1, 1024]
    spread = [int(x) for x in np.linspace(3, n - 3, 64).astype(np.int64)]
    return np.array(sorted(set(special + spread)), np.int64)


def units_of(n, c):
    """"block_units" of a case for an active set of `groups` groups: groups x c, or TIGHT_U whatever the set (c = "tight")."""
    return (lambda groups: TIGHT_U) if c == "tight" else (lambda groups: groups * c)


def cases():
    """Every (n, active count, U) the GPU file runs."""
    out = []
    for n, cs in CUTS.items():
        for c in cs + (("tight",) if n == MAIN else ()):
            for act in wrap_sets(n) + [depth_set(n)]:
                out.append((n, len(act), units_of(n, c)(-(-len(act) // GROUP))))
    return out


def fp64_rows(n, limit=1024):
    """The rows whose (a1, j1) are compared with fp64: all of them up to `limit` bodies, else an even spread plus the specials."""
    if n <= limit:
        return np.arange(n, dtype=np.int64)
    special = [0, n - 1, 511, 512, 1022, 1023, 1, 1024]
    spread = [int(x) for x in np.linspace(0, n - 1, limit - len(special)).astype(np.int64)]
    return np.array(sorted(set(special + spread)), np.int64)

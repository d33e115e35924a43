"""The shapes of the FULL Hermite sweep (murb_force_jerk_sweep: the sweep of murbhip_compute_acc_jerk, murbhip_step and
murbhip_evolve) that tests/test_full_wrap_gpu.py runs in its nearest, contact and potential form beyond six layout tiles, and
the rule of info("hermite_parts") restated from include/murbhip.h, shared with tests/test_full_wrap_host.py, which pins their
arithmetic.  numpy only; nothing here touches a device.

A sweep over `tiles` layout tiles of 512 slots runs one workgroup per (i group of 16 bodies, chunk); chunk c of `chunks` holds
the tiles [tiles c / chunks, tiles (c + 1) / chunks) and walks them in stages of two (the last stage of an odd chunk holds
one).  A wave's four bodies lie in one layout tile, its own.  The nearest and contact forms treat a tile as masked when it is
the wave's own or holds a slot >= n (padding); the potential form when it is the wave's own.  A masked tile adds nothing to
the side product inside the loop and is looked at again behind it."""
import numpy as np

TILE, GROUP, STAGE, SLOT_STEP = 512, 16, 2, 1024
CUS = 256                      # an MI355X
MAX_PARTS = 32                 # the most chunks "jsplit" can ask for
MIN_TILES_PER_CHUNK = 8        # the automatic rule never cuts finer
BLOCKS_PER_CU = 144            # ... and aims at 6 x 24 workgroups per CU

# lattice sizes (nearest_ref.dense_lattice): 10 tiles without a padding slot; 10 tiles, one body in the last; 20 tiles, 18 full,
# one body in tile 18, tile 19 padding only; 26 tiles in the same pattern
FULL, ONE_IN_LAST, DEEP, DEEPER = 5120, 4609, 9217, 12289
LATTICE_SIZES = (FULL, ONE_IN_LAST, DEEP, DEEPER)
ALL_CUTS = (0, 1, 3, 7, 32)                      # "jsplit"
CUTS = {FULL: ALL_CUTS, ONE_IN_LAST: ALL_CUTS, DEEP: ALL_CUTS, DEEPER: (0, 1, 32)}
EVOLVE_CUT = 3                                   # the cut at which evolve() is compared with step(); DEEPER has no 3 and takes 0
GALAXY_SIZES = (12289, 30000)
GALAXY_CUTS = {12289: (0, 1, 32), 30000: (0, 1)}        # potential
GALAXY_NEAREST_CUTS = (0, 1, 32)                 # nearest, n = 30 000
GALAXY_SOFT = np.float32(2e8)
DEFAULT_CHUNKS = {FULL: 1, ONE_IN_LAST: 1, DEEP: 2, DEEPER: 3, 30000: 7}      # "jsplit" 0 on 256 CUs
OWN_PAIR_SLOTS = (7 * TILE + 5, 17 * TILE + 1)   # the heavy pair of potential_ref.own_term_pair at n = DEEP: tiles 7 and 17
OWN_PAIR_CUTS = (0, 1, 32)
SPARSE_SOURCES = 64                              # potential_ref.sparse(DEEP, sources=64): sources in all 19 body-holding tiles
WALK = (32, 1, 7, 0, 32)                         # the cuts one context walks through at n = DEEP


def slots_of(n):
    """Body slots of one shard (multiples of 1 024; asserted against murbhip_slice_slots on the host)."""
    return -(-n // SLOT_STEP) * SLOT_STEP


def tiles_of(n):
    return slots_of(n) // TILE


def parts(jsplit, n, cus=CUS):
    """info("hermite_parts"): "jsplit" clamped to the layout tiles and 32, or for 0 the automatic rule: enough chunks for
    144 workgroups per CU, but chunks of at least 8 tiles, at most 32."""
    tiles = tiles_of(n)
    if jsplit > 0:
        return min(jsplit, tiles, MAX_PARTS)
    groups = slots_of(n) // GROUP
    return max(1, min(-(-cus * BLOCKS_PER_CU // groups), tiles // MIN_TILES_PER_CHUNK, MAX_PARTS))


def cut(tiles, chunks):
    """[(first tile, end tile)] of the chunks, like the sweep."""
    return [(tiles * c // chunks, tiles * (c + 1) // chunks) for c in range(chunks)]


def masked(tile, own, n, padding=True):
    """murb_nn_tile_masked: the tile holds the wave's own bodies or (padding) a slot >= n.  padding=False: the potential form."""
    return tile == own or (padding and (tile + 1) * TILE > n)


def stages(n, chunks, own, padding=True):
    """Per chunk the stages of a wave whose bodies lie in tile `own`: a list (chunks) of lists (stages) of strings, one letter
    per tile of the stage, "M" masked or "U" unmasked: "UU", "UM", "MU", "MM", and "U" or "M" for a lone last tile."""
    out = []
    for t0, t1 in cut(tiles_of(n), chunks):
        out.append(["".join("M" if masked(t, own, n, padding) else "U" for t in range(vs, min(vs + STAGE, t1)))
                    for vs in range(t0, t1, STAGE)])
    return out


def longest_unmasked_run(chunk_stages):
    """The most consecutive fully unmasked two-tile stages of one chunk."""
    best = run = 0
    for st in chunk_stages:
        run = run + 1 if st == "UU" else 0
        best = max(best, run)
    return best


def cases(cus=CUS):
    """Every (n, jsplit, chunks) of the lattice and galaxy cases the GPU file runs."""
    out = [(n, j, parts(j, n, cus)) for n in LATTICE_SIZES for j in CUTS[n]]
    out += [(n, j, parts(j, n, cus)) for n in GALAXY_SIZES for j in GALAXY_CUTS[n]]
    return out + [(30000, j, parts(j, 30000, cus)) for j in GALAXY_NEAREST_CUTS]


def spread_rows(n, count=1024):
    """The rows compared with fp64 where all n are too many: an even spread plus the tile ends and the first and last body."""
    if n <= count:
        return np.arange(n, dtype=np.int64)
    special = [0, 1, 511, 512, 1022, 1023, 1024, n - 2, n - 1, (n - 1) // TILE * TILE]
    spread = [int(x) for x in np.linspace(0, n - 1, count).astype(np.int64)]
    return np.array(sorted(set(special + spread)), np.int64)


def doubled(s):
    """The state a context evaluates before every measured evaluation, on the same rows: positions doubled."""
    return {k: (np.float32(2.0) * v if k in ("qx", "qy", "qz") else v.copy()) for k, v in s.items()}

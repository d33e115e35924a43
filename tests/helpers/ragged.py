"""TEST INFRASTRUCTURE: the residues of a ragged last block that the layout checker (tests/test_abi_and_host.py), the planner
self-test (plan_selftest.cpp keeps its own copy of the list) and the GPU probes (tests/test_ragged_block_gpu.py) sweep, and the
probe sources that put mass on both sides of every place where the pair-symmetric work list can cut such a block.

`rem` is the number of real bodies in the last block of 1024 slots of a slice.  The pad-aware work list cuts the piece that
straddles the last real body to the next multiple of 16 x waves bodies (64 or 128), derives a triangular diagonal piece's
steps of 128 bodies from the cut, and drops sub-blocks that lie wholly in padding."""
import numpy as np

BLOCK = 1024
# both sides of: one body, the 16-slot granule, the 64- and 128-body cuts, the triangular pieces' 128-body steps (odd multiples
# of 64 as well), the 512-slot layout tile, the sub-blocks of a split of 4, 8 and 16, and the full block
REMS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 383, 385, 511, 513, 767, 769, 895, 897, 959, 961, 1023)


def ragged_offsets(real):
    """Offsets in a block that holds `real` < 1024 bodies: its first body, both sides of every multiple of 64 below `real`,
    the body before the last one (oracle.probe_sources places a slice's last body itself)."""
    offs = {0, max(real - 2, 0)}
    for c in range(64, real, 64):
        offs.update((c - 1, c))
    return sorted(o for o in offs if o < real)


def ragged_sources(firsts, counts, slice_slots):
    """Body indices at ragged_offsets() of every block that is partly filled (a slice's last one)."""
    out = []
    for f, c in zip(firsts, counts):
        for b in range(slice_slots // BLOCK):
            real = min(BLOCK, max(0, c - b * BLOCK))
            if 0 < real < BLOCK:
                out.extend(f + b * BLOCK + o for o in ragged_offsets(real))
    return np.array(sorted(set(out)), np.int64)

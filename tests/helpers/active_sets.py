"""Active sets of one block step, shared by the GPU tests that force the shape of the active sweep."""
import numpy as np

SIZES = (1, 3, 4, 5, 15, 16, 17, 64, 65)


def active_sets(n):
    """Active sets of 1 ... n bodies.  The places: slot 0, both halves of a pair, the last slot of a tile and the first of the
    next, the last real body before the padding; the rest spread evenly."""
    special = [0, n - 1, 511, 512, 1022, 1023, 1, 1024]
    spread = [int(x) for x in np.linspace(2, n - 2, 97).astype(np.int64) if int(x) not in special]
    order = special + spread
    sets = [[b] for b in (0, 511, 512, n - 1)] + [[1022, 1023]] + [order[:m] for m in SIZES if m > 1]
    sets += [list(range(1, n)), list(range(n))]
    return [np.array(sorted(set(x)), np.int64) for x in sets]

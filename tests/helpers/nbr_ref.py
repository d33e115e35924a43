"""numpy restatement of the neighbours-within-a-radius read-out, written from the text of include/murbnbr.h, not from the device
code.

Per point the candidates (all real bodies but the point's skipped slot; massless ones included, never the padding behind the n
bodies) with r2 <= thr, thr = (float)((double)h * h + (double)soft2), in ascending body index, in CSR form."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as K           # noqa: E402
import nearest_ref as NR      # noqa: E402


def thresholds(h, soft2, count):
    """float32 thr per point of a scalar h or of one radius per point (nearest_ref.threshold: murbhip_set_encounter's rule)."""
    h = np.broadcast_to(np.asarray(h, np.float32), (count,))
    return np.array([NR.threshold(x, soft2) for x in h], np.float32)


def csr(inside, r2):
    """(offsets uint64, idx int32, r2 float32) of a boolean matrix (points, bodies) and the r2 of its pairs: row-major order is
    ascending body index within a point."""
    counts = inside.sum(1)
    offsets = np.zeros(inside.shape[0] + 1, np.uint64)
    offsets[1:] = np.cumsum(counts)
    p, j = np.nonzero(inside)
    return offsets, j.astype(np.int32), r2[p, j].astype(np.float32)


def neighbours(q_int, soft2, h, bodies=None, strict=False, block=NR.ROW_BLOCK):
    """Lists of the listed bodies (None: all, in order) of an integer lattice (exact r2: nearest_ref.r2_rows, +inf at a body's own
    index).  strict: the deliberately wrong rule r2 < thr."""
    q_int = np.asarray(q_int)
    n = q_int.shape[1]
    rows = np.arange(n) if bodies is None else np.asarray(bodies, np.int64)
    thr = thresholds(h, soft2, len(rows))
    parts = []
    for a in range(0, n, block):
        b = min(a + block, n)
        r2 = NR.r2_rows(q_int, soft2, a, b)
        parts.append(r2)
    full = np.concatenate(parts, 0)[rows]      # (count, n); the lattices of the tests have a few thousand bodies
    inside = (full < thr[:, None]) if strict else (full <= thr[:, None])
    return csr(inside, full)


def neighbours_at(q_int, soft2, h, p_int, skip=None):
    """Lists of integer points p_int (3, P) with per point a skipped body or -1 (None: none)."""
    qi, pi = np.asarray(q_int, np.int64), np.asarray(p_int, np.int64)
    d2 = np.zeros((pi.shape[1], qi.shape[1]), np.int64)
    for c, pc in zip(qi, pi):
        d = c[None, :] - pc[:, None]
        d2 += d * d
    want = d2.astype(np.float64) + float(soft2)
    r2 = want.astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), want), "r2 is not exact in fp32"
    if skip is not None:
        skip = np.asarray(skip)
        rows = np.nonzero(skip >= 0)[0]
        r2[rows, skip[rows]] = np.inf
    thr = thresholds(h, soft2, pi.shape[1])
    return csr(r2 <= thr[:, None], r2)


def neighbours_f64(state, soft, h):
    """(inside (n, n) bool, r2 (n, n) fp64, thr float32, near): membership of a float state's bodies from knn_ref.r2_f64 at a
    common h, and the number of pairs whose fp64 r2 lies within 4 fp32 ulps of thr, the pairs a test cannot decide."""
    soft2 = np.float32(soft) * np.float32(soft)
    thr = NR.threshold(h, soft2)
    r2 = K.r2_f64(state, soft)
    ulp = float(np.spacing(thr))
    near = int((np.abs(r2 - float(thr)) <= 4 * ulp).sum())
    return r2 <= float(thr), r2, thr, near


def fof_bfs(inside):
    """Group labels (the smallest body index of the connected component) of a symmetric boolean adjacency matrix: a plain
    breadth-first search."""
    n = inside.shape[0]
    label = np.full(n, -1, np.int32)
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s
        todo = [s]
        while todo:
            nxt = []
            for a in todo:
                for b in np.nonzero(inside[a])[0]:
                    if label[b] < 0:
                        label[b] = s
                        nxt.append(b)
            todo = nxt
    return label


def same(a, b):
    """Two (offsets, idx, r2) results, bit for bit."""
    return (np.array_equal(np.asarray(a[0], np.uint64), np.asarray(b[0], np.uint64)) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.int32), np.asarray(b[2], np.float32).view(np.int32)))

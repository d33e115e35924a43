"""numpy restatement of the k-nearest-neighbour read-out, the density estimator and the density centre, written from the text of
include/murbknn.h, not from the device code.

Per point the k smallest candidates under the total order (r2 as fp32, index), ascending; candidates are all real bodies but
the point's skipped slot (massless ones included, never the padding behind the n bodies); fewer than k: tails of -1 / +inf."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nearest_ref as NR      # noqa: E402

TILE = NR.TILE
FOUR_THIRDS_PI = 4.1887902047863905


def take_k(r2, k, first=0):
    """Of rows of fp32 r2 (rows, m) whose column c is candidate first + c (+inf: no candidate): (idx (rows, k) int32,
    r2 (rows, k) float32).  A stable sort keeps equal r2 in index order."""
    rows, m = r2.shape
    order = np.argsort(r2, axis=1, kind="stable")[:, :k]
    val = np.take_along_axis(r2, order, 1)
    idx = np.where(np.isinf(val), -1, order + first).astype(np.int32)
    if m < k:
        idx = np.concatenate([idx, np.full((rows, k - m), -1, np.int32)], 1)
        val = np.concatenate([val, np.full((rows, k - m), np.inf, np.float32)], 1)
    return idx, val.astype(np.float32)


def knn(q_int, soft2, k, lo=0, hi=None, block=NR.ROW_BLOCK):
    """Lists of every body of an integer lattice (exact r2: nearest_ref.r2_rows), candidates restricted to bodies [lo, hi)."""
    q_int = np.asarray(q_int)
    n = q_int.shape[1]
    hi = n if hi is None else min(hi, n)
    idx, val = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    for a in range(0, n, block):
        b = min(a + block, n)
        r2 = NR.r2_rows(q_int, soft2, a, b)[:, lo:hi]      # +inf at every body's own index
        idx[a:b], val[a:b] = take_k(r2, k, lo)
    return idx, val


def knn_at(q_int, soft2, k, p_int, skip):
    """Lists of integer points p_int (3, P) with per point a skipped body or -1."""
    qi, pi = np.asarray(q_int, np.int64), np.asarray(p_int, np.int64)
    d2 = np.zeros((pi.shape[1], qi.shape[1]), np.int64)
    for c, pc in zip(qi, pi):
        d = c[None, :] - pc[:, None]
        d2 += d * d
    want = d2.astype(np.float64) + float(soft2)
    r2 = want.astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), want), "r2 is not exact in fp32"
    skip = np.asarray(skip)
    rows = np.nonzero(skip >= 0)[0]
    r2[rows, skip[rows]] = np.inf
    return take_k(r2, k)


def merge(idx_a, r2_a, idx_b, r2_b, high_wins=False):
    """The k first of the merge of two lists under (r2, index), -1 last.  high_wins: the deliberately wrong rule "the higher
    index wins a tie"."""
    k = len(idx_a)
    idx = np.concatenate([idx_a, idx_b]).astype(np.int64)
    r2 = np.concatenate([r2_a, r2_b]).astype(np.float32)
    key = np.where(idx < 0, np.iinfo(np.int64).max, -idx if high_wins else idx)
    order = np.lexsort((key, r2))[:k]
    return idx[order].astype(np.int32), r2[order]


def density(idx, r2, masses, soft2):
    """float32 rho of lists idx, r2 (rows, k), k >= 2: include/murbknn.h's formula in numpy fp64 (every step one operation)."""
    idx, r2 = np.atleast_2d(idx), np.atleast_2d(r2)
    k = idx.shape[1]
    m = np.asarray(masses, np.float32).astype(np.float64)
    short = idx[:, k - 1] < 0
    d2 = np.where(short, 1.0, r2[:, k - 1].astype(np.float64) - float(np.float32(soft2)))
    mass = np.zeros(idx.shape[0])
    for l in range(k - 1):      # in list order
        mass = mass + np.where(short, 0.0, m[np.maximum(idx[:, l], 0)])
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = (mass / (FOUR_THIRDS_PI * (d2 * np.sqrt(d2)))).astype(np.float32)
    rho[d2 == 0.0] = np.inf
    rho[short] = 0.0
    return rho


def centre(rho, q):
    """out8 of include/murbknn.h in fp64 (math.fsum: the correctly rounded sums), and the scale sum rho |q| / S1 of X's bound."""
    import math
    rho = np.asarray(rho, np.float32)
    used = np.isfinite(rho)
    w = rho[used].astype(np.float64)
    p = np.asarray(q, np.float32)[:, used].astype(np.float64)
    s1, s2 = math.fsum(w), math.fsum(w * w)
    out = np.full(8, np.nan)
    out[5], out[6], out[7] = s1, used.sum(), (~used).sum()
    if s1 == 0.0:
        return out, np.nan
    x = np.array([math.fsum(w * c) / s1 for c in p])
    e = p - x[:, None]
    out[:3] = x
    out[3] = math.sqrt(math.fsum((w * w) * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) / s2)
    out[4] = s2 / s1
    return out, math.fsum(w * np.sqrt((p * p).sum(0))) / s1


def plummer(n, centre=(40.0, -25.0, 10.0), seed=3):
    """(state dict, soft): a Plummer sphere of scale 1 and total mass 1 about `centre`, truncated at 10 scale lengths, at rest
    velocities drawn small (the tests integrate it for a few steps only).  soft 1e-3."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, n)
    r = np.minimum(1.0 / np.sqrt(np.maximum(x ** (-2.0 / 3.0) - 1.0, 1e-2)), 10.0)
    u = rng.standard_normal((3, n))
    u /= np.linalg.norm(u, axis=0)
    q = (u * r + np.asarray(centre)[:, None]).astype(np.float32)
    v = (0.1 * rng.standard_normal((3, n))).astype(np.float32)
    m = np.full(n, 1.0 / n, np.float32)
    return {"qx": q[0], "qy": q[1], "qz": q[2], "vx": v[0], "vy": v[1], "vz": v[2], "m": m}, np.float32(1e-3)


def r2_f64(s, soft, n=None):
    """(n, n) fp64 r2 = |q_j - q_i|^2 + (fp32 soft * soft) of a state's fp32 positions, +inf on the diagonal."""
    q = np.stack([s["qx"], s["qy"], s["qz"]]).astype(np.float64)
    n = q.shape[1] if n is None else n
    r2 = np.zeros((n, n))
    for c in q:
        d = c[None, :n] - c[:n, None]
        r2 += d * d
    r2 += float(np.float32(soft) * np.float32(soft))
    r2[np.arange(n), np.arange(n)] = np.inf
    return r2

"""numpy restatement of the contact search by radii beside the Hermite sweeps (option "contact"), written from the text of
include/murbhip.h, not from the device code.

For real bodies i != j, with r2 the sweep's fp32 |q_j - q_i|^2 + soft2:
    s = R_i + R_j        e = r2 - soft2        gap2 = fmaf(-s, s, e)          (one fp32 operation each)
Per real body i the lexicographic minimum of (gap2, index) over all real j != i, massless ones included, never the body
itself, never the padding slots behind the n bodies.  A lone body has index -1 and gap2 = +inf.  gap2 <= 0: the two touch."""
import numpy as np

import nearest_ref as N
import hermite_block_ref as B   # noqa: F401  (the GPU tests take their clusters from it through this module)

TILE = N.TILE


def lattice(n, seed=1):
    """(state dict, soft, radii): nearest_ref.lattice(n) with radii that are multiples of 0.5, so that r2, e and gap2 are exact
    in fp32 (coordinates <= 1024, radii <= 200: every value is a multiple of 0.25 below 2^24 / 4).  From n = 513 up:
      R = 0.5 everywhere, except
      R[7] = 0       the massless body: bodies 7 and 8 are one unit apart, gap2 = 1 - 0.25 = 0.75 for both
      R[20] = 1.5    bodies 21 and 300 lie 2 away: s = 2, gap2 = 0 for all three, an exact touch (20 keeps the lowest index, 21)
      R[n-1] = 3     body 30 lies 3 away: gap2 = 9 - 12.25 = -3.25, although body 100 is just as near; body 100 gets 18 - 12.25
      R[50] = 200    with body 50 moved to (900, 900, 400): dozens of bodies lie inside it, most of which have a nearer neighbour
      bodies 5, 400  on one point: gap2 = 0 - 1 = -1."""
    s, soft = N.lattice(n, seed)
    s = {k: v.copy() for k, v in s.items()}
    r = np.full(n, 0.5, np.float32)
    if n >= 513:
        r[7], r[20], r[n - 1], r[50] = 0.0, 1.5, 3.0, 200.0
        s["qx"][50], s["qy"][50], s["qz"][50] = 900.0, 900.0, 400.0
    return s, soft, r


def _exact_gap2(qi, radii, soft2, lo, hi, rows=slice(None)):
    """gap2 (n, hi - lo) fp32 of every body (of the bodies `rows`) against bodies [lo, hi) of a lattice; asserts that every
    fp32 step is exact."""
    d = qi[:, None, lo:hi] - qi[:, rows, None]
    d2 = (d * d).sum(0).astype(np.float64)
    r2 = (d2 + float(soft2)).astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), d2 + float(soft2)), "r2 is not exact in fp32"
    e = r2 - np.float32(soft2)
    assert np.array_equal(e.astype(np.float64), d2), "e is not exact in fp32"
    s = radii[rows, None] + radii[None, lo:hi]                    # fp32 add
    s64 = radii.astype(np.float64)[rows, None] + radii.astype(np.float64)[None, lo:hi]
    assert np.array_equal(s.astype(np.float64), s64), "s is not exact in fp32"
    g64 = d2 - s64 * s64                                          # the fused multiply-add rounds this once
    g = g64.astype(np.float32)
    assert np.array_equal(g.astype(np.float64), g64), "gap2 is not exact in fp32"
    return g + np.float32(0.0)                                    # no -0


def contact(q, radii, soft2, n=None):
    """Brute force on a lattice (integer coordinates, radii multiples of 0.5): (index int32, gap2 float32), the lowest index
    among equal gap2."""
    q = np.asarray(q)
    n = q.shape[1] if n is None else int(n)
    radii = np.asarray(radii, np.float32)[:n]
    if n == 1:
        return np.array([-1], np.int32), np.array([np.inf], np.float32)
    g = _exact_gap2(q[:, :n].astype(np.int64), radii, soft2, 0, n)
    g[np.arange(n), np.arange(n)] = np.inf
    idx = g.argmin(1).astype(np.int32)      # argmin returns the first (lowest) index of the minimum
    return idx, g[np.arange(n), idx]


def gap2_rows(q_int, radii, soft2, lo, hi):
    """Rows [lo, hi) of gap2_matrix: fp32 gap2 (hi - lo, n), +inf at every body's own index."""
    qi = np.asarray(q_int, np.int64)
    n = qi.shape[1]
    g = _exact_gap2(qi, np.asarray(radii, np.float32)[:n], soft2, 0, n, rows=slice(lo, hi))
    g[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    return g


def contact_blocked(q_int, radii, soft2, block=N.ROW_BLOCK):
    """contact() without the (3, n, n) tensor: the same arithmetic in blocks of `block` rows.  Returns (index int32, gap2
    float32), the lowest index among equal gap2; a lone body has -1 and +inf."""
    n = np.asarray(q_int).shape[1]
    if n == 1:
        return np.array([-1], np.int32), np.array([np.inf], np.float32)
    idx, best = np.empty(n, np.int32), np.empty(n, np.float32)
    for lo in range(0, n, block):
        g = gap2_rows(q_int, radii, soft2, lo, min(lo + block, n))
        k = g.argmin(1)      # argmin returns the first (lowest) index of the minimum
        idx[lo:lo + block], best[lo:lo + block] = k, g[np.arange(len(k)), k]
    return idx, best


def chunked(q, radii, soft2, n, tiles, chunks):
    """The same search with the j range cut like the device cuts it (nearest_ref.chunked): every chunk's own lexicographic
    minimum, then the fold over the chunks in index order."""
    qi = np.asarray(q)[:, :n].astype(np.int64)
    radii = np.asarray(radii, np.float32)[:n]
    best_g = np.full(n, np.inf, np.float32)
    best_idx = np.full(n, -1, np.int32)
    own = np.arange(n)
    for c in range(chunks):
        lo, hi = TILE * (tiles * c // chunks), min(TILE * (tiles * (c + 1) // chunks), n)
        if hi <= lo:
            continue
        g = _exact_gap2(qi, radii, soft2, lo, hi)
        inside = (own >= lo) & (own < hi)
        g[own[inside], own[inside] - lo] = np.inf
        k = g.argmin(1)
        g_c = g[own, k]
        idx_c = np.where(np.isinf(g_c), -1, k + lo).astype(np.int32)
        best_g, best_idx = N.lex_min(best_g, best_idx, g_c, idx_c)
    return best_idx, best_g


def candidates(q, radii, soft2, n=None):
    """fp64 form on any values: (gap2 (n, n) fp64 with +inf on the diagonal, its minimum per body, bound (n, n)).
    bound = 1e-6 (r2 + s^2): the fp32 roundings are at most 6 on the r2 side (three differences, squared, three fused adds ...)
    and 3 on the s^2 side, each 2^-24, which stays below 4e-7 of r2 + s^2.  An index j is accepted for body i when
    gap2[i, j] <= best[i] + bound[i, j]; a value when it lies within bound[i, j] of gap2[i, j]."""
    q = np.asarray(q)
    n = q.shape[1] if n is None else int(n)
    q64 = q[:, :n].astype(np.float64)
    r64 = np.asarray(radii, np.float32)[:n].astype(np.float64)
    d = q64[:, None, :] - q64[:, :, None]
    d2 = (d * d).sum(0)
    s = r64[:, None] + r64[None, :]
    gap2 = d2 - s * s
    bound = 1e-6 * (d2 + float(soft2) + s * s)
    gap2[np.arange(n), np.arange(n)] = np.inf
    best = gap2.min(1) if n > 1 else np.full(n, np.inf)
    return gap2, best, bound


def check_candidates(idx, gap2, q, radii, soft2, rows=None):
    """(every index of `rows` is an accepted candidate, largest value error in units of the bound) for a device result."""
    g, best, bound = candidates(q, radii, soft2)
    n = g.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    ok_range = ((idx[rows] >= 0) & (idx[rows] < n) & (idx[rows] != rows)).all()
    if not ok_range:
        return False, np.inf
    gj, bj = g[rows, idx[rows]], bound[rows, idx[rows]]
    accepted = (gj <= best[rows] + bj).all()
    err = np.abs(gap2[rows].astype(np.float64) - gj) / bj
    return bool(accepted), float(err.max()) if len(rows) else 0.0


dense_lattice, shifted = N.dense_lattice, N.shifted      # the same bodies and the same shift serve both searches


def dense_radii(n, seed=1):
    """Radii for dense_lattice(n, seed): multiples of 0.5 from {0, 0.5, 1, 1.5} with weights (.5, .3, .15, .05), so that grid
    neighbours (one unit apart) overlap, touch exactly (s = 1) or miss each other, many of them at equal gap2, and a larger
    body further away often beats the nearest one."""
    rng = np.random.default_rng(seed + 104729)
    return rng.choice(np.array([0.0, 0.5, 1.0, 1.5], np.float32), size=n, p=[0.5, 0.3, 0.15, 0.05]).astype(np.float32)


def gap2_matrix(q_int, radii, soft2):
    """fp32 gap2 (n, n) of a lattice, +inf on the diagonal; _exact_gap2's asserts hold for every pair."""
    qi = np.asarray(q_int, np.int64)
    n = qi.shape[1]
    g = _exact_gap2(qi, np.asarray(radii, np.float32)[:n], soft2, 0, n)
    g[np.arange(n), np.arange(n)] = np.inf
    return g

"""numpy restatement of the nearest-neighbour search beside the Hermite sweeps (option "nearest") and of the encounter
threshold, written from the text of include/murbhip.h, not from the device code.

Per real body i the nearest other real body j != i (massless ones included, never the body itself, never the zero-mass
padding slots behind the n bodies), by the lexicographic minimum of (r2, index), r2 = |q_j - q_i|^2 + soft^2.  A lone body has
index -1 and r2 = +inf."""
import numpy as np

TILE = 512   # body slots per layout tile: the unit in which the device cuts the j range into chunks


def nearest(q, soft2, n=None, exact=False):
    """Brute force over the first n bodies of q (3, >= n).
    exact=True: q holds integers (a lattice), d2 is formed in int64 and r2 = float32(d2 + soft2), which is exact while
    d2 + soft2 needs no more than 24 bits: returns (index int32, r2 float32), the lowest index among equal r2.
    exact=False: fp64 arithmetic on the given values: returns (r2 fp64 minimum per body, candidates (n, n) bool): every j whose
    d2 + soft2 lies within a relative 1e-6 of the minimum."""
    q = np.asarray(q)
    n = q.shape[1] if n is None else int(n)
    q = q[:, :n]
    if exact:
        qi = q.astype(np.int64)
        d = qi[:, None, :] - qi[:, :, None]
        d2 = (d * d).sum(0)
        r2 = (d2.astype(np.float64) + float(soft2)).astype(np.float32)
        assert np.array_equal(r2.astype(np.float64), d2.astype(np.float64) + float(soft2)), "r2 is not exact in fp32"
        r2[np.arange(n), np.arange(n)] = np.inf
        if n == 1:
            return np.array([-1], np.int32), np.array([np.inf], np.float32)
        idx = r2.argmin(1).astype(np.int32)      # argmin returns the first (lowest) index of the minimum
        return idx, r2[np.arange(n), idx]
    q64 = q.astype(np.float64)
    d = q64[:, None, :] - q64[:, :, None]
    r2 = (d * d).sum(0) + float(soft2)
    r2[np.arange(n), np.arange(n)] = np.inf
    best = r2.min(1) if n > 1 else np.full(n, np.inf)
    return best, r2 <= best[:, None] * (1.0 + 1e-6)


def lex_min(r2_a, idx_a, r2_b, idx_b):
    """Elementwise lexicographic minimum of (r2 as fp32, index); index -1 (no candidate, r2 = +inf) loses to everything."""
    key_a = np.where(idx_a < 0, np.iinfo(np.int64).max, idx_a.astype(np.int64))
    key_b = np.where(idx_b < 0, np.iinfo(np.int64).max, idx_b.astype(np.int64))
    take_b = (r2_b < r2_a) | ((r2_b == r2_a) & (key_b < key_a))
    return np.where(take_b, r2_b, r2_a), np.where(take_b, idx_b, idx_a)


def chunked(q, soft2, n, tiles, chunks):
    """The same search with the j range cut like the device cuts it: `tiles` layout tiles of 512 slots (slots >= n are
    padding, no candidates) into `chunks` chunks [tiles * c // chunks, tiles * (c + 1) // chunks), each chunk's own
    lexicographic minimum, then the fold over the chunks in index order.  Lattice input (exact r2)."""
    qi = np.asarray(q)[:, :n].astype(np.int64)
    best_r2 = np.full(n, np.inf, np.float32)
    best_idx = np.full(n, -1, np.int32)
    for c in range(chunks):
        lo, hi = TILE * (tiles * c // chunks), min(TILE * (tiles * (c + 1) // chunks), n)
        if hi <= lo:
            continue
        d = qi[:, None, lo:hi] - qi[:, :, None]
        r2 = ((d * d).sum(0).astype(np.float64) + float(soft2)).astype(np.float32)
        own = np.arange(n)
        inside = (own >= lo) & (own < hi)
        r2[own[inside], own[inside] - lo] = np.inf
        k = r2.argmin(1)
        r2_c = r2[own, k]
        idx_c = np.where(np.isinf(r2_c), -1, k + lo).astype(np.int32)
        best_r2, best_idx = lex_min(best_r2, best_idx, r2_c, idx_c)
    return best_idx, best_r2


def threshold(radius, soft2):
    """thr = (float)((double)radius * radius + (double)soft2): a body with r2 <= thr has met its neighbour."""
    return np.float32(float(np.float32(radius)) * float(np.float32(radius)) + float(np.float32(soft2)))


def lattice(n, seed=1):
    """(state dict, soft): n bodies on integer coordinates in [0, 1024]^3 with softening 0.5, so that every r2 is exact in fp32.
      body 0        at the origin, where the padding slots lie; every other body is at least 300 away in each coordinate
      bodies 5, 400 on the same point: a spacing below the softening, r2 = soft^2 like the body's own
      body 7        massless, and the nearest of body 8 (one unit away)
      body 20       has bodies 21 and 300 at the same distance 2: the lowest index wins
      body 30       has bodies 100 and n - 1 at the same distance 3, in different layout tiles (n >= 513)
    (the special bodies exist from n = 513 up; n = 2: the origin and one far body).  Velocities and masses are arbitrary."""
    rng = np.random.default_rng(seed)
    q = rng.integers(300, 1025, size=(3, n)).astype(np.int64)
    q[:, 0] = 0
    if n >= 513:
        q[:, 400] = q[:, 5]
        q[:, 8] = q[:, 7] + np.array([1, 0, 0]) * (1 if q[0, 7] < 1024 else -1)
        q[:, 20] = (500, 600, 700)
        q[:, 21] = (502, 600, 700)
        q[:, 300] = (498, 600, 700)
        q[:, 30] = (700, 400, 900)
        q[:, 100] = (700, 403, 900)
        q[:, n - 1] = (700, 400, 897)
    v = rng.standard_normal((3, n)).astype(np.float32)
    m = rng.uniform(1e20, 2e20, n).astype(np.float32)
    if n >= 513:
        m[7] = 0.0
    s = {"qx": q[0].astype(np.float32), "qy": q[1].astype(np.float32), "qz": q[2].astype(np.float32),
         "vx": v[0], "vy": v[1], "vz": v[2], "m": m}
    return s, np.float32(0.5)


def dense_side(n):
    """The smallest side of a cubic grid with side^3 >= 1.07 n cells."""
    side = 1
    while side ** 3 < 1.07 * n:
        side += 1
    return side


DENSE_PAIRS = ((10, 11), (12, 1500))      # (kept, moved onto it): inside a slot pair, across tiles; (13, n - 2) is the third
DENSE_TRIPLE = (14, 600, 1100)            # one point, three tiles
DENSE_PARTNER = 700                       # the body of tile 1 that body n - 1 sits next to
DENSE_MASSLESS = (12, 700)                # the winners of bodies 1500 and n - 1


def shifted(q_int, seed=1):
    """(q2_int, k): q2 = q_int[:, pi] for a seeded permutation pi of the bodies, the same points held by other bodies, and
    k = q2 - q_int (integers).  With dt = 2^-30 and velocities k 2^30 (exact in fp32) the Hermite predictor takes every body
    from q to q2 exactly: v dt = k, and the acceleration and jerk terms stay far below half an ulp of a coordinate >= 1."""
    q_int = np.asarray(q_int, np.int64)
    pi = np.random.default_rng(seed + 7919).permutation(q_int.shape[1])
    q2 = q_int[:, pi].copy()
    return q2, q2 - q_int


def dense_lattice(n, seed=1):
    """(state dict, soft, q_int): n >= 2049 bodies on n cells of a full cubic grid of spacing 1 (dense_side(n) cells a side,
    coordinates from 3 up), chosen and ordered by a seeded permutation, so that the six neighbours of a cell carry unrelated
    indices: nearly every body has several nearest bodies at the same r2 = 1.25, in several layout tiles, lanes and lane steps.
    Softening 0.5, masses from [1, 2), integer coordinates >= 1: every r2 is exact in fp32.  Written over grid bodies:
      body 0                   at (1, 1, 1), alone: the padding slots at the origin would be its nearest if they were candidates
      bodies n - 1 and 700     one unit apart, 4 and more beyond the grid's far corner: each is the other's only nearest; n - 1
                               lies in the last tile that holds bodies, 700 in tile 1
      bodies 10 = 11, 12 = 1500, 13 = n - 2      on one point each: inside a slot pair, across tiles, with the last but one
      bodies 14 = 600 = 1100   one point in three tiles; for all of these r2 = soft^2 exactly, like the body's own term
      bodies 12 and 700        massless, and the winners of bodies 1500 and n - 1
    The velocities are shifted(q_int, seed)'s k times 2^30: one predictor step of 2^-30 moves the bodies onto q2."""
    assert n >= 2049
    rng = np.random.default_rng(seed)
    side = dense_side(n)
    g = np.arange(side, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1) + 3
    q = cells[:, rng.permutation(side ** 3)[:n]].copy()
    q[:, 0] = 1
    far = side + 6
    q[:, DENSE_PARTNER] = (far, far, far)
    q[:, n - 1] = (far, far, far + 1)
    for a, b in DENSE_PAIRS + ((13, n - 2),):
        q[:, b] = q[:, a]
    for b in DENSE_TRIPLE[1:]:
        q[:, b] = q[:, DENSE_TRIPLE[0]]
    m = rng.uniform(1.0, 2.0, n).astype(np.float32)
    m[list(DENSE_MASSLESS)] = 0.0
    _, k = shifted(q, seed)
    v = (k.astype(np.float64) * 2.0 ** 30).astype(np.float32)
    assert q.min() >= 1 and np.array_equal(v.astype(np.float64), k * 2.0 ** 30)
    s = {"qx": q[0].astype(np.float32), "qy": q[1].astype(np.float32), "qz": q[2].astype(np.float32),
         "vx": v[0], "vy": v[1], "vz": v[2], "m": m}
    return s, np.float32(0.5), q


def r2_matrix(q_int, soft2):
    """fp32 r2 (n, n) of a lattice, +inf on the diagonal; asserts that every value is exact in fp32."""
    qi = np.asarray(q_int, np.int64)
    n = qi.shape[1]
    d2 = np.zeros((n, n), np.int64)
    for c in qi:
        d = c[None, :] - c[:, None]
        d2 += d * d
    want = d2.astype(np.float64) + float(soft2)
    r2 = want.astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), want), "r2 is not exact in fp32"
    r2[np.arange(n), np.arange(n)] = np.inf
    return r2


ROW_BLOCK = 512      # rows of one block of the row-blocked forms: a block's int64 arrays stay at some 50 MB at n = 12 289


def r2_rows(q_int, soft2, lo, hi):
    """Rows [lo, hi) of r2_matrix: fp32 r2 (hi - lo, n), +inf at every body's own index; the same arithmetic, the same assert."""
    qi = np.asarray(q_int, np.int64)
    d2 = np.zeros((hi - lo, qi.shape[1]), np.int64)
    for c in qi:
        d = c[None, :] - c[lo:hi, None]
        d2 += d * d
    want = d2.astype(np.float64) + float(soft2)
    r2 = want.astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), want), "r2 is not exact in fp32"
    r2[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    return r2


def nearest_blocked(q_int, soft2, block=ROW_BLOCK):
    """nearest(exact=True) without the (3, n, n) tensor: r2_matrix's arithmetic in blocks of `block` rows.  Returns
    (index int32, r2 float32), the lowest index among equal r2; a lone body has -1 and +inf."""
    n = np.asarray(q_int).shape[1]
    if n == 1:
        return np.array([-1], np.int32), np.array([np.inf], np.float32)
    idx, best = np.empty(n, np.int32), np.empty(n, np.float32)
    for lo in range(0, n, block):
        r2 = r2_rows(q_int, soft2, lo, min(lo + block, n))
        k = r2.argmin(1)      # argmin returns the first (lowest) index of the minimum
        idx[lo:lo + block], best[lo:lo + block] = k, r2[np.arange(len(k)), k]
    return idx, best


def tie_stats_blocked(q_int, soft2, rows_of, block=ROW_BLOCK):
    """tie_stats, highest_index_wins and later_tile_wins of a lattice without its (n, n) matrix.  rows_of(lo, hi) gives the rows
    [lo, hi) of the candidate values (r2_rows, contact_ref.gap2_rows).  Returns a dict of per-row arrays: idx (the rule's
    winner), val, cnt, span, own, high, later."""
    n = np.asarray(q_int).shape[1]
    tiles = -(-n // TILE)
    out = {k: [] for k in ("idx", "val", "cnt", "span", "own", "high", "later")}
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        values = rows_of(lo, hi)
        rows = np.arange(hi - lo)
        best = values.min(1)
        tie = np.zeros((hi - lo, tiles * TILE), bool)
        tie[:, :n] = values == best[:, None]
        by_tile = tie.reshape(hi - lo, tiles, TILE)
        per_tile = by_tile.any(2)
        span = per_tile.sum(1)
        last_tile = tiles - 1 - per_tile[:, ::-1].argmax(1)      # the last tile that holds a candidate at the minimum ...
        later = last_tile * TILE + by_tile[rows, last_tile].argmax(1)      # ... and its first one: later_tile_wins
        for k, x in (("idx", tie.argmax(1)), ("val", best), ("cnt", tie.sum(1)), ("span", span),
                     ("own", per_tile[rows, np.arange(lo, hi) // TILE] & (span >= 2)),
                     ("high", tiles * TILE - 1 - tie[:, ::-1].argmax(1)), ("later", later)):
            out[k].append(x)
    return {k: np.concatenate(v) for k, v in out.items()}


def tie_stats(values):
    """Of an (n, n) matrix of candidate values (+inf on the diagonal), per row: the number of candidates at the row's minimum,
    the number of layout tiles they lie in, and whether one lies in the row's own tile and another outside it."""
    n = values.shape[0]
    tie = values == values.min(1)[:, None]
    per_tile = np.stack([tie[:, lo:lo + TILE].any(1) for lo in range(0, n, TILE)], 1)
    own = per_tile[np.arange(n), np.arange(n) // TILE]
    span = per_tile.sum(1)
    return tie.sum(1), span, own & (span >= 2)


def highest_index_wins(values):
    """A deliberately wrong rule: the highest index among equal values."""
    n = values.shape[0]
    return (n - 1 - values[:, ::-1].argmin(1)).astype(np.int32)


def later_tile_wins(values):
    """A deliberately wrong rule: every tile's own (correct) minimum, but in the fold over the tiles a later tile wins a tie."""
    n = values.shape[0]
    best, idx = np.full(n, np.inf, values.dtype), np.full(n, -1, np.int32)
    for lo in range(0, n, TILE):
        k = values[:, lo:lo + TILE].argmin(1)
        v = values[np.arange(n), k + lo]
        take = v <= best
        best, idx = np.where(take, v, best), np.where(take, k + lo, idx).astype(np.int32)
    return idx

"""Per-body potential of the Hermite sweeps (option "potential"), restated from include/murbhip.h in fp64, and the probes that
tests/test_potential_host.py (CPU) and tests/test_potential_gpu.py (GPU) share.  numpy only; nothing here touches a device.

    phi_i = sum over real bodies j != i of G m_j / sqrt(|q_j - q_i|^2 + soft^2)

The body's own SLOT is left out, nothing else: another body at the same position counts with G m_j / soft, a massless body
has a phi of its own and adds to nobody's.  The bound everywhere is the project's force bound TOL_F64_MAX, relative to the fp64
phi_i: all terms are positive, so the sum of the term magnitudes is phi_i itself."""
import numpy as np

import hermite_ref as H

TOL_F64_MAX = 2e-6       # tests/helpers/hermite_probe.py, forces
POWER_FACTOR = 10.0      # a probe must show one term at 10 x the bound on 99 % of the bodies
TILE = 512               # slots per layout tile (MURB_TILE_BODIES)
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")


def phi_f64(q, gm, soft, rows=None, want_min=False):
    """fp64 phi of the bodies `rows` (all by default) at positions q (3, n) with G m = gm (n); with want_min also every
    body's smallest term among the bodies of non-zero mass (+inf where there is none).  Blocked over i."""
    q, gm = np.asarray(q, np.float64), np.asarray(gm, np.float64)
    n = q.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    soft2 = float(soft) * float(soft)
    phi, mn = np.zeros(len(rows)), np.full(len(rows), np.inf)
    for lo in range(0, len(rows), 256):
        r = rows[lo:lo + 256]
        d = q[:, None, :] - q[:, r, None]
        with np.errstate(divide="ignore", invalid="ignore"):      # soft == 0: the own slot's term, dropped below
            t = gm[None, :] / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2)
        t[np.arange(len(r)), r] = 0.0      # the own slot, by index
        phi[lo:lo + 256] = t.sum(1)
        if want_min:
            t[:, gm == 0.0] = np.inf
            t[np.arange(len(r)), r] = np.inf
            mn[lo:lo + 256] = t.min(1)
    return (phi, mn) if want_min else phi


def phi_of(s, soft, **kw):
    return phi_f64(H._stack(s, Q), H._gm(s), soft, **kw)


def energy_of(s, phi):
    """w = -1/2 sum_i m_i phi_i in fp64."""
    return -0.5 * float((np.asarray(s["m"], np.float64) * np.asarray(phi, np.float64)).sum())


def rel_err(got, want):
    """|got - want| / want per body; 0 where both are exactly 0 (a lone body)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(want == 0.0, np.where(got == 0.0, 0.0, np.inf), np.abs(got - want) / want)


def state(q, m, v=None):
    q = np.asarray(q, np.float32)
    v = np.zeros_like(q) if v is None else np.asarray(v, np.float32)
    s = {k: np.ascontiguousarray(q[i]) for i, k in enumerate(Q)}
    s.update({k: np.ascontiguousarray(v[i]) for i, k in enumerate(V)})
    s["m"] = np.asarray(m, np.float32)
    return s


# ---- the own term ------------------------------------------------------------------------------------------------------------
OWN_MASS, OWN_SEP, OWN_SOFT = 1e30, 1e10, np.float32(1e6)   # the own term G m / soft is 1e4 x the pair term G m / sep
OWN_SLOTS = (5, 513)


def own_term_pair(n, slots=OWN_SLOTS):
    """(state, soft, the two massive bodies): n = 2, or n >= 514 with the two at `slots` (5 and 513 by default: two layout
    tiles) and every other body massless and at least 1e13 m away from them and from each other."""
    if n == 2:
        return state([[0.0, OWN_SEP], [0.0, 0.0], [0.0, 0.0]], [OWN_MASS, OWN_MASS]), OWN_SOFT, (0, 1)
    k = np.arange(n, dtype=np.float64)
    q = np.stack([1e13 + 1e13 * k, -2e13 - 1e13 * (k % 7), 3e13 + 5e12 * (k % 11)])
    m = np.zeros(n)
    a, b = slots
    q[:, a], q[:, b] = (0.0, 0.0, 0.0), (OWN_SEP, 0.0, 0.0)
    m[a] = m[b] = OWN_MASS
    return state(q, m), OWN_SOFT, (a, b)


# ---- coincident bodies -------------------------------------------------------------------------------------------------------
COINCIDENT_SOFT = np.float32(0.5)
COINCIDENT_PAIRS = ((4, 5), (4, 10), (4, 600))      # the same pair of slots, different lanes of a tile, different tiles


def coincident(pair, n=1024, seed=3):
    """n massive bodies on integer coordinates in [300, 1024]^3 (every difference exact in fp32), body pair[1] moved onto body
    pair[0]: each of the two has the other's G m / soft in its phi."""
    rng = np.random.default_rng(seed)
    q = rng.integers(300, 1025, size=(3, n)).astype(np.float64)
    q[:, pair[1]] = q[:, pair[0]]
    m = rng.uniform(1e8, 2e8, n)
    return state(q, m, rng.standard_normal((3, n))), COINCIDENT_SOFT


# ---- sparse sources ----------------------------------------------------------------------------------------------------------
SPARSE_N, SPARSE_SOFT = 2049, np.float32(0.01)
SPARSE_SOURCES = (0, 5, 100, 511, 512, 700, 777, 1023, 1024, 1300, 1535, 1536, 1801, 2000, 2047, 2048)   # every tile's ends


def tile_sources(n, count):
    """About `count` source slots over ALL layout tiles that hold bodies: every such tile's first and last real slot, the rest
    an even spread over the bodies."""
    tiles = -(-n // TILE)
    ends = {t * TILE for t in range(tiles)} | {min(t * TILE + TILE - 1, n - 1) for t in range(tiles)}
    assert count >= len(ends), "fewer sources than tile ends"
    spread = {int(x) for x in np.linspace(3, n - 3, count - len(ends)).astype(np.int64)}
    return tuple(sorted(ends | spread))


def sparse(n=SPARSE_N, seed=11, velocities=False, sources=0):
    """(state, soft, sources): n bodies in a unit cube, mass (1 ... 2) x 1e10 kg on the sources alone — G m / r of order 1.
    sources = 0: the 16 SPARSE_SOURCES below n; a count: tile_sources(n, count)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 1.0, (3, n))
    m = np.zeros(n)
    src = np.array([x for x in (tile_sources(n, sources) if sources else SPARSE_SOURCES) if x < n], np.int64)
    m[src] = 1e10 * rng.uniform(1.0, 2.0, len(src))
    v = 1e-3 * rng.standard_normal((3, n)) if velocities else None
    return state(q, m, v), SPARSE_SOFT, src


def power(s, soft):
    """Per body: the share of its smallest source term in its phi (inf where it has no source term)."""
    phi, mn = phi_of(s, soft, want_min=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isfinite(mn), mn / phi, np.inf)


# ---- the dense system and the order of the tiles -------------------------------------------------------------------------------
DENSE_N, DENSE_SOFT = 2049, np.float32(0.01)


def dense(n=DENSE_N, seed=23):
    """(state, soft): n bodies in a unit cube, every one with a mass of (1 ... 2) x 1e10 kg and a velocity of order 1e-3:
    every tile adds to every body's phi, so the order in which an fp32 sum receives the tiles shows in its last bits."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 1.0, (3, n))
    m = 1e10 * rng.uniform(1.0, 2.0, n)
    return state(q, m, 1e-3 * rng.standard_normal((3, n))), DENSE_SOFT


def dense_probes(count=64, tile=0):
    """`count` bodies of one tile, spread over its lanes and lane steps."""
    return tile * TILE + np.unique(np.linspace(0, TILE - 1, count).astype(np.int64))


def sweep_terms_f32(s, soft, rows, tiles):
    """float32 terms G m_j * inv_ij of the bodies `rows` against all slots of `tiles` layout tiles, shaped (rows, tiles, 4 lane
    steps, 64 lanes, 2 halves): slot = 512 tile + 128 step + 2 lane + half.  Every operation rounds once to float32 (the
    differences, r2 as one fused chain, 1 / sqrt, the product); the own slot and the padding hold +0."""
    f = np.float32
    n = len(s["m"])
    rows = np.asarray(rows, np.int64)
    q = np.zeros((3, tiles * TILE), f)
    q[:, :n] = np.stack([np.asarray(s[k], f) for k in Q])
    gm = np.zeros(tiles * TILE, f)
    gm[:n] = np.asarray(H._gm(s), f)
    soft2 = float(f(soft) * f(soft))
    out = np.empty((len(rows), tiles * TILE), f)
    for lo in range(0, len(rows), 64):
        r = rows[lo:lo + 64]
        d = (q[:, None, :] - q[:, r, None]).astype(np.float64)      # fp32 differences, held in fp64: their squares are exact
        r2 = (d[0] * d[0] + soft2).astype(f).astype(np.float64)      # one rounding per fused multiply-add
        r2 = (d[1] * d[1] + r2).astype(f).astype(np.float64)
        r2 = (d[2] * d[2] + r2).astype(f).astype(np.float64)
        out[lo:lo + 64] = gm[None, :] * (1.0 / np.sqrt(r2)).astype(f)
        out[np.arange(lo, lo + len(r)), r] = 0.0
    return out.reshape(len(rows), tiles, TILE // 128, 64, 2)


def sweep_phi_f32(terms, rows, chunks):
    """numpy float32 emulation of the FULL potential sweep's summation order on sweep_terms_f32's terms: per chunk
    [tiles c / chunks, tiles (c + 1) / chunks) 128 lane-half accumulators receive the chunk's tiles in layout order, lane steps
    rising, the body's own tile after the others (it is added behind the loop), then the two halves and the lanes are folded;
    the chunks' totals are added in index order.  The fold's pairing is a butterfly; the device's differs in order, not in
    depth."""
    f = np.float32
    rows = np.asarray(rows, np.int64)
    count, tiles = terms.shape[:2]
    own, lanes = rows // TILE, np.arange(64)
    phi = np.zeros(count, f)
    for c in range(chunks):
        t0, t1 = tiles * c // chunks, tiles * (c + 1) // chunks
        acc = np.zeros((count, 64, 2), f)
        for t in range(t0, t1):
            other = (own != t)[:, None, None]
            for step in range(terms.shape[2]):
                acc = acc + np.where(other, terms[:, t, step], f(0.0))      # + 0 changes no bit of a sum of positive terms
        inside = ((own >= t0) & (own < t1))[:, None, None]
        mine = terms[np.arange(count), own]
        for step in range(terms.shape[2]):
            acc = acc + np.where(inside, mine[:, step], f(0.0))
        fold = acc[:, :, 0] + acc[:, :, 1]
        for sft in (1, 2, 4, 8, 16, 32):
            fold = fold + fold[:, lanes ^ sft]
        phi = phi + fold[:, 0]
    assert phi.dtype == f
    return phi


def lane_sums_f32(s, soft, body, order):
    """numpy float32 emulation of one body's phi in one wave of the potential sweep: 64 lanes with two accumulators each (the
    halves of a packed register); lane l takes the slot pairs l, l + 64, l + 128, l + 192 of a tile, one rounded addition per
    term; the tiles come in `order`; the body's own slot adds nothing.  Returns (the 128 lane accumulators, the folded total:
    the two halves added, then a butterfly over the lanes).  1 / sqrt in float32 stands for the device's reciprocal square
    root: the question is the order of the additions alone."""
    f = np.float32
    q = np.stack([np.asarray(s[k], f) for k in Q])
    n = q.shape[1]
    gm = np.asarray(H._gm(s), f)
    soft2 = f(soft) * f(soft)
    acc = np.zeros((64, 2), f)
    lanes = np.arange(64)
    for tile in order:
        for qs in range(TILE // 2 // 64):
            for half in (0, 1):
                j = tile * TILE + 2 * (qs * 64 + lanes) + half
                ok = (j < n) & (j != body)
                jj = np.minimum(j, n - 1)
                d = q[:, jj] - q[:, body, None]
                r2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + soft2
                gi = np.where(ok, gm[jj] * (f(1.0) / np.sqrt(r2)), f(0.0)).astype(f)
                acc[:, half] = acc[:, half] + gi
    fold = acc[:, 0] + acc[:, 1]
    for sft in (32, 16, 8, 4, 2, 1):
        fold = fold + fold[lanes ^ sft]
    return acc, fold[0]

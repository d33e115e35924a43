"""numpy restatement of the pair-separation read-out, written from the text of include/murbsep.h, not from the device code.

For a point p and the bodies j of a subset S: d = q_j - p, d2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, +0))) in fp32 (no softening).
Sum: the distances sqrt(d2) over S.  Histogram: the bin of a pair is read off the bits of its fp32 d2:
    k = (bits(d2) >> sh) - (bits(2^lo_exp) >> sh),   sh = 23 - sub
0 <= k < bins: bin k; k < 0: below; k >= bins, +inf, NaN: above.  A d2 on an edge belongs to the bin above the edge.  A listed
body's own entry (d2 == +0) is struck from "below" and from "pairs".

On integer lattices d2 is exact in fp32 whatever the order of the operations, so the bins are decided exactly."""
import numpy as np

U = 2.0 ** -24      # unit round-off of fp32


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def base_key(lo_exp, sub):
    two = np.float32(2.0) ** np.float32(lo_exp)
    return int(bits(np.array([two]))[0] >> np.uint32(23 - sub))


def valid(lo_exp, sub, bins):
    """The header's ranges, and a finite top edge."""
    if not (-126 <= lo_exp <= 127 and 0 <= sub <= 6 and 1 <= bins <= 1022):
        return False
    return base_key(lo_exp, sub) + bins < (255 << sub)


def edges2(lo_exp, sub, bins):
    """bins + 1 exact float32 edges in d2: float_from_bits((base + k) << sh)."""
    key = np.arange(bins + 1, dtype=np.uint64) + np.uint64(base_key(lo_exp, sub))
    return (key << np.uint64(23 - sub)).astype(np.uint32).view(np.float32)


def edges_r(lo_exp, sub, bins):
    return np.sqrt(edges2(lo_exp, sub, bins).astype(np.float64))


def bin_of(d2, lo_exp, sub, bins, rule=None):
    """int64 per entry of the float32 array d2: -1 below, bins above, else the bin.
    rule None: the header's.  The deliberately wrong rules:
      "edge below"   a pair on an edge goes to the bin below the edge
      "steps in r"   bins of equal width in r between the lowest and the top edge"""
    d2 = np.ascontiguousarray(d2, np.float32)
    if rule is None:
        k = (bits(d2) >> np.uint32(23 - sub)).astype(np.int64) - base_key(lo_exp, sub)
        return np.clip(k, -1, bins)
    e2 = edges2(lo_exp, sub, bins)
    if rule == "edge below":
        k = np.searchsorted(e2, d2, side="left").astype(np.int64) - 1
        return np.where(np.isnan(d2), bins, np.clip(k, -1, bins))
    if rule == "steps in r":
        r, er = np.sqrt(d2.astype(np.float64)), np.sqrt(e2.astype(np.float64))
        k = np.floor((r - er[0]) / (er[-1] - er[0]) * bins)
        return np.where(np.isnan(d2), bins, np.clip(np.nan_to_num(k, posinf=bins), -1, bins)).astype(np.int64)
    raise ValueError(rule)


def bin_by_edges(d2, lo_exp, sub, bins):
    """The header's rule stated through the edges instead of the bits: the last edge that is <= d2."""
    d2 = np.ascontiguousarray(d2, np.float32)
    k = np.searchsorted(edges2(lo_exp, sub, bins), d2, side="right").astype(np.int64) - 1
    return np.where(np.isnan(d2), bins, k)


def d2_lattice(q_int, p_int=None):
    """float32 d2 (points, n) of integer points against integer bodies (the bodies themselves when p_int is None); asserts that
    every value is exact in fp32."""
    qi = np.asarray(q_int, np.int64)
    pi = qi if p_int is None else np.asarray(p_int, np.int64)
    d2 = np.zeros((pi.shape[1], qi.shape[1]), np.int64)
    for c, pc in zip(qi, pi):
        d = c[None, :] - pc[:, None]
        d2 += d * d
    out = d2.astype(np.float32)
    assert np.array_equal(out.astype(np.int64), d2), "d2 is not exact in fp32"
    return out


def histogram(d2, lo_exp, sub, bins, member=None, own=None, rule=None):
    """(hist uint64 (bins), {"pairs", "below", "above"}) of the rows of d2 (points, n) against the bodies the mask lets in.
    own: per point its own body index, or None (points of the caller's): that body's entry is left out when it is in S.
    rule "own counted": the deliberately wrong rule that keeps it; the other rules are bin_of's."""
    d2 = np.asarray(d2, np.float32)
    points, n = d2.shape
    inside = np.ones(n, bool) if member is None else np.asarray(member) != 0
    keep = np.broadcast_to(inside[None, :], d2.shape).copy()
    if own is not None and rule != "own counted":
        keep[np.arange(points), np.asarray(own)] = False
    k = bin_of(d2[keep], lo_exp, sub, bins, None if rule == "own counted" else rule)
    hist = np.bincount(k[(k >= 0) & (k < bins)], minlength=bins).astype(np.uint64)
    return hist, {"pairs": int(keep.sum()), "below": int((k < 0).sum()), "above": int((k >= bins).sum())}


def sums64(q, points=None, member=None, own=None):
    """fp64 sum of distances per point from the float32 coordinates: q (3, n) bodies, points (3, P) (None: the bodies)."""
    q = np.asarray(q, np.float32).astype(np.float64)
    p = q if points is None else np.asarray(points, np.float32).astype(np.float64)
    inside = np.ones(q.shape[1], bool) if member is None else np.asarray(member) != 0
    d2 = np.zeros((p.shape[1], int(inside.sum())))
    for c, pc in zip(q[:, inside], p):
        d = c[None, :] - pc[:, None]
        d2 += d * d
    return np.sqrt(d2).sum(1)


def sum_bound(tiles, chunks):
    """The relative bound of a sum against fp64: k u / (1 - k u) with k = 5 + 4 ceil(tiles / chunks) + 8: five roundings of d2
    halved by the root plus the root's 1 ulp, one add per lane step of the longest chunk, the fold.  All terms are positive."""
    k = 5 + 4 * -(-tiles // chunks) + 8
    return k * U / (1.0 - k * U)


def positions(s):
    return np.stack([s["qx"], s["qy"], s["qz"]])


def mean_separation(s, member=None):
    """The members' fp64 sums added in index order over M (M - 1); NaN for fewer than 2 members."""
    inside = np.ones(len(s["m"]), bool) if member is None else np.asarray(member) != 0
    m = int(inside.sum())
    if m < 2:
        return float("nan")
    q = positions(s)[:, inside]
    total = 0.0
    for v in sums64(q):
        total += float(v)
    return total / (m * (m - 1.0))


def q_parameter(s, mean_edge, member=None):
    """(q, m_bar, s_bar, radius) in the 3-D convention from the tree's mean edge length: R the largest fp64 distance of a member
    from the members' unweighted mean position, s_bar = mean separation / R, m_bar = mean edge / ((M^2 4/3 pi R^3)^(1/3) / (M - 1))."""
    inside = np.ones(len(s["m"]), bool) if member is None else np.asarray(member) != 0
    m = int(inside.sum())
    if m < 2:
        return (float("nan"),) * 4
    q = positions(s)[:, inside].astype(np.float64)
    d = q - q.mean(axis=1, keepdims=True)
    radius = float(np.sqrt((d * d).sum(0)).max())
    s_bar = mean_separation(s, member) / radius
    m_bar = mean_edge / ((m * m * 4.0 / 3.0 * np.pi * radius ** 3) ** (1.0 / 3.0) / (m - 1.0))
    return m_bar / s_bar, m_bar, s_bar, radius

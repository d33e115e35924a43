"""numpy restatement of the bound-pair read-out, written from the text of include/murbbind.h, not from the device code.

Per point the candidate with the smallest h = w2 / 2 - (gm_j + gm_p) / sqrt(d2 + soft2) under the total order (h as fp32,
index); candidates are all real bodies but the point's skipped slot (massless ones included, never the padding behind the n
bodies); none: -1 / +inf.  A pair is mutual when each is the other's partner, bound when mutual with h < 0.

On a lattice (integer positions and velocities, equal masses) r2, w2 and gs are exact in fp32, so the fp32 h of a candidate is
a function of its CLASS, the exact integers (d2, w2), whatever v_rsq_f32 returns: equal classes give equal bits, and the partner
is "the lowest index of the minimal class" as long as distinct classes lie further apart than the fp32 error (the tests pin
that gap)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as K           # noqa: E402
import nearest_ref as NR      # noqa: E402

TILE = NR.TILE
TWO_PI = 6.283185307179586
ELEMENT_KEYS = ("a", "e", "period", "h", "energy", "r")


# ------------------------------------------------------------------------------------------------------------------ lattices
def bind_lattice(n, seed=11):
    """(state dict, soft, g, q_int, v_int): nearest_ref.dense_lattice(n)'s points, all masses 1, G = 1, softening 0.5, per-body
    integer velocities drawn from {-1, 0, 1}^3 with a fixed seed.  gm = 1 and gs = 2 for every pair, exactly."""
    s, soft, q = NR.dense_lattice(n)
    v = np.random.default_rng(seed).integers(-1, 2, size=(3, n)).astype(np.int64)
    s = dict(s)
    for k, c in zip(("vx", "vy", "vz"), v):
        s[k] = c.astype(np.float32)
    s["m"] = np.ones(n, np.float32)
    return s, np.float32(soft), np.float32(1.0), np.asarray(q, np.int64), v


def class_rows(q_int, v_int, lo, hi):
    """The classes of rows [lo, hi): exact integers d2, w2 (hi - lo, n)."""
    d2 = np.zeros((hi - lo, q_int.shape[1]), np.int64)
    w2 = np.zeros_like(d2)
    for c in np.asarray(q_int, np.int64):
        d = c[None, :] - c[lo:hi, None]
        d2 += d * d
    for c in np.asarray(v_int, np.int64):
        d = c[None, :] - c[lo:hi, None]
        w2 += d * d
    return d2, w2


def lattice_stats(q_int, v_int, soft2=0.25, gs=2.0, block=NR.ROW_BLOCK):
    """Per body of a lattice, in row blocks: idx (the rule's partner: the lowest index of the minimal class), key (the fp64 h of
    that class), scale (w2 / 2 + gs / rs of it), gap (the next class's fp64 h minus the minimal one, relative to scale), cnt
    (candidates in the minimal class), span (layout tiles they lie in), and three deliberately wrong rules: nearest (the nearest
    neighbour, lowest index), high (the highest index of the minimal class), later (a later tile wins a tie)."""
    n = q_int.shape[1]
    tiles = -(-n // TILE)
    out = {k: [] for k in ("idx", "key", "scale", "gap", "cnt", "span", "nearest", "high", "later")}
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        rows, own = np.arange(hi - lo), np.arange(lo, hi)
        d2, w2 = class_rows(q_int, v_int, lo, hi)
        rs = np.sqrt(d2.astype(np.float64) + float(soft2))
        key = 0.5 * w2 - gs / rs
        key[rows, own] = np.inf
        k = key.argmin(1)
        tie = np.zeros((hi - lo, tiles * TILE), bool)
        tie[:, :n] = (d2 == d2[rows, k][:, None]) & (w2 == w2[rows, k][:, None])
        tie[rows, own] = False
        rest = np.where(tie[:, :n], np.inf, key)
        scale = 0.5 * w2[rows, k] + gs / rs[rows, k]
        by_tile = tie.reshape(hi - lo, tiles, TILE)
        per_tile = by_tile.any(2)
        last_tile = tiles - 1 - per_tile[:, ::-1].argmax(1)
        near = d2.astype(np.float64)
        near[rows, own] = np.inf
        for name, x in (("idx", tie.argmax(1)), ("key", key[rows, k]), ("scale", scale), ("gap", (rest.min(1) - key[rows, k]) / scale),
                        ("cnt", tie.sum(1)), ("span", per_tile.sum(1)), ("nearest", near.argmin(1)),
                        ("high", tiles * TILE - 1 - tie[:, ::-1].argmax(1)),
                        ("later", last_tile * TILE + by_tile[rows, last_tile].argmax(1))):
            out[name].append(x)
    res = {k: np.concatenate(v) for k, v in out.items()}
    for k in ("idx", "nearest", "high", "later"):
        res[k] = res[k].astype(np.int32)
    return res


# -------------------------------------------------------------------------------------------------------------- general states
def gm_of(s, g):
    """The fp32 G * m the upload folds into the records: one fp32 multiply."""
    return (np.float32(g) * np.asarray(s["m"], np.float32)).astype(np.float32)


def key_matrix(s, g, soft):
    """(key, scale): the fp64 key h (n, n) of a state's fp32 values, +inf on the diagonal, and w2 / 2 + gs / rs."""
    q = np.stack([s["qx"], s["qy"], s["qz"]]).astype(np.float64)
    v = np.stack([s["vx"], s["vy"], s["vz"]]).astype(np.float64)
    n = q.shape[1]
    d2, w2 = np.zeros((n, n)), np.zeros((n, n))
    for c in q:
        d = c[None, :] - c[:, None]
        d2 += d * d
    for c in v:
        d = c[None, :] - c[:, None]
        w2 += d * d
    gm = gm_of(s, g).astype(np.float64)
    gs = gm[None, :] + gm[:, None]
    rs = np.sqrt(d2 + float(np.float32(soft) * np.float32(soft)))
    key = 0.5 * w2 - gs / rs
    key[np.arange(n), np.arange(n)] = np.inf
    return key, 0.5 * w2 + gs / rs


def pair_lists(partner, h):
    """(mutual, bound): arrays (pairs, 2) of i < j ascending in i: each the other's partner; and those with h[i] < 0."""
    partner = np.asarray(partner)
    i = np.arange(partner.shape[0])
    ok = partner > i
    ok[ok] = partner[partner[ok]] == i[ok]
    mutual = np.stack([i[ok], partner[ok]], 1)
    bound = mutual[np.asarray(h)[mutual[:, 0]] < 0] if len(mutual) else mutual
    return mutual, bound


def elements(g, soft, qi, vi, mi, qj, vj, mj):
    """The elements chain of include/murbbind.h in numpy fp64, one operation per step: arrays (pairs, 6) {a, e, P, h64, E_b, r}.
    qi, vi, qj, vj: (3, pairs) fp32; mi, mj: (pairs,) fp32."""
    f32 = lambda x: np.atleast_1d(np.asarray(x, np.float32))      # noqa: E731
    qi, vi, qj, vj = (np.asarray(x, np.float32).reshape(3, -1) for x in (qi, vi, qj, vj))
    mi, mj = f32(mi), f32(mj)
    soft2 = np.float64(np.float32(soft) * np.float32(soft))
    gmi, gmj = (np.float32(g) * mi).astype(np.float32), (np.float32(g) * mj).astype(np.float32)
    d = qj.astype(np.float64) - qi.astype(np.float64)
    w = vj.astype(np.float64) - vi.astype(np.float64)
    with np.errstate(all="ignore"):
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        w2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        r = np.sqrt(d2)
        rs = np.sqrt(d2 + soft2)
        GM = gmi.astype(np.float64) + gmj.astype(np.float64)
        h64 = 0.5 * w2 - GM / rs
        a = GM / (-2.0 * h64)
        cx, cy, cz = d[1] * w[2] - d[2] * w[1], d[2] * w[0] - d[0] * w[2], d[0] * w[1] - d[1] * w[0]
        L2 = (cx * cx + cy * cy) + cz * cz
        e = np.sqrt(np.fmax(0.0, 1.0 + ((2.0 * h64) * L2) / (GM * GM)))      # fmax: 0 where the argument is NaN
        P = TWO_PI * np.sqrt(((a * a) * a) / GM)
        ms = mi.astype(np.float64) + mj.astype(np.float64)
        mu = np.where(ms == 0.0, 0.0, (mi.astype(np.float64) * mj.astype(np.float64)) / np.where(ms == 0.0, 1.0, ms))
    return np.stack([a, e, P, h64, mu * h64, r], 1)


def state_elements(s, g, soft, pairs):
    """elements() of the listed pairs (pairs, 2) of a state."""
    q = np.stack([s["qx"], s["qy"], s["qz"]]).astype(np.float32)
    v = np.stack([s["vx"], s["vy"], s["vz"]]).astype(np.float32)
    i, j = np.asarray(pairs, np.int64).reshape(-1, 2).T
    return elements(g, soft, q[:, i], v[:, i], s["m"][i], q[:, j], v[:, j], s["m"][j])


def census(partner, h, bound, elems):
    """out8 of include/murbbind.h from the arrays of murbbind_of, the bound list and its elements; the sum by math.fsum."""
    partner, h = np.asarray(partner), np.asarray(h)
    mutual, _ = pair_lists(partner, h)
    out = np.full(8, np.nan)
    out[0], out[1] = len(bound), math.fsum(elems[:, 4]) if len(bound) else 0.0
    if len(bound):
        k = int(np.argmin(elems[:, 4]))      # the first (lowest i) of the smallest E_b
        out[2], out[3], out[4], out[5] = bound[k, 0], bound[k, 1], elems[k, 4], elems[:, 0].min()
    out[6] = int(((partner >= 0) & (h < 0)).sum())
    out[7] = len(mutual)
    return out


# ------------------------------------------------------------------------------------------------------------ planted systems
def kepler_pair(m1, m2, a, e, g=1.0, phase=0.0):
    """Relative position and velocity (3,), (3,) of a Kepler orbit of semi-major axis a and eccentricity e in the x-y plane at true
    anomaly `phase`, and each body's offset from the centre of mass: (q1, v1, q2, v2)."""
    M = m1 + m2
    p = a * (1.0 - e * e)
    r = p / (1.0 + e * math.cos(phase))
    k = math.sqrt(g * M / p)
    d = np.array([r * math.cos(phase), r * math.sin(phase), 0.0])
    w = np.array([-k * math.sin(phase), k * (e + math.cos(phase)), 0.0])
    return -d * m2 / M, -w * m2 / M, d * m1 / M, w * m1 / M


def planted(n=3000):
    """(state, soft, g, info): knn_ref.plummer(n) with an equal-mass binary (a = 0.01, e = 0.5) and a hierarchical triple (inner
    a = 0.005, e = 0.2; the outer body on a circle of 0.05 about the inner pair, in phase with it, so that the outer body moves
    along with one inner body and is bound to it: h about -0.2 against the inner pair's -1.3) appended, both far above the
    softening 1e-3 and placed 15 scale lengths off the cluster's centre on either side.  Their masses are 20 cluster bodies' each.
    info: binary (i, j), inner (i, j), outer."""
    s, soft = K.plummer(n)
    g = 1.0
    m = 20.0 / n
    centre = np.array([40.0, -25.0, 10.0])
    add_q, add_v, add_m = [], [], []
    q1, v1, q2, v2 = kepler_pair(m, m, 0.01, 0.5, g, 1.0)
    at = centre + np.array([15.0, 0.0, 0.0])
    add_q += [at + q1, at + q2]; add_v += [v1, v2]; add_m += [m, m]
    q1, v1, q2, v2 = kepler_pair(m, m, 0.005, 0.2, g, 0.5)
    o1q, o1v, o2q, o2v = kepler_pair(2 * m, m, 0.05, 0.0, g, 0.5)
    at = centre - np.array([15.0, 0.0, 0.0])
    add_q += [at + o1q + q1, at + o1q + q2, at + o2q]; add_v += [o1v + v1, o1v + v2, o2v]; add_m += [m, m, m]
    q = np.concatenate([np.stack([s["qx"], s["qy"], s["qz"]]), np.array(add_q).T.astype(np.float32)], 1)
    v = np.concatenate([np.stack([s["vx"], s["vy"], s["vz"]]), np.array(add_v).T.astype(np.float32)], 1)
    out = {"qx": q[0], "qy": q[1], "qz": q[2], "vx": v[0], "vy": v[1], "vz": v[2],
           "m": np.concatenate([s["m"], np.array(add_m, np.float32)])}
    out = {k: np.ascontiguousarray(x, np.float32) for k, x in out.items()}
    return out, soft, g, {"binary": (n, n + 1), "inner": (n + 2, n + 3), "outer": n + 4}

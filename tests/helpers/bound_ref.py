"""numpy fp64 restatement of include/murbbound.h, written from the header: the direct masked potential, one unbinding round,
the whole loop (with the deliberately wrong rules the host test tells apart) and the Lagrangian radii; and the two fixtures
the tests share.  G = 1, total mass 1, soft = 0.01."""
from functools import lru_cache

import numpy as np

Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
G, SOFT = 1.0, np.float32(0.01)
TOL_F64_MAX = 2e-6       # tests/test_gpu_parity.py: the sweeps' fp32 sums against fp64
BAND = 2 * TOL_F64_MAX   # bodies with |e| <= BAND * phi are left out of a round's set comparison
A_SPHERE, A_FAST, A_CLUMP = 1536, 64, 128
OUT16 = ("members", "mass", "rounds", "converged", "vx", "vy", "vz", "cx", "cy", "cz", "kinetic", "potential", "virial_ratio",
         "removed", "unbound_bodies")


# ------------------------------------------------------------------------------------------------------------------- fixtures
def plummer(n, rng, mass=1.0, size=1.0):
    """(q (3, n), v (3, n), m (n)) in fp64: a Plummer sphere of total mass `mass` and scale radius size * 3 pi / 16 (virial units
    at mass = size = 1) in equilibrium with G = 1, cut at 10 scale radii."""
    a = size * 3.0 * np.pi / 16.0
    r = np.empty(0)
    while len(r) < n:
        u = rng.uniform(1e-6, 1.0, 2 * n)
        x = a / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
        r = np.concatenate([r, x[x < 10.0 * a]])
    r = r[:n]

    def directions(count):
        z = rng.uniform(-1.0, 1.0, count)
        t = rng.uniform(0.0, 2.0 * np.pi, count)
        s = np.sqrt(1.0 - z * z)
        return np.stack([s * np.cos(t), s * np.sin(t), z])
    f = np.empty(0)
    while len(f) < n:      # the speed as a fraction of the escape speed: g(f) = f^2 (1 - f^2)^3.5, at most 0.1 below
        x, y = rng.uniform(0.0, 1.0, 4 * n), rng.uniform(0.0, 0.1, 4 * n)
        f = np.concatenate([f, x[y < x * x * (1.0 - x * x) ** 3.5]])
    speed = f[:n] * np.sqrt(2.0 * G * mass) * (r * r + a * a) ** -0.25
    return directions(n) * r, directions(n) * speed, np.full(n, mass / n)


def _state(q, v, m):
    s = {"m": m.astype(np.float32)}
    for keys, arr in ((Q, q), (V, v)):
        for k, c in zip(keys, arr):
            s[k] = c.astype(np.float32)
    return s


@lru_cache(maxsize=None)
def fixture_a(seed=4):
    """n = 1664 (a ragged fourth tile): a Plummer sphere of 1536 bodies (mass 0.92) of which the first 64 have their velocities
    times 4, then a clump of 128 (a Plummer sphere 0.2 times the size, mass 0.08) at x = 30 moving at v_x = 3.  Do not modify."""
    rng = np.random.default_rng(seed)
    q, v, m = plummer(A_SPHERE, rng, mass=0.92)
    v[:, :A_FAST] *= 4.0
    cq, cv, cm = plummer(A_CLUMP, rng, mass=0.08, size=0.2)
    cq[0] += 30.0
    cv[0] += 3.0
    return _state(np.concatenate([q, cq], 1), np.concatenate([v, cv], 1), np.concatenate([m, cm]))


@lru_cache(maxsize=None)
def fixture_b(seed=12):
    """n = 1200: a Plummer sphere with its velocities times 1.3.  Do not modify."""
    q, v, m = plummer(1200, np.random.default_rng(seed))
    return _state(q, v * 1.3, m)


def clump_mask():
    mask = np.zeros(A_SPHERE + A_CLUMP, bool)
    mask[A_SPHERE:] = True
    return mask


# ------------------------------------------------------------------------------------------------------------------ potential
def gm_of(s, g=G):
    """The records' fp32 G * m, widened."""
    return (np.float32(g) * s["m"].astype(np.float32)).astype(np.float64)


def potential(s, g=G, soft=SOFT, member=None, points=None, skip=None, self_term=False):
    """phi in fp64 at the bodies themselves (points None: each with itself left out) or at `points` (3, count) with the bodies
    skip[p] >= 0 left out: the sum of G m_j / sqrt(d^2 + soft^2) over the bodies the mask lets in.  self_term: nothing is left
    out (a deliberately wrong rule)."""
    q = np.stack([s[k] for k in Q]).astype(np.float64)
    n = q.shape[1]
    gm = gm_of(s, g)
    if member is not None:
        gm = np.where(np.asarray(member) != 0, gm, 0.0)
    if points is None:
        p, skip = q, np.arange(n)
    else:
        p = np.asarray(points, np.float32).astype(np.float64)
    soft2 = float(np.float32(soft) * np.float32(soft))
    d2 = np.full((p.shape[1], n), soft2)
    for c in range(3):
        d2 += (q[c][None, :] - p[c][:, None]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        w = gm[None, :] / np.sqrt(d2)
    if skip is not None and not self_term:
        skip = np.asarray(skip)
        rows = np.nonzero(skip >= 0)[0]
        w[rows, skip[rows]] = 0.0
    return w.sum(1)


# ------------------------------------------------------------------------------------------------------------------ unbinding
def frame(s, member):
    """V = (sum over the set of m v) / (sum of m), 0 when that mass is 0."""
    m = np.where(member, s["m"].astype(np.float64), 0.0)
    mass = m.sum()
    if mass == 0.0:
        return np.zeros(3)
    return np.array([(m * s[k].astype(np.float64)).sum() for k in V]) / mass


def energy(s, frame_v, phi):
    """e = 0.5 * ((wx*wx + wy*wy) + wz*wz) - phi with w = (double)v - V."""
    w = [s[k].astype(np.float64) - frame_v[c] for c, k in enumerate(V)]
    return 0.5 * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) - np.asarray(phi, np.float64)


def one_round(s, member, frame_v=None, g=G, soft=SOFT, rule="right"):
    """(next set, e, V, phi) of one round from the set `member` (bool).  rule: "right", or a deliberately wrong one: "self" keeps
    the self term, "nomask" takes phi from all bodies, "readmit" lets dropped bodies back in."""
    member = np.asarray(member) != 0
    v = frame(s, member) if frame_v is None else np.asarray(frame_v, np.float64)
    phi = potential(s, g, soft, None if rule == "nomask" else member, self_term=rule == "self")
    e = energy(s, v, phi)
    keep = e < 0.0          # NaN is dropped
    return (keep if rule == "readmit" else member & keep), e, v, phi


def unbind(s, start=None, frame_v=None, max_iter=64, g=G, soft=SOFT, rule="right"):
    """The whole call: dict with member, e (all bodies against the final set and its V), v, phi, rounds, converged, dropped (per
    round) and the out16 fields.  rule "frame": V is that of the start set throughout (wrong)."""
    n = len(s["m"])
    member = np.ones(n, bool) if start is None else np.asarray(start) != 0
    first = int(member.sum())
    fixed = frame_v if rule != "frame" else frame(s, member)
    rounds, converged, dropped = 0, False, []
    while rounds < max_iter and not converged:
        new, e, v, phi = one_round(s, member, fixed, g, soft, rule if rule != "frame" else "right")
        rounds += 1
        converged = np.array_equal(new, member)
        dropped.append(int(member.sum()) - int(new.sum()))
        member = new
    if not converged:
        v = frame(s, member) if fixed is None else np.asarray(fixed, np.float64)
        phi = potential(s, g, soft, member)
        e = energy(s, v, phi)
    m = np.where(member, s["m"].astype(np.float64), 0.0)
    w2 = sum((s[k].astype(np.float64) - v[c]) ** 2 for c, k in enumerate(V))
    kin, pot = (0.5 * m * w2).sum(), -0.5 * (m * phi).sum()
    empty = not member.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        centre = np.array([(m * s[k].astype(np.float64)).sum() for k in Q]) / m.sum()
        ratio = kin / abs(pot)
    return {"member": member, "e": e, "v": np.full(3, np.nan) if empty else v, "phi": phi, "rounds": rounds, "converged": converged,
            "dropped": dropped, "members": int(member.sum()), "mass": m.sum(), "centre": centre, "kinetic": kin, "potential": pot,
            "virial_ratio": ratio, "removed": first - int(member.sum()), "unbound_bodies": int((e >= 0.0).sum())}


def in_band(e, phi):
    """Bodies whose membership fp32 rounding of phi may decide: |e| <= 2 * TOL_F64_MAX * phi."""
    return np.abs(e) <= BAND * np.abs(phi)


# ---------------------------------------------------------------------------------------------------------------------- radii
def radii(q, m, fractions, centre, member=None):
    """Lagrangian radii: the members ordered by (d2, index); sqrt(d2) of the first body at which the running mass, in that order,
    reaches the fraction of the total of the same order; NaN when that total is 0."""
    q = [np.asarray(x, np.float32).astype(np.float64) for x in q]
    m = np.asarray(m, np.float32).astype(np.float64)
    idx = np.arange(len(m)) if member is None else np.nonzero(np.asarray(member) != 0)[0]
    d = [q[c][idx] - float(centre[c]) for c in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    order = np.lexsort((idx, d2))
    run = np.zeros(len(idx))
    total = 0.0
    for k, o in enumerate(order):      # a sequential sum: np.cumsum's order is its own
        total += m[idx[o]]
        run[k] = total
    out = np.full(len(fractions), np.nan)
    if not total > 0.0:
        return out
    for f, frac in enumerate(fractions):
        out[f] = np.sqrt(d2[order[np.nonzero(run >= frac * total)[0][0]]])
    return out

"""Field at arbitrary points (murbfield_at / murbfield_of), restated from include/murbfield.h, and the inputs that
tests/test_field_host.py (CPU) and tests/test_field_gpu.py (GPU) share.  numpy only; nothing here touches a device.

    d = q_j - p    w = v_j - pv    r2 = |d|^2 + soft^2          over every real body j != skip_p:
    a_p = sum G m_j d r2^(-3/2)     j_p = sum G m_j (w - 3 (d.w) d / r2) r2^(-3/2)     phi_p = sum G m_j r2^(-1/2)

The skipped body is left out by INDEX, nothing else: another body at the same place counts.

The bound (bound_of / check): the jerk bound of tests/test_hermite_gpu.py, for a, j and phi alike.  A point's error is scaled by
the sum of the magnitudes of its terms and bounded by C * 2^-24 with C = 4 x what a plain numpy float32 evaluation of the same
formula (128 partial sums per point, then added) attains against fp64 on the same inputs — the largest figure over the points
of the case, per quantity, computed on the CPU and never from a device's output.  The factor 4 covers v_rsq_f32's 1 ulp
against numpy's correctly rounded 1 / sqrt and a different summation tree."""
import numpy as np

import hermite_ref as H
import potential_ref as PR

Q, V = PR.Q, PR.V
TILE = PR.TILE
KEYS = ("ax", "ay", "az", "jx", "jy", "jz", "phi")
POWER_FACTOR = PR.POWER_FACTOR
U24 = 2.0 ** -24


def _eval(points, pvel, skip, q, v, gm, soft, dtype, nsplit, want_abs, block=256):
    points = np.asarray(points, dtype).reshape(3, -1)
    count = points.shape[1]
    pvel = np.zeros((3, count), dtype) if pvel is None else np.asarray(pvel, dtype).reshape(3, -1)
    skip = np.full(count, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    q, v, gm = np.asarray(q, dtype), np.asarray(v, dtype), np.asarray(gm, dtype)
    n = q.shape[1]
    soft2 = dtype(soft) * dtype(soft)
    a, j, phi = np.zeros((3, count), dtype), np.zeros((3, count), dtype), np.zeros(count, dtype)
    ab = {k: np.zeros(count) for k in ("a", "j", "phi")}
    bounds = [(n * k) // nsplit for k in range(nsplit + 1)]
    cols = np.arange(n)

    def fold(terms):
        if nsplit == 1:
            return terms.sum(1, dtype=dtype)
        out = np.zeros(terms.shape[0], dtype)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if hi > lo:
                out = out + terms[:, lo:hi].sum(1, dtype=dtype)
        return out

    def norm64(t):
        t = [np.asarray(x, np.float64) for x in t]
        return np.sqrt(t[0] ** 2 + t[1] ** 2 + t[2] ** 2)

    for i0 in range(0, count, block):
        i1 = min(count, i0 + block)
        keep = cols[None, :] != skip[i0:i1, None]
        d = q[:, None, :] - points[:, i0:i1, None]
        w = v[:, None, :] - pvel[:, i0:i1, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
            inv = dtype(1.0) / np.sqrt(r2)
            inv2 = inv * inv
            g = np.where(keep, gm[None, :] * inv, dtype(0.0))           # the skipped body: by index
            s = g * inv2
            c = dtype(-3.0) * ((d[0] * w[0] + d[1] * w[1] + d[2] * w[2]) * inv2)
            ta = [np.where(keep, s * d[k], dtype(0.0)) for k in range(3)]
            tj = [np.where(keep, s * (w[k] + c * d[k]), dtype(0.0)) for k in range(3)]
        for k in range(3):
            a[k, i0:i1], j[k, i0:i1] = fold(ta[k]), fold(tj[k])
        phi[i0:i1] = fold(g)
        if want_abs:
            ab["a"][i0:i1], ab["j"][i0:i1] = norm64(ta).sum(1), norm64(tj).sum(1)
            ab["phi"][i0:i1] = np.asarray(g, np.float64).sum(1)
    return a, j, phi, ab


def field_f64(points, pvel, skip, state, soft, want_abs=True, block=256):
    """fp64 (a (3, P), j (3, P), phi (P), abs): the field of `state`'s bodies at `points` (3, P) moving with `pvel` (3, P or None:
    at rest), body skip[k] (or -1 / None: nobody) left out for point k.  abs: dict a, j, phi of the per-point sums of the terms'
    magnitudes (with want_abs).  block: points evaluated at a time (memory alone; no value depends on it)."""
    return _eval(points, pvel, skip, H._stack(state, Q), H._stack(state, V), H._gm(state), soft, np.float64, 1, want_abs, block)


def field_f32(points, pvel, skip, state, soft, nsplit=128, block=256):
    """The same formula in plain numpy float32, `nsplit` partial sums per point, then added (hermite_ref.acc_jerk_f32's shape)."""
    a, j, phi, _ = _eval(points, pvel, skip, H._stack(state, Q, np.float32), H._stack(state, V, np.float32), H._gm(state, np.float32),
                         soft, np.float32, nsplit, False, block)
    return a, j, phi


def scaled_errors(got, ref):
    """dict a, j, phi of per-point |got - fp64| / (sum of the magnitudes of the point's terms); got: a dict with KEYS or a tuple
    (a, j, phi); ref: field_f64's result.  0 where a point has no terms and the value is exactly 0, inf where it is not."""
    if isinstance(got, dict):
        got = (np.stack([got[k] for k in KEYS[:3]]), np.stack([got[k] for k in KEYS[3:6]]), got["phi"])
    a, j, phi, ab = ref
    out = {}
    for name, g, r in (("a", got[0], a), ("j", got[1], j), ("phi", np.asarray(got[2])[None], phi[None])):
        diff = np.sqrt(((np.asarray(g, np.float64) - r) ** 2).sum(0))
        with np.errstate(invalid="ignore", divide="ignore"):
            out[name] = np.where(ab[name] == 0.0, np.where(diff == 0.0, 0.0, np.inf), diff / ab[name])
    return out


def bound_of(points, pvel, skip, state, soft, ref=None, block=256):
    """(ref, C): field_f64's result and, per quantity, C of the bound in units of 2^-24 (the module's docstring)."""
    ref = field_f64(points, pvel, skip, state, soft, block=block) if ref is None else ref
    e = scaled_errors(field_f32(points, pvel, skip, state, soft, block=block), ref)
    return ref, {k: 4.0 * float(np.max(v, initial=0.0)) / U24 for k, v in e.items()}


def check(got, ref, c, what, rows=None):
    """Print the figures of `got` beside the bound and assert them; rows: the points of ref that got holds (all by default)."""
    if rows is not None:
        rows = np.asarray(rows)
        a, j, phi, ab = ref
        ref = (a[:, rows], j[:, rows], phi[rows], {k: v[rows] for k, v in ab.items()})
    e = scaled_errors(got, ref)
    fig = {k: float(np.max(v, initial=0.0)) / U24 for k, v in e.items()}
    print(f"{what}: scaled error in 2^-24: " + ", ".join(f"{k} {fig[k]:.2f} (bound {c[k]:.2f})" for k in ("a", "j", "phi")))
    for k in ("a", "j", "phi"):
        assert fig[k] <= c[k], f"{what}: {k} of point {int(np.argmax(e[k]))} off by {fig[k]:.2f} x 2^-24, bound {c[k]:.2f}"
    return fig


# ---- inputs ------------------------------------------------------------------------------------------------------------------
SOFT = np.float32(0.01)


def system(n, seed=23):
    """n bodies in a unit cube, every one with (1 ... 2) x 1e10 kg and a velocity of order 1e-3 (potential_ref.dense)."""
    return PR.dense(n, seed)[0]


def body_points(s, bodies):
    """(points, velocities, skip) of murbfield_of(bodies): the bodies' own q and v, themselves skipped."""
    b = np.asarray(bodies, np.int64)
    return np.stack([s[k][b] for k in Q]), np.stack([s[k][b] for k in V]), b.astype(np.int32)


def midpoints(s, count, stride=7):
    """Midpoints of the body pairs (k, k + stride mod n) with the mean velocity, rounded to fp32; nobody skipped.  n = 1: the
    body's own place, whose own term then counts."""
    n = len(s["m"])
    k = np.arange(count) % n
    o = (k + stride) % n
    p = np.stack([(s[c][k].astype(np.float64) + s[c][o]) * 0.5 for c in Q]).astype(np.float32)
    v = np.stack([(s[c][k].astype(np.float64) + s[c][o]) * 0.5 for c in V]).astype(np.float32)
    return p, v, None


def far_points(count, seed=5):
    """Points at rest 1e3 box lengths away, in all directions: every term nearly parallel, the jerk sums cancel."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((3, count))
    return (0.5 + 1e3 * u / np.linalg.norm(u, axis=0)).astype(np.float32), None, None


def sparse_sources(n=PR.SPARSE_N, seed=11):
    """(state, soft, sources): potential_ref.sparse with velocities: mass at every tile's first and last slot alone."""
    return PR.sparse(n, seed, velocities=True)


def only_source(s, src):
    """The state with body `src` alone massive."""
    t = {k: v.copy() for k, v in s.items()}
    t["m"][:] = 0
    t["m"][src] = s["m"][src]
    return t


def displaced(s, body, soft, factor=10.0):
    """One point displaced from `body` by factor x soft along x, moving with it."""
    p = np.array([[s["qx"][body] + np.float32(factor) * np.float32(soft)], [s["qy"][body]], [s["qz"][body]]], np.float32)
    v = np.array([[s[k][body]] for k in V], np.float32)
    return p, v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in KEYS)

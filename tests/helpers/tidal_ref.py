"""Tidal tensor at arbitrary points (murbtidal_at / murbtidal_of), restated from include/murbtidal.h, for
tests/test_tidal_host.py (CPU) and tests/test_tidal_gpu.py (GPU).  numpy only; nothing here touches a device.  The inputs are
tests/helpers/field_ref.py's (system, midpoints, far_points, sparse_sources, only_source, body_points, displaced).

    d = q_j - p    r2 = |d|^2 + soft^2    inv = r2^(-1/2)    n = d inv    s = (G m_j inv) inv^2          over every real body j != skip_p:
    T_ab(p) = sum  s (3 n_a n_b - delta_ab)          the pair's term formed per pair: (3 s n_a) n_b - s delta_ab, then summed

The skipped body is left out by INDEX, nothing else: another body at the same place counts.

The bound (bound_of / check) is field_ref's in method.  A point's error is the Frobenius norm of got - fp64 over the symmetric
3 x 3 matrix (the off-diagonal components counted twice), scaled by the sum over the bodies of the Frobenius norm of each pair's
term, and bounded by C * 2^-24 with C = 4 x what a plain numpy float32 evaluation of the same formula (128 partial sums per
point, then added) attains against fp64 on the same inputs — the largest figure over the points of the case, computed on the CPU
and never from a device's output.  The factor 4 covers v_rsq_f32's 1 ulp against numpy's correctly rounded 1 / sqrt and a
different summation tree."""
import numpy as np

import field_ref as F
import hermite_ref as H

KEYS = ("txx", "tyy", "tzz", "txy", "txz", "tyz")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # (a, b) of KEYS
WEIGHT = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])             # the Frobenius norm counts an off-diagonal component twice
U24 = F.U24
Q = F.Q


def _eval(points, skip, q, gm, soft, dtype, nsplit, want_abs, block=256):
    points = np.asarray(points, dtype).reshape(3, -1)
    count = points.shape[1]
    skip = np.full(count, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    q, gm = np.asarray(q, dtype), np.asarray(gm, dtype)
    n = q.shape[1]
    soft2 = dtype(soft) * dtype(soft)
    t = np.zeros((6, count), dtype)
    ab, tr = np.zeros(count), np.zeros(count)
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

    for i0 in range(0, count, block):
        i1 = min(count, i0 + block)
        keep = cols[None, :] != skip[i0:i1, None]
        d = q[:, None, :] - points[:, i0:i1, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
            inv = dtype(1.0) / np.sqrt(r2)
            inv2 = inv * inv
            g = np.where(keep, gm[None, :] * inv, dtype(0.0))           # the skipped body: by index
            s = g * inv2
            s3 = dtype(3.0) * s
            nv = [d[k] * inv for k in range(3)]
            tv = [s3 * nv[k] for k in range(3)]
            terms = [np.where(keep, tv[a] * nv[b] - (s if a == b else dtype(0.0)), dtype(0.0)) for a, b in PAIRS]
        for k in range(6):
            t[k, i0:i1] = fold(terms[k])
        if want_abs:
            t64 = [np.asarray(x, np.float64) for x in terms]
            ab[i0:i1] = np.sqrt(sum(w * x * x for w, x in zip(WEIGHT, t64))).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                tr[i0:i1] = np.where(keep, -3.0 * np.float64(soft2) * np.asarray(s, np.float64) * np.asarray(inv2, np.float64), 0.0).sum(1)
    return t, ab, tr


def tidal_f64(points, skip, state, soft, want_abs=True, block=256):
    """fp64 (T (6, P) in KEYS' order, abs (P), trace (P)): the tidal tensor of `state`'s bodies at `points` (3, P), body skip[k]
    (or -1 / None: nobody) left out for point k.  abs: per point the sum over the bodies of the Frobenius norm of the pair's
    term; trace: -3 soft^2 sum G m inv^5, what txx + tyy + tzz is analytically (both with want_abs).  block: points evaluated at
    a time (memory alone; no value depends on it)."""
    return _eval(points, skip, H._stack(state, Q), H._gm(state), soft, np.float64, 1, want_abs, block)


def tidal_f32(points, skip, state, soft, nsplit=128, block=256):
    """The same formula in plain numpy float32, `nsplit` partial sums per point, then added (field_ref.field_f32's shape)."""
    return _eval(points, skip, H._stack(state, Q, np.float32), H._gm(state, np.float32), soft, np.float32, nsplit, False, block)[0]


def stack(got):
    """(6, P) of a result: the dict of Simulation.tidal_at, or an array."""
    return np.stack([np.asarray(got[k]) for k in KEYS]) if isinstance(got, dict) else np.asarray(got)


def scaled_errors(got, ref):
    """Per point: Frobenius norm of got - fp64 over the symmetric matrix / (the sum of the pair terms' Frobenius norms); ref:
    tidal_f64's result.  0 where a point has no terms and the value is exactly 0, inf where it is not."""
    t, ab = ref[0], ref[1]
    diff = np.sqrt((WEIGHT[:, None] * (stack(got).astype(np.float64) - t) ** 2).sum(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ab == 0.0, np.where(diff == 0.0, 0.0, np.inf), diff / ab)


def bound_of(points, skip, state, soft, ref=None, block=256):
    """(ref, C): tidal_f64's result and C of the bound in units of 2^-24 (the module's docstring)."""
    ref = tidal_f64(points, skip, state, soft, block=block) if ref is None else ref
    e = scaled_errors(tidal_f32(points, skip, state, soft, block=block), ref)
    return ref, 4.0 * float(np.max(e, initial=0.0)) / U24


def check(got, ref, c, what, rows=None):
    """Print the figure of `got` beside the bound and assert it; rows: the points of ref that got holds (all by default)."""
    if rows is not None:
        rows = np.asarray(rows)
        ref = (ref[0][:, rows], ref[1][rows], ref[2][rows])
    e = scaled_errors(got, ref)
    fig = float(np.max(e, initial=0.0)) / U24
    print(f"{what}: scaled error {fig:.2f} x 2^-24 (bound {c:.2f})")
    assert fig <= c, f"{what}: point {int(np.argmax(e))} off by {fig:.2f} x 2^-24, bound {c:.2f}"
    return fig


def trace_errors(got, ref):
    """Per point: |txx + tyy + tzz - (-3 soft^2 sum G m inv^5)| / (the scaling sum), the three components added in fp64."""
    g = stack(got).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(g[0] + g[1] + g[2] - ref[2]) / ref[1]


def matrix(t):
    """(P, 3, 3) symmetric matrices of a (6, P) array."""
    t = np.asarray(t)
    m = np.empty((t.shape[1], 3, 3), t.dtype)
    for k, (a, b) in enumerate(PAIRS):
        m[:, a, b] = m[:, b, a] = t[k]
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in KEYS)

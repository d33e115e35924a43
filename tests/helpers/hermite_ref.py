"""fp64 yardstick of the Hermite integrator (option "integrator" 2), numpy only, blocked over i so that N = 30 000 fits
in memory.  Written from the formulas, not from the device code:

    d = q_j - q_i    w = v_j - v_i    r2 = |d|^2 + soft^2
    a_i = sum_j G m_j d r2^(-3/2)          j_i = sum_j G m_j (w - 3 (d.w) d / r2) r2^(-3/2)

    predict   qp = q + v dt + a0 dt^2/2 + j0 dt^3/6          vp = v + a0 dt + j0 dt^2/2
    evaluate  (a1, j1) at (qp, vp)
    correct   v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12
              q1 = q + (v + v1) dt/2  + (a0 - a1) dt^2/12     (a0, j0) <- (a1, j1)

The sums of predict / correct are taken left to right as written, in fp64, with the coefficients formed in fp64 from the
fp32 dt (dt*0.5, dt*dt*0.5, dt*dt*dt/6, dt*dt/12) — include/murbhip.h's definition of the update, which the device
rounds to fp32 once per stored value.  state32=True rounds q, v, a, j to fp32 at exactly those stores (and uses the
rounded v1 in q1), so that only the force sweep's own fp32 arithmetic separates the device from this restatement."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

G = np.float32(6.67384e-11)   # reference SimulationNBodyInterface.hpp:18
_Q, _V = ("qx", "qy", "qz"), ("vx", "vy", "vz")


def _stack(s, keys, dtype=np.float64):
    return np.stack([np.asarray(s[k], dtype) for k in keys])


def _evaluate(q, v, gm, soft, dtype=np.float64, block=128, want_abs=False, nsplit=1):
    """(a, j, abs_j): accelerations (3, n), jerks (3, n; None without v) and, with want_abs, the per-body sum of the
    magnitudes of its jerk terms.  All arithmetic in `dtype`.  nsplit > 1: every body's sums are taken as `nsplit`
    partial sums over contiguous ranges of j, added afterwards in index order (the shape of a GPU sweep)."""
    q = np.asarray(q, dtype)
    gm = np.asarray(gm, dtype)
    n = q.shape[1]
    soft2 = dtype(soft) * dtype(soft)
    a = np.zeros((3, n), dtype)
    j = np.zeros((3, n), dtype) if v is not None else None
    abs_j = np.zeros(n, np.float64) if want_abs else None
    if v is not None:
        v = np.asarray(v, dtype)
    bounds = [(n * k) // nsplit for k in range(nsplit + 1)]

    def fold(terms):   # (b, n) -> (b,): partial sums over the j ranges, then added in order
        if nsplit == 1:
            return terms.sum(1, dtype=dtype)
        out = np.zeros(terms.shape[0], dtype)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if hi > lo:
                out = out + terms[:, lo:hi].sum(1, dtype=dtype)
        return out

    def one_block(i0):
        i1 = min(n, i0 + block)
        d = q[:, None, :] - q[:, i0:i1, None]                 # (3, b, n)
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
        inv = dtype(1.0) / np.sqrt(r2)
        inv2 = inv * inv
        s = (gm[None, :] * inv) * inv2
        for k in range(3):
            a[k, i0:i1] = fold(s * d[k])
        if v is None:
            return
        w = v[:, None, :] - v[:, i0:i1, None]
        c = dtype(-3.0) * ((d[0] * w[0] + d[1] * w[1] + d[2] * w[2]) * inv2)
        t = [s * (w[k] + c * d[k]) for k in range(3)]
        for k in range(3):
            j[k, i0:i1] = fold(t[k])
        if want_abs:
            t64 = [np.asarray(x, np.float64) for x in t]
            abs_j[i0:i1] = np.sqrt(t64[0] ** 2 + t64[1] ** 2 + t64[2] ** 2).sum(1)

    starts = range(0, n, block)
    if n * n < (1 << 24):
        for i0 in starts:
            one_block(i0)
    else:   # the blocks write disjoint columns and numpy releases the interpreter lock inside its loops
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(one_block, starts))
    return a, j, abs_j


def _gm(s, dtype=np.float64):
    return dtype(G) * np.asarray(s["m"], dtype)


def acc_f64(s, soft):
    """fp64 accelerations (3, n) of the state dict s."""
    return _evaluate(_stack(s, _Q), None, _gm(s), soft)[0]


def acc_jerk_f64(s, soft, want_abs=False):
    """fp64 (a, j) of the state dict s, each (3, n); with want_abs also the per-body sum of |jerk terms|."""
    a, j, ab = _evaluate(_stack(s, _Q), _stack(s, _V), _gm(s), soft, want_abs=want_abs)
    return (a, j, ab) if want_abs else (a, j)


def acc_jerk_f32(s, soft, nsplit=128):
    """The same formulas in plain numpy float32: `nsplit` partial sums per body, then added.  What fp32 arithmetic
    attains on these inputs without any device: the yardstick the jerk bound of the GPU tests is derived from."""
    a, j, _ = _evaluate(_stack(s, _Q, np.float32), _stack(s, _V, np.float32), _gm(s, np.float32), soft, dtype=np.float32,
                        nsplit=nsplit)
    return a, j


def acc_jerk_sources(s, src, soft, dtype=np.float64, block=1024):
    """(a, j, abs_a, abs_j, min_j) of every body due to the bodies `src` alone (a sparse-mass probe, oracle.probe_state:
    every other mass is 0): a, j (3, n) in `dtype`, every operation of the header's formulas in `dtype`; abs_a, abs_j the
    per-body sums of the magnitudes of the terms and min_j the smallest jerk term over the sources other than the body
    itself (+inf without one), those three in fp64 from the terms as computed.  O(n K), blocked over i."""
    src = np.asarray(src, np.int64)
    q, v = _stack(s, _Q, dtype), _stack(s, _V, dtype)
    n = q.shape[1]
    gm = _gm(s, dtype)[src]
    qs, vs = q[:, src], v[:, src]
    soft2 = dtype(soft) * dtype(soft)
    a, j = np.zeros((3, n), dtype), np.zeros((3, n), dtype)
    abs_a, abs_j, min_j = np.zeros(n), np.zeros(n), np.full(n, np.inf)
    if len(src) == 0:
        return a, j, abs_a, abs_j, min_j

    def norm64(t):
        t = [np.asarray(x, np.float64) for x in t]
        return np.sqrt(t[0] ** 2 + t[1] ** 2 + t[2] ** 2)

    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        d = qs[:, None, :] - q[:, i0:i1, None]                 # (3, b, K)
        w = vs[:, None, :] - v[:, i0:i1, None]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
        inv = dtype(1.0) / np.sqrt(r2)
        inv2 = inv * inv
        sc = (gm[None, :] * inv) * inv2
        c = dtype(-3.0) * ((d[0] * w[0] + d[1] * w[1] + d[2] * w[2]) * inv2)
        ta = [sc * d[k] for k in range(3)]
        tj = [sc * (w[k] + c * d[k]) for k in range(3)]
        for k in range(3):
            a[k, i0:i1] = ta[k].sum(1, dtype=dtype)
            j[k, i0:i1] = tj[k].sum(1, dtype=dtype)
        na, nj = norm64(ta), norm64(tj)
        abs_a[i0:i1], abs_j[i0:i1] = na.sum(1), nj.sum(1)
        other = src[None, :] != np.arange(i0, i1)[:, None]
        min_j[i0:i1] = np.where(other, nj, np.inf).min(1)
    return a, j, abs_a, abs_j, min_j


def scaled_err(test, truth, abs_sum):
    """Per body |test - truth| / (sum of the magnitudes of the body's terms): oracle.probe_err's convention."""
    t = np.stack([np.asarray(c, np.float64) for c in test])
    r = np.stack([np.asarray(c, np.float64) for c in truth])
    return np.sqrt(((t - r) ** 2).sum(0)) / np.maximum(abs_sum, np.finfo(np.float64).tiny)


def _r32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def predict(q, v, a0, j0, dt):
    """fp64 (qp, vp), unrounded; dt is taken as the fp32 value the device gets."""
    dt = float(np.float32(dt))
    c2, c3 = dt * dt * 0.5, dt * dt * dt / 6.0
    q, v, a0, j0 = (np.asarray(x, np.float64) for x in (q, v, a0, j0))
    return ((q + v * dt) + a0 * c2) + j0 * c3, (v + a0 * dt) + j0 * c2


def correct(q, v, a0, j0, a1, j1, dt, state32=True):
    """(q1, v1) of the corrector, fp64 intermediates; state32: v1 is rounded to fp32 before q1 uses it, q1 once."""
    dt = float(np.float32(dt))
    h, c12 = dt * 0.5, dt * dt / 12.0
    q, v, a0, j0, a1, j1 = (np.asarray(x, np.float64) for x in (q, v, a0, j0, a1, j1))
    v1 = (v + (a0 + a1) * h) + (j0 - j1) * c12
    if state32:
        v1 = _r32(v1)
    q1 = (q + (v + v1) * h) + (a0 - a1) * c12
    if state32:
        q1 = _r32(q1)
    return q1, v1


def hermite_f64(s, steps, soft, dt, state32=False, gm=None):
    """`steps` Hermite steps from the state dict s (not modified).  Returns a state dict (fp32 arrays with state32,
    fp64 otherwise) with the masses of s.  gm: the bodies' G m in another unit system (default: G of the reference times
    the masses of s)."""
    q, v, gm = _stack(s, _Q), _stack(s, _V), _gm(s) if gm is None else np.asarray(gm, np.float64)
    rnd = _r32 if state32 else (lambda x: x)
    a0, j0, _ = _evaluate(q, v, gm, soft)
    a0, j0 = rnd(a0), rnd(j0)
    for _ in range(steps):
        qp, vp = predict(q, v, a0, j0, dt)
        a1, j1, _ = _evaluate(rnd(qp), rnd(vp), gm, soft)
        a1, j1 = rnd(a1), rnd(j1)
        q, v = correct(q, v, a0, j0, a1, j1, dt, state32)
        a0, j0 = a1, j1
    out = {k: np.array(x, np.float32 if state32 else np.float64) for k, x in zip(_Q + _V, list(q) + list(v))}
    out["m"] = np.array(s["m"])
    if "r" in s:
        out["r"] = np.array(s["r"])
    return out

"""Massless tracers (include/murbtracer.h) restated in fp64, and the inputs tests/test_tracer_host.py (CPU) and
tests/test_tracer_gpu.py (GPU) share.  numpy only; nothing here touches a device.

A tracer feels the bodies and nothing feels a tracer: its (a, j) are the field's direct sum at its place and velocity with no
body skipped (field_ref.field_f64), and predictor and corrector are the bodies' (hermite_ref.predict / correct, fp64
intermediates, the stored values rounded once to fp32 with state32).  One step of a set of tracers beside the bodies:

    bodies:   (qp, vp) = predict(q, v, a0, j0)        tracers:  (tp, tw) = predict(tq, tv, ta0, tj0)
              (a1, j1) at (qp, vp)                              (ta1, tj1) = field of the bodies AT (qp, vp), at (tp, tw)
              correct                                           correct

Everything is taken from hermite_ref.py and field_ref.py by import."""
import numpy as np

import field_ref as F
import hermite_adaptive_ref as HA
import hermite_ref as H

Q, V = F.Q, F.V
r32 = H._r32


def stack(d, keys):
    return np.stack([np.asarray(d[k]) for k in keys])


def acc_jerk(points, pvel, state, soft):
    """fp64 (a, j), each (3, P): the direct sum over the bodies of `state` at `points` moving with `pvel` (None: at rest)."""
    a, j, _, _ = F.field_f64(points, pvel, None, state, soft, want_abs=False)
    return a, j


def predicted_state(state, a0, j0, dt, state32=True):
    """The bodies' predicted state as a state dict (fp32 arrays with state32: the records the device's sweeps read)."""
    qp, vp = H.predict(stack(state, Q), stack(state, V), a0, j0, dt)
    dtype = np.float32 if state32 else np.float64
    out = {k: np.array(x, dtype) for k, x in zip(Q + V, list(qp) + list(vp))}
    out["m"] = np.array(state["m"])
    return out


def run(state, tq, tv, steps, soft, dt, state32=False):
    """`steps` Hermite steps of the bodies of `state` with the tracers (tq, tv), each (3, M), beside them; fp64 sums, the stored
    values rounded to fp32 with state32.  Returns (state dict of the bodies, tq, tv)."""
    rnd = r32 if state32 else (lambda x: np.asarray(x, np.float64))
    q, v, gm = H._stack(state, Q), H._stack(state, V), H._gm(state)
    tq, tv = np.asarray(tq, np.float64), np.asarray(tv, np.float64)

    def bodies_of(q, v):
        s = {k: x for k, x in zip(Q + V, list(q) + list(v))}
        s["m"] = state["m"]
        return s

    a0, j0, _ = H._evaluate(q, v, gm, soft)
    a0, j0 = rnd(a0), rnd(j0)
    ta0, tj0 = (rnd(x) for x in acc_jerk(tq, tv, bodies_of(q, v), soft))
    for _ in range(steps):
        qp, vp = (rnd(x) for x in H.predict(q, v, a0, j0, dt))
        tp, tw = (rnd(x) for x in H.predict(tq, tv, ta0, tj0, dt))
        a1, j1, _ = H._evaluate(qp, vp, gm, soft)
        a1, j1 = rnd(a1), rnd(j1)
        ta1, tj1 = (rnd(x) for x in acc_jerk(tp, tw, bodies_of(qp, vp), soft))
        q, v = H.correct(q, v, a0, j0, a1, j1, dt, state32)
        tq, tv = H.correct(tq, tv, ta0, tj0, ta1, tj1, dt, state32)
        a0, j0, ta0, tj0 = a1, j1, ta1, tj1
    return bodies_of(q, v), tq, tv


# The bodies' step criterion on a tracer's own evaluations ("tracer_dt" 1): hermite_adaptive_ref's, by name.
aarseth_step = HA.body_steps            # (a0, j0, a1, j1, dt, eta) -> fp64 (M,), +inf where not a finite positive number
first_step = HA.first_body_steps        # (a0, j0, eta_start): eta_start |a0| / |j0|


# ---- inputs ------------------------------------------------------------------------------------------------------------------
SOFT = F.SOFT
DT = np.float32(1e-3)     # F.system(n): G m about 0.7 per body in a unit cube, so a crossing takes about 0.05 at n = 513


def tracers(state, count, seed=41):
    """(tq, tv), each (3, count) float32: points in the bodies' cube and a little outside, velocities of the bodies' order."""
    rng = np.random.default_rng(seed)
    tq = rng.uniform(-0.25, 1.25, (3, count)).astype(np.float32)
    tv = (1e-3 * rng.standard_normal((3, count))).astype(np.float32)
    return tq, tv


def kepler(gm=1.0, r=1.0):
    """(state dict of ONE body of G m = gm at rest at the origin, tq, tv of one tracer on the circular orbit of radius r, period)."""
    state = {k: np.zeros(1) for k in Q + V}
    state["m"] = np.array([gm / float(H.G)])
    vc = np.sqrt(gm / r)
    return state, np.array([[r], [0.0], [0.0]]), np.array([[0.0], [vc], [0.0]]), 2.0 * np.pi * r / vc


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(x, y):
    """Two dicts of arrays, or two arrays: equal in every bit."""
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == "f":
        return x.shape == y.shape and np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64),
                                                     y.view(np.uint32 if y.dtype == np.float32 else np.uint64))
    return np.array_equal(x, y)

"""numpy restatement of the shared adaptive time step of the Hermite integrator (murbhip_evolve), written from the
formulas of include/murbhip.h, not from the device code.  With |x| the Euclidean norm, for every real body

    a2 = (-6 (a0 - a1) - dt (4 j0 + 2 j1)) / dt^2     a3 = (12 (a0 - a1) + 6 dt (j0 + j1)) / dt^3     a2 += dt a3
    dt_i = sqrt( eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2) )

the candidate is min_i dt_i (a dt_i that is not a finite positive number counts as +inf), rounded once to fp32 and clamped
to [dt_min, dt_max]; a call that finds no proposal starts from eta_start * min_i |a0| / |j0|; a candidate >= duration - t
is replaced by (float)(duration - t), and that step is the last.  All of it in fp64, in the order written below (sums of
squares left to right, |x|^2 taken as the sum of squares itself, products left to right)."""
import numpy as np

import hermite_ref as H

_INF32 = np.float32(np.inf)


def _f64(*xs):
    return [np.asarray(x, np.float64) for x in xs]


def _sumsq(x):
    return (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]


def _positive(d):
    return np.where(np.isfinite(d) & (d > 0.0), d, np.inf)


def body_steps(a0, j0, a1, j1, dt, eta):
    """dt_i of every body, fp64 (n,), +inf where the expression is not a finite positive number.  a0 ... j1 are (3, n)."""
    a0, j0, a1, j1 = _f64(a0, j0, a1, j1)
    dt, eta = float(np.float32(dt)), float(eta)
    with np.errstate(all="ignore"):
        dt2 = dt * dt
        dt3 = dt2 * dt
        d = a0 - a1
        a2 = ((-6.0 * d) - dt * ((4.0 * j0) + (2.0 * j1))) / dt2
        a3 = ((12.0 * d) + (6.0 * dt) * (j0 + j1)) / dt3
        a2 = a2 + dt * a3
        s_a1, s_j1, s_a2, s_a3 = _sumsq(a1), _sumsq(j1), _sumsq(a2), _sumsq(a3)
        num = eta * (np.sqrt(s_a1) * np.sqrt(s_a2) + s_j1)
        den = np.sqrt(s_j1) * np.sqrt(s_a3) + s_a2
        return _positive(np.sqrt(num / den))


def first_body_steps(a0, j0, eta_start):
    """eta_start |a0| / |j0| of every body, fp64, +inf where that is not a finite positive number."""
    a0, j0 = _f64(a0, j0)
    with np.errstate(all="ignore"):
        return _positive(float(eta_start) * (np.sqrt(_sumsq(a0)) / np.sqrt(_sumsq(j0))))


def candidate(a0, j0, a1, j1, dt, eta):
    """The unclamped proposal for the next step: fp32 (+inf when no body yields one)."""
    with np.errstate(over="ignore"):
        return np.float32(body_steps(a0, j0, a1, j1, dt, eta).min(initial=np.inf))


def first_candidate(a0, j0, eta_start):
    with np.errstate(over="ignore"):
        return np.float32(first_body_steps(a0, j0, eta_start).min(initial=np.inf))


def clamp(c, dt_min, dt_max):
    return np.float32(max(np.float32(dt_min), min(np.float32(c), np.float32(dt_max))))


def choose(cand, t, duration, dt_min, dt_max):
    """(dt, last): the fp32 step taken from the unclamped candidate at clock t."""
    dt = clamp(cand, dt_min, dt_max)
    if float(dt) >= float(duration) - float(t):
        return np.float32(float(duration) - float(t)), True
    return dt, False


def evolve(s, duration, soft, eta=0.02, eta_start=0.01, dt_min=0.0, dt_max=None, max_steps=1_000_000, fixed_dt=None):
    """Hermite steps over `duration` seconds from the state dict s (not modified), fp64 sweeps, state, a and j rounded to
    fp32 at every store (hermite_ref.hermite_f64 with state32).  fixed_dt: that step every time instead of the rule.
    Returns (state dict, list of the fp32 steps taken, clock reached, unclamped proposal for the next step)."""
    q, v, gm = H._stack(s, H._Q), H._stack(s, H._V), H._gm(s)
    dt_max = duration if dt_max is None else dt_max
    a0, j0, _ = H._evaluate(q, v, gm, soft)
    a0, j0 = H._r32(a0), H._r32(j0)
    cand = first_candidate(a0, j0, eta_start)
    t, dts, last = 0.0, [], False
    while not last and len(dts) < max_steps:
        if fixed_dt is None:
            dt, last = choose(cand, t, duration, dt_min, dt_max)
        else:
            dt, last = choose(np.float32(fixed_dt), t, duration, 0.0, np.inf)
        qp, vp = H.predict(q, v, a0, j0, dt)
        a1, j1, _ = H._evaluate(H._r32(qp), H._r32(vp), gm, soft)
        a1, j1 = H._r32(a1), H._r32(j1)
        q, v = H.correct(q, v, a0, j0, a1, j1, dt, True)
        cand = candidate(a0, j0, a1, j1, dt, eta)
        a0, j0 = a1, j1
        t = float(duration) if last else t + float(dt)
        dts.append(dt)
    out = {k: np.array(x, np.float32) for k, x in zip(H._Q + H._V, list(q) + list(v))}
    out["m"] = np.array(s["m"])
    return out, dts, t, cand


# ---- the equal-mass binary of the tests ------------------------------------------------------------------------------
def binary(e, m=1e30, a=1e11):
    """(state dict, period): two bodies of mass m on an orbit of semi-major axis a and eccentricity e, at pericentre (where
    the starting rule eta_start |a0| / |j0| is at its smallest), centre of mass at rest at the origin, orbit in the x-y
    plane."""
    mu = float(H.G) * 2.0 * m
    r = a * (1.0 - e)
    vrel = np.sqrt(mu * (1.0 + e) / r)
    z = np.zeros(2, np.float32)
    s = {"qx": np.array([-r / 2, r / 2], np.float32), "qy": z.copy(), "qz": z.copy(),
         "vx": z.copy(), "vy": np.array([-vrel / 2, vrel / 2], np.float32), "vz": z.copy(),
         "m": np.array([m, m], np.float32)}
    return s, 2.0 * np.pi * np.sqrt(a * a * a / mu)


def energy(s, soft):
    """Kinetic + softened pair potential of a state dict, fp64 (any constant convention cancels in a relative error)."""
    q, v, m = H._stack(s, H._Q), H._stack(s, H._V), np.asarray(s["m"], np.float64)
    ke = 0.5 * (m * (v * v).sum(0)).sum()
    d = q[:, :, None] - q[:, None, :]
    r = np.sqrt((d * d).sum(0) + float(soft) ** 2)
    iu = np.triu_indices(len(m), 1)
    return ke - float(H.G) * (np.outer(m, m)[iu] / r[iu]).sum()

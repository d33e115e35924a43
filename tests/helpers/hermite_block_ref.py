"""numpy restatement of the individual block time steps of the Hermite integrator (murbhip_evolve_block), written from the
text of include/murbhip.h, not from the device code.

A block of dt_max seconds is T = 2^kmax ticks.  Body i holds a level k_i in [0, kmax] (its step is dt_max 2^-k_i seconds,
T >> k_i ticks) and its own time t_i in ticks, in [0, T).  Time is integer throughout; seconds are only ever
ticks * (dt_max * 2^-kmax), an exact product in fp64.  One block step: t_next = min_i (t_i + (T >> k_i)); every body is predicted
to t_next with its own dt; (a1, j1) of the active bodies (those that attain the minimum) at the predicted state of all; each active
body is corrected from its own (q, v, a0, j0) with its own dt_i; its new level follows from the step criterion of the shared
scheme (hermite_adaptive_ref.body_steps) rounded to fp32.  Sweeps are fp64 here, every stored value is rounded to fp32
(hermite_ref's state32 convention), so that only the device's fp32 sweep separates the two."""
import numpy as np

import hermite_adaptive_ref as A
import hermite_ref as H


def level_dt(dt_max, k):
    """dt_max 2^-k as the fp32 value (exact while it is a normal number)."""
    return np.float32(np.ldexp(np.float32(dt_max), -int(k)))


def tick_seconds(dt_max, kmax):
    return float(np.float32(dt_max)) * 2.0 ** -int(kmax)


def k_req(req, dt_max, kmax):
    """(level, clamped): the smallest k in [0, kmax] with dt_max 2^-k <= req; +inf gives 0; none: kmax, clamped."""
    req = np.float32(req)
    for k in range(int(kmax) + 1):
        if level_dt(dt_max, k) <= req:
            return k, False
    return int(kmax), True


def new_level(k, kreq, t_next, kmax):
    """Any number of halvings at once; one doubling, and only where the coarser grid has a point; else unchanged."""
    T = 1 << int(kmax)
    if kreq > k:
        return kreq
    if kreq < k and t_next % (2 * (T >> k)) == 0:
        return k - 1
    return k


def to_f32_or_inf(x):
    """The criterion's fp64 values (already +inf where not finite and positive) rounded to fp32."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def start_levels(a0, j0, eta_start, dt_max, kmax):
    req = to_f32_or_inf(A.first_body_steps(a0, j0, eta_start))
    return np.array([k_req(r, dt_max, kmax)[0] for r in req], np.int32)


def next_time(ticks, levels, kmax):
    """(t_next, mask of the active bodies)."""
    T = 1 << int(kmax)
    nxt = ticks.astype(np.int64) + (T >> levels.astype(np.int64))
    t_next = int(nxt.min())
    return t_next, nxt == t_next


def predict_all(q, v, a0, j0, ticks, t_next, dt_max, kmax):
    """fp64 (qp, vp) of every body at t_next, each with its own dt, unrounded: hermite_ref.predict's sums with a per-body dt."""
    dt = (t_next - ticks.astype(np.int64)).astype(np.float64) * tick_seconds(dt_max, kmax)
    c2, c3 = dt * dt * 0.5, dt * dt * dt / 6.0
    q, v, a0, j0 = (np.asarray(x, np.float64) for x in (q, v, a0, j0))
    return ((q + v * dt) + a0 * c2) + j0 * c3, (v + a0 * dt) + j0 * c2


def levels_after(a0, j0, a1, j1, levels, active, t_next, eta, dt_max, kmax):
    """(new levels, number of clamped steps) from both evaluations of the active bodies; a0 ... j1 are (3, n), only the active
    columns are read.  Bodies of one level share dt_i, so the criterion is evaluated level by level."""
    out, clamped = levels.copy(), 0
    for k in np.unique(levels[active]):
        sel = np.flatnonzero(active & (levels == k))
        req = to_f32_or_inf(A.body_steps(a0[:, sel], j0[:, sel], a1[:, sel], j1[:, sel], level_dt(dt_max, k), eta))
        for i, r in zip(sel, req):
            kr, cl = k_req(r, dt_max, kmax)
            clamped += int(cl)
            out[i] = new_level(int(k), kr, t_next, kmax)
    return out, clamped


def evaluate_rows(q, v, gm, idx, soft, dtype=np.float64):
    """(a, j, abs_j) of the bodies `idx` alone against all n bodies, hermite_ref._evaluate's formulas in `dtype`: a, j (3, m),
    abs_j (m) the fp64 sum of the magnitudes of each body's jerk terms.  Blocked over i: (3, 256, n) temporaries."""
    q, v, gm = np.asarray(q, dtype), np.asarray(v, dtype), np.asarray(gm, dtype)
    idx = np.asarray(idx, np.int64)
    a, j, abs_j = np.zeros((3, len(idx)), dtype), np.zeros((3, len(idx)), dtype), np.zeros(len(idx))
    soft2 = dtype(soft) * dtype(soft)
    for lo in range(0, len(idx), 256):
        rows = idx[lo:lo + 256]
        d = q[:, None, :] - q[:, rows, None]
        w = v[:, None, :] - v[:, rows, None]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
        inv = dtype(1.0) / np.sqrt(r2)
        inv2 = inv * inv
        sc = (gm[None, :] * inv) * inv2
        c = dtype(-3.0) * ((d[0] * w[0] + d[1] * w[1] + d[2] * w[2]) * inv2)
        tj = [sc * (w[k] + c * d[k]) for k in range(3)]
        for k in range(3):
            a[k, lo:lo + 256] = (sc * d[k]).sum(1, dtype=dtype)
            j[k, lo:lo + 256] = tj[k].sum(1, dtype=dtype)
        t64 = [np.asarray(x, np.float64) for x in tj]
        abs_j[lo:lo + 256] = np.sqrt(t64[0] ** 2 + t64[1] ** 2 + t64[2] ** 2).sum(1)
    return a, j, abs_j


class Run:
    """State of a run: q, v, a0, j0 (3, n) fp32 values held as fp64, ticks, levels; counters like out8."""

    def __init__(self, s, soft, dt_max, kmax=12, eta=0.02, eta_start=0.01, levels=None):
        self.soft, self.dt_max, self.kmax, self.eta = soft, np.float32(dt_max), int(kmax), eta
        self.T = 1 << self.kmax
        self.m = np.array(s["m"])
        self.gm = H._gm(s)
        self.q, self.v = H._stack(s, H._Q), H._stack(s, H._V)
        a0, j0, _ = H._evaluate(self.q, self.v, self.gm, soft)
        self.a0, self.j0 = H._r32(a0), H._r32(j0)
        n = self.q.shape[1]
        self.ticks = np.zeros(n, np.int64)
        self.levels = (start_levels(self.a0, self.j0, eta_start, self.dt_max, self.kmax) if levels is None
                       else np.array(levels, np.int32))
        self.steps = self.body_steps = self.clamped = self.max_active = self.ticks_done = 0
        self.k_lo, self.k_hi = self.kmax, 0
        self.clock = 0

    def step(self):
        """One block step; returns the mask of the bodies it advanced."""
        t_next, act = next_time(self.ticks, self.levels, self.kmax)
        qp, vp = predict_all(self.q, self.v, self.a0, self.j0, self.ticks, t_next, self.dt_max, self.kmax)
        a1, j1 = self.evaluate_active(H._r32(qp), H._r32(vp), act)
        for k in np.unique(self.levels[act]):      # bodies of one level share dt_i: hermite_ref.correct per level
            sel = act & (self.levels == k)
            q1, v1 = H.correct(self.q[:, sel], self.v[:, sel], self.a0[:, sel], self.j0[:, sel], a1[:, sel], j1[:, sel],
                               level_dt(self.dt_max, k), True)
            self.q[:, sel], self.v[:, sel] = q1, v1
        new, cl = levels_after(self.a0, self.j0, a1, j1, self.levels, act, t_next, self.eta, self.dt_max, self.kmax)
        self.k_lo, self.k_hi = min(self.k_lo, int(self.levels[act].min())), max(self.k_hi, int(self.levels[act].max()))
        self.a0[:, act], self.j0[:, act] = a1[:, act], j1[:, act]
        self.levels = new
        self.ticks[act] = 0 if t_next == self.T else t_next
        self.ticks_done += t_next - self.clock
        self.clock = 0 if t_next == self.T else t_next
        self.steps += 1
        self.body_steps += int(act.sum())
        self.clamped += cl
        self.max_active = max(self.max_active, int(act.sum()))
        return act

    def evaluate_active(self, qp, vp, act):
        """fp64 (a1, j1) of the active bodies at the predicted state of all, rounded to fp32; (3, n) with the other columns 0."""
        a1, j1 = np.zeros_like(self.q), np.zeros_like(self.q)
        idx = np.flatnonzero(act)
        a1[:, idx], j1[:, idx], _ = evaluate_rows(qp, vp, self.gm, idx, self.soft)
        return H._r32(a1), H._r32(j1)

    def run(self, blocks=1, max_steps=None, check=None):
        """Block steps until `blocks` block boundaries are reached (or max_steps taken); check(self, active) after each."""
        left = blocks
        while left > 0 and (max_steps is None or self.steps < max_steps):
            act = self.step()
            if check is not None:
                check(self, act)
            if self.clock == 0:
                left -= 1
        return self

    def time(self):
        return self.ticks_done * tick_seconds(self.dt_max, self.kmax)

    def state(self):
        out = {k: np.array(x, np.float32) for k, x in zip(H._Q + H._V, list(self.q) + list(self.v))}
        out["m"] = np.array(self.m)
        return out


# ---- the system the feature was specified with ----------------------------------------------------------------------------
SOFT = 1e6
FIELD_MASS, FIELD_R0, FIELD_R1 = 1e26, 2e12, 8e12


def cluster(n):
    """(state, binary period): hermite_adaptive_ref.binary(0.9) plus n - 2 light field bodies of 1e26 kg on circular orbits in
    the x-y plane at radii 2e12 ... 8e12 m (evenly spaced in radius, and in phase once round), around the binary's 2e30 kg."""
    s, period = A.binary(0.9)
    nf = n - 2
    r = np.linspace(FIELD_R0, FIELD_R1, nf)
    ph = 2.0 * np.pi * np.arange(nf) / nf
    vc = np.sqrt(float(H.G) * 2e30 / r)
    add = {"qx": r * np.cos(ph), "qy": r * np.sin(ph), "qz": np.zeros(nf),
           "vx": -vc * np.sin(ph), "vy": vc * np.cos(ph), "vz": np.zeros(nf), "m": np.full(nf, FIELD_MASS)}
    return {k: np.concatenate([s[k], add[k].astype(np.float32)]) for k in s}, period

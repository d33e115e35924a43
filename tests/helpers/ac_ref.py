"""The Ahmad-Cohen neighbour scheme (murbac_begin / murbac_steps), restated from include/murbac.h, and the inputs that
tests/test_ac_host.py (CPU) and tests/test_ac_gpu.py (GPU) share.  numpy only; nothing here touches a device.

    begin      L = the neighbours within h; (aI, jI) the list field over L; (a0, j0) the full sweep; aR = a0 - aI, jR = j0 - jI (fp32);
               a2R = a3R = 0; m = 0
    irregular  predict; (aI1, jI1) over L at the predicted state; tau = (m + 1) dt;
               a1 = aI1 + (float)(((aR + jR tau) + a2R (tau tau 0.5)) + a3R (tau tau tau / 6)),
               j1 = jI1 + (float)((jR + a2R tau) + a3R (tau tau 0.5)); correct; m += 1
    regular    predict; (a1, j1) the full sweep; (aIo, jIo) over the OLD L; A1 = a1 - aIo, J1 = j1 - jIo; T = n_irr dt;
               x2 = (-6 (aR - A1) - T (4 jR + 2 J1)) / T^2, x3 = (12 (aR - A1) + 6 T (jR + J1)) / T^3, a2R = x2 + T x3, a3R = x3;
               new L', (aIn, jIn) over it; aR = a1 - aIn, jR = j1 - jIn; correct with the total; m = 0

The forces come from hermite_ref (full sweep) and list_ref (list field): in fp64 (sums="f64"), or in plain float32 with a list's terms
added in list order (sums="f32").  The state and every stored force are rounded to fp32 at the stores (state32), as on the device;
the polynomial, the derivative update and the corrector are evaluated in fp64 exactly as the header states them.  The lists are
list_ref.neighbours_f32's (the predicate in fma-free float32: a pair within an ulp of the sphere may differ from the device's).

WRONG names deliberately wrong readings of the definition, for the test that shows the inputs tell them apart."""
import numpy as np

import hermite_ref as H
import list_ref as R

Q, V = R.Q, R.V
SOFT = R.SOFT
WRONG = ("the new list used for A1", "a2R left at the step's start value x2", "tau counted from the last step")
NAMES = ("aI", "jI", "aR", "jR", "a2R", "a3R")


def f32(x):
    return np.asarray(x, np.float32)


def poly(aR, jR, a2R, a3R, tau):
    """(aR(tau), jR(tau)) in fp32: fp64 intermediates, left to right, one rounding."""
    aR, jR, a2R, a3R = (np.asarray(x, np.float64) for x in (aR, jR, a2R, a3R))
    tau = float(tau)
    a = ((aR + jR * tau) + a2R * (tau * tau * 0.5)) + a3R * (tau * tau * tau / 6.0)
    j = (jR + a2R * tau) + a3R * (tau * tau * 0.5)
    return f32(a), f32(j)


def derivatives(A0, J0, A1, J1, T, keep_x2=False, exact=False):
    """(a2R, a3R) at the END of an interval T from the force and jerk at both ends; exact: unrounded fp64."""
    A0, J0, A1, J1 = (np.asarray(x, np.float64) for x in (A0, J0, A1, J1))
    T = float(T)
    d = A0 - A1
    x2 = (-6.0 * d - T * (4.0 * J0 + 2.0 * J1)) / (T * T)
    x3 = (12.0 * d + 6.0 * T * (J0 + J1)) / (T * T * T)
    a2 = x2 if keep_x2 else x2 + T * x3
    return (a2, x3) if exact else (f32(a2), f32(x3))


def elapsed(steps, dt):
    return float(steps) * float(np.float32(dt))


def _state(q, v, s):
    out = {k: np.array(x, np.float32) for k, x in zip(Q + V, list(q) + list(v))}
    out["m"] = np.array(s["m"])
    return out


class Scheme:
    """The scheme on the state dict s (not modified).  h: a scalar or one radius per body."""

    def __init__(self, s, h, n_irr, soft, sums="f64", wrong=None):
        assert sums in ("f64", "f32") and (wrong is None or wrong in WRONG)
        self.s, self.soft, self.n_irr, self.sums, self.wrong = s, soft, int(n_irr), sums, wrong
        self.n = len(s["m"])
        self.h = np.broadcast_to(np.asarray(h, np.float32), (self.n,))
        self.q = H._stack(s, Q, np.float32).astype(np.float64)
        self.v = H._stack(s, V, np.float32).astype(np.float64)
        self.m, self.steps, self.regular, self.time = 0, 0, 0, 0.0
        self.lists = self._neighbours(self.q)
        self.a0, self.j0 = self._full(self.q, self.v)
        self.aI, self.jI = self._listed(self.q, self.v, self.lists)
        self.aR, self.jR = self.a0 - self.aI, self.j0 - self.jI   # fp32
        self.a2R, self.a3R = np.zeros((3, self.n), np.float32), np.zeros((3, self.n), np.float32)

    # -- forces of a state (fp32 values), rounded to fp32
    def _neighbours(self, q):
        return R.neighbours_f32(_state(q, self.v, self.s), self.h, self.soft)

    def _full(self, q, v):
        if self.sums == "f64":
            a, j, _ = H._evaluate(q, v, H._gm(self.s), self.soft)
        else:
            a, j, _ = H._evaluate(f32(q), f32(v), H._gm(self.s, np.float32), self.soft, dtype=np.float32, nsplit=128)
        return f32(a), f32(j)

    def _listed(self, q, v, lists):
        t = _state(q, v, self.s)
        p, pv = f32(q), f32(v)
        if self.sums == "f64":
            a, j = R.list_f64(p, pv, lists[0], lists[1], t, self.soft)[:2]
        else:
            a, j = R.list_f32(p, pv, lists[0], lists[1], t, self.soft)[:2]
        return f32(a), f32(j)

    def step(self, dt):
        dt = np.float32(dt)
        qp, vp = H.predict(self.q, self.v, self.a0, self.j0, dt)
        qp, vp = H._r32(qp), H._r32(vp)
        if self.m + 1 < self.n_irr:
            aI1, jI1 = self._listed(qp, vp, self.lists)
            tau = elapsed(1 if self.wrong == WRONG[2] else self.m + 1, dt)
            aRt, jRt = poly(self.aR, self.jR, self.a2R, self.a3R, tau)
            a1, j1 = aI1 + aRt, jI1 + jRt   # fp32
            self.aI, self.jI = aI1, jI1
            self.m += 1
        else:
            a1, j1 = self._full(qp, vp)
            new = self._neighbours(qp)
            aIn, jIn = self._listed(qp, vp, new)
            aIo, jIo = (aIn, jIn) if self.wrong == WRONG[0] else self._listed(qp, vp, self.lists)
            A1, J1 = a1 - aIo, j1 - jIo   # fp32
            self.a2R, self.a3R = derivatives(self.aR, self.jR, A1, J1, elapsed(self.n_irr, dt), keep_x2=self.wrong == WRONG[1])
            self.aR, self.jR, self.aI, self.jI, self.lists = a1 - aIn, j1 - jIn, aIn, jIn, new
            self.m = 0
            self.regular += 1
        self.q, self.v = H.correct(self.q, self.v, self.a0, self.j0, a1, j1, dt, state32=True)
        self.a0, self.j0 = a1, j1
        self.steps += 1
        self.time += float(dt)

    def run(self, dt, steps):
        for _ in range(steps):
            self.step(dt)
        return self

    def state(self):
        return _state(self.q, self.v, self.s)

    def forces(self):
        return {k: getattr(self, k) for k in NAMES}


def run(s, h, n_irr, steps, soft, dt, sums="f64", wrong=None):
    return Scheme(s, h, n_irr, soft, sums, wrong).run(dt, steps)


def distance(x, y):
    """(largest |dq|, largest |dv|) over the bodies between two state dicts."""
    dq = np.sqrt(sum((np.asarray(x[k], np.float64) - np.asarray(y[k], np.float64)) ** 2 for k in Q)).max()
    dv = np.sqrt(sum((np.asarray(x[k], np.float64) - np.asarray(y[k], np.float64)) ** 2 for k in V)).max()
    return float(dq), float(dv)


def energy(s, soft, g=H.G):
    """Total energy of a state dict in fp64, softened: sum m v^2 / 2 - sum_{i<j} G m_i m_j / sqrt(r^2 + soft^2)."""
    q, v, m = H._stack(s, Q), H._stack(s, V), np.asarray(s["m"], np.float64)
    ke = 0.5 * float((m * (v * v).sum(0)).sum())
    d = q[:, None, :] - q[:, :, None]
    r = np.sqrt((d * d).sum(0) + float(soft) ** 2)
    np.fill_diagonal(r, np.inf)
    pe = -0.5 * float(g) * float((m[:, None] * m[None, :] / r).sum())
    return ke + pe


# ---- inputs ------------------------------------------------------------------------------------------------------------------
system = R.system
radii = R.radii
SIZES = (1025, 2049)


def time_step(s, soft, fraction=0.02):
    """A step for the unit-cube system: `fraction` of the shortest |a| / |j| over the bodies, in fp64, rounded to fp32."""
    a, j = H.acc_jerk_f64(s, soft)
    return np.float32(fraction * float(np.min(np.sqrt((a * a).sum(0) / (j * j).sum(0)))))

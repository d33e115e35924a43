"""What tests/test_hermite_coverage.py (GPU) and tests/test_hermite_coverage_host.py (CPU) share: the truth and the bounds of a
sparse-mass probe of the acceleration + jerk sweep, the inputs that put the deciding body of the adaptive step into a chosen
slot, and the binary that makes murbhip_evolve's step ring wrap.  numpy only; nothing here touches a device.

The bounds are the project's own.  Accelerations: oracle.probe_err <= TOL_F64_MAX (tests/test_pair_coverage.py).  Jerks:
hermite_ref.scaled_err <= C 2^-24 with C = JERK_MARGIN x what hermite_ref.acc_jerk_sources attains in float32 against its own
fp64 result on the same probe (the rule of tests/test_hermite_gpu.py) — from the CPU alone, never from a device's output."""
import numpy as np

import hermite_adaptive_ref as A
import hermite_ref as H
from oracle import probe_err, probe_power     # pure numpy there; tests/conftest.py puts oracle/ on the path

TOL_F64_MAX = 2e-6       # tests/test_gpu_parity.py, forces
JERK_MARGIN = 4.0        # tests/test_hermite_gpu.py
POWER_FACTOR = 10.0      # a probe must show one term at 10 x the bound on 99 % of the bodies (tests/test_pair_coverage.py)
TILE, GROUP = 512, 16    # slots per layout tile (MURB_TILE_BODIES), i bodies per workgroup of the sweep (4 waves x 4)
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")


class Truth:
    """fp64 (a, j) of a probe state due to its sources, the term-magnitude sums, C of the jerk bound (units of 2^-24) and
    the share of each body's smallest jerk term; asserts the probe's power to show one term."""

    def __init__(self, ps, src, soft):
        self.a, self.j, self.abs_a, self.abs_j, min_j = H.acc_jerk_sources(ps, src, soft)
        a32, j32, _, _, _ = H.acc_jerk_sources(ps, src, soft, np.float32)
        self.acc32 = float(probe_err(a32, self.a, self.abs_a).max(initial=0.0))
        self.c32 = float(H.scaled_err(j32, self.j, self.abs_j).max(initial=0.0)) * 2.0 ** 24
        self.c = JERK_MARGIN * self.c32
        self.power = probe_power(self.abs_j, min_j)
        need = POWER_FACTOR * self.c * 2.0 ** -24
        assert (self.power >= need).mean() >= 0.99, (f"jerk probe too weak: 1 % share {np.quantile(self.power, 0.01):.2e}, "
                                                     f"needs {need:.2e} (C = {self.c:.2f})")


def where(i):
    """A body's place in the sweep (one shard: slot = body), for a failure message."""
    return f"body {i} (tile {i // TILE}, offset {i % TILE}; i group {i // GROUP}, lane {i % GROUP})"


def check(got_a, got_j, truth, what):
    """Every body of a probe against `truth`; returns the line of figures (also printed) for the record."""
    assert all(np.isfinite(x).all() for x in tuple(got_a) + tuple(got_j)), what
    ea = probe_err(got_a, truth.a, truth.abs_a)
    ej = H.scaled_err(got_j, truth.j, truth.abs_j) * 2.0 ** 24
    wa, wj = (int(np.argmax(e)) if len(e) else 0 for e in (ea, ej))
    line = (f"{what}: acc {ea[wa]:.2e} of the source terms (bound {TOL_F64_MAX:.0e}; float32 numpy {truth.acc32:.1e}); "
            f"jerk {ej[wj]:.2f} x 2^-24 (bound C = {truth.c:.2f})")
    print(line)
    assert ea[wa] <= TOL_F64_MAX, f"{what}: acceleration of {where(wa)} off by {ea[wa]:.3e}; {(ea > TOL_F64_MAX).sum()} bodies over"
    assert ej[wj] <= truth.c, (f"{what}: jerk of {where(wj)} off by {ej[wj]:.2f} x 2^-24 of its source terms, bound {truth.c:.2f}; "
                               f"{(ej > truth.c).sum()} bodies over")
    return line


def predicted(ps, a0, j0, dt):
    """The probe state at hermite_ref.predict of (q, v) with the given fp32 (a0, j0), rounded to fp32: what the sweep of a step
    of size dt is given."""
    qp, vp = H.predict(H._stack(ps, Q), H._stack(ps, V), np.stack(a0), np.stack(j0), dt)
    p = {k: np.array(v) for k, v in ps.items()}
    for i in range(3):
        p[Q[i]], p[V[i]] = qp[i].astype(np.float32), vp[i].astype(np.float32)
    return p


# ---- where the deciding body sits ---------------------------------------------------------------------------------------
# The adaptive corrector and murb_evolve_first_kernel give slots 2 t, 2 t + 1 to thread t of workgroups of 256 threads: a
# workgroup spans 512 slots, wave w of it the slots 128 w ... 128 w + 127, lane l the pair 2 l, 2 l + 1.
FAST_BODY, FAST_FACTOR = 0, np.float32(1024.0)
ETA, ETA_START, DECIDE_STEPS, DECIDE_DURATION = 0.02, 0.01, 4, 1.0e6
MARGIN = 1.02            # the runner-up's step over the deciding body's: a condition on the inputs
_LANES = (0, 15, 16, 31, 32, 47, 48, 63)

TARGET_GROUPS = {
    "wave0": list(range(128)),
    "waves1to3": [128 * w + 2 * lane + h for w in (1, 2, 3) for lane in _LANES for h in (0, 1)],
    "workgroups1and2": [512 * g + 2 * lane + h for g in (1, 2) for lane in _LANES for h in (0, 1)],
    "edges": [511, 512, 1023, 1024],
}


def fast_state(base):
    """`base` with the velocity of body FAST_BODY multiplied by 1024 (exact in fp32)."""
    s = {k: np.array(v, np.float32) for k, v in base.items()}
    for k in V:
        s[k][FAST_BODY] *= FAST_FACTOR
    return s


def swapped(s, t):
    """`s` with the bodies FAST_BODY and t exchanged (every field): the same physics under other labels."""
    out = {k: np.array(v) for k, v in s.items()}
    for v in out.values():
        v[[FAST_BODY, t]] = v[[t, FAST_BODY]]
    return out


def decider(body_steps):
    """(arg-min, runner-up / minimum) of a vector of per-body steps."""
    o = np.argsort(body_steps, kind="stable")
    return int(o[0]), (float(body_steps[o[1]] / body_steps[o[0]]) if len(o) > 1 else np.inf)


class Replay:
    """The restatement's view of a recorded run, fed with the (a, j) downloaded around every replayed step."""

    def __init__(self, a0, j0, duration, eta=ETA, eta_start=ETA_START):
        self.a0, self.j0, self.duration, self.eta, self.t = np.stack(a0), np.stack(j0), duration, eta, 0.0
        steps = A.first_body_steps(self.a0, self.j0, eta_start)
        self.deciders = [decider(steps)]
        with np.errstate(over="ignore"):
            self.cand = np.float32(steps.min(initial=np.inf))

    def want(self):
        """The fp32 step the rule takes next."""
        return A.choose(self.cand, self.t, self.duration, 0.0, self.duration)[0]

    def took(self, dt, a1, j1):
        a1, j1 = np.stack(a1), np.stack(j1)
        steps = A.body_steps(self.a0, self.j0, a1, j1, dt, self.eta)
        self.deciders.append(decider(steps))
        with np.errstate(over="ignore"):
            self.cand = np.float32(steps.min(initial=np.inf))
        self.a0, self.j0, self.t = a1, j1, self.t + float(dt)

    def dt_next(self):
        return A.clamp(self.cand, 0.0, self.duration)


# ---- the run that wraps the step ring -------------------------------------------------------------------------------------
# hermite_adaptive_ref.binary(0.9) at softening 1e6: 850 steps over 5 periods at eta 0.02 (BINARY_TABLE), the count goes with
# 1 / sqrt(eta).  eta 0.005 over 18 periods: 6121 steps of 628 s ... 3.6e5 s in the restatement.
RING = 4096              # MURB_EVOLVE_RING
RING_SOFT, RING_ETA, RING_PERIODS = 1e6, 0.005, 18.0
RING_STEPS = (4500, 8000)


def ring_run():
    """(state, duration): the duration a whole number of seconds, so that the clocks of a run in pieces are exact sums."""
    s, period = A.binary(0.9)
    return s, float(round(RING_PERIODS * period))

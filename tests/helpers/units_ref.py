"""Inputs and fp64 truth for the tests that leave the SI regime of the reference's `galaxy` / `random` schemes: a Plummer
sphere in seven unit systems, and exact power-of-two rescalings of it.  numpy only; nothing here touches a device or the
oracle library (whose G is compiled in).

    plummer(n, seed)     Hénon units (G = M = 1, virial radius 1), equal masses, rounded once to float32
    SYSTEMS              name -> (g, length scale, body mass, softening); system(name, n) builds the entry
                         System(g, state, soft, dt): velocities virial, dt about 1/64 of a crossing time
    acc_jerk_f64 / _f32  hermite_ref._evaluate on gm = float32(g) * float32(m), the value the upload stores: the truth, and
                         what plain float32 arithmetic attains on the same input (128 partial sums per body)
    acc_f32_cubed_first  the same float32 sum with the pair factor formed as gm * ((inv * inv) * inv): the order that leaves
                         the float32 range on large systems, kept to show that the bound of the GPU tests sees it
    energy_f64, moments_f64   plain fp64, physical masses
    rescale(sys, a, bm, bg, c)   lengths and softening x 2^a, masses x 2^bm, g x 2^bg, velocities x 2^c (all exact in fp32)
                         with the exact binary exponents by which every result must change
    ranges / in_range    the smallest and largest non-zero magnitude, over all pairs and in fp64, of every intermediate of
                         the one-sided order; in_range: all inside [2^-118, 2^120], eight binades clear of either end of the
                         normal float32 range, so that neither an underflow nor flush-to-zero (which loading the oracle
                         library switches on for the process) takes part in a float32 result
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import hermite_ref as H

Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
R_MAX = 6.0                       # bodies beyond 6 virial radii are drawn again (0.6 % of the mass of the model)
LO, HI = 2.0 ** -118, 2.0 ** 120
CROSSING = 2.0 * np.sqrt(2.0)     # crossing time in Hénon units

System = namedtuple("System", "g state soft dt")

# name -> (g, length scale, body mass (None: 1/n), softening)
SYSTEMS = {
    "henon": (1.0, 1.0, None, 1e-3),
    "au_msun_yr": (39.478, 2e4, 1.0, 10.0),
    "si_1e9m": (6.67384e-11, 1e9, 1e20, 2e8),
    "si_1e13m": (6.67384e-11, 1e13, 2e30, 1e9),
    "si_1e15m": (6.67384e-11, 1e15, 2e30, 1e11),
    "si_1pc": (6.67384e-11, 3.086e16, 2e30, 1e13),
    "small": (1.0, 2.0 ** -30, None, 2.0 ** -40),
}
# The seed of the sample, per body count (and per system where one seed does not serve all seven).  The bodies nearest the
# centre feel forces that cancel to a small net pull, and plain float32 arithmetic loses 1e-6 or more of it on one body in a
# few thousand of an unlucky sample; these samples keep the honest float32 yardstick at or below half of the GPU tests'
# bound on every system (tests/test_units_host.py asserts it and lists the values).
SEEDS = {1500: 11, 2048: 6, 2049: 7, 3035: 12, 4100: 2, ("si_1e15m", 2049): 1}


def seed_of(name, n):
    return SEEDS.get((name, n), SEEDS.get(n, 1))


# the ladder of the exact-covariance tests: lengths x 2^a, masses x 2^bm, g x 2^bg; velocities x 2^c with
# 2 c = bg + bm - a (the system stays virial), so only tuples with an even sum are taken
LADDER_A, LADDER_BM, LADDER_BG = (-30, 0, 20, 40, 54), (-20, 0, 60, 100), (-34, 0, 5)


def ladder():
    """Every (a, bm, bg, c) of the ladder that keeps the system virial with an integer c, the identity left out."""
    out = []
    for a in LADDER_A:
        for bm in LADDER_BM:
            for bg in LADDER_BG:
                if (bg + bm - a) % 2 == 0 and (a, bm, bg) != (0, 0, 0):
                    out.append((a, bm, bg, (bg + bm - a) // 2))
    return out


def _pair_potential(q, m, block=256):
    """sum_{i<j} m_i m_j / |q_i - q_j| in fp64 (no softening)."""
    n = q.shape[1]
    tot = 0.0
    for i0 in range(0, n, block):
        d = q[:, None, :] - q[:, i0:i0 + block, None]
        r2 = (d * d).sum(0)
        np.fill_diagonal(r2[:, i0:], np.inf)
        tot += ((m[None, :] * m[i0:i0 + block, None]) / np.sqrt(r2)).sum()
    return 0.5 * tot


@lru_cache(maxsize=None)
def _plummer64(n, seed):
    rng = np.random.default_rng([seed, n])
    q = np.zeros((3, n))
    v = np.zeros((3, n))
    for i in range(n):
        while True:     # radius from the cumulative mass, model units (scale length 1); R_MAX virial radii = R_MAX 16/(3 pi)
            r = 1.0 / np.sqrt(rng.uniform(1e-10, 1.0) ** (-2.0 / 3.0) - 1.0)
            if r <= R_MAX * 16.0 / (3.0 * np.pi):
                break
        while True:     # speed as a share x of the escape speed: density x^2 (1 - x^2)^(7/2), by rejection
            x, y = rng.uniform(0.0, 1.0), rng.uniform(0.0, 0.1)
            if y < x * x * (1.0 - x * x) ** 3.5:
                break
        speed = x * np.sqrt(2.0) * (1.0 + r * r) ** -0.25
        for vec, length in ((q, r), (v, speed)):
            z = rng.uniform(-1.0, 1.0)
            phi = rng.uniform(0.0, 2.0 * np.pi)
            s = np.sqrt(1.0 - z * z)
            vec[:, i] = length * np.array([s * np.cos(phi), s * np.sin(phi), z])
    m = np.full(n, 1.0 / n)
    q -= q.mean(1, keepdims=True)
    v -= v.mean(1, keepdims=True)
    if n > 1:
        q *= 2.0 * _pair_potential(q, m)                                       # virial radius G M^2 / (2 |W|) = 1
        v *= np.sqrt(0.5 * _pair_potential(q, m) / (0.5 * (m * (v * v).sum(0)).sum()))   # 2 K = |W|
    return q, v, m


def plummer(n, seed=1):
    """State dict of float32 arrays: a Plummer sphere of n equal masses in Hénon units, centre of mass at rest at the origin,
    virial radius 1 and 2 K = |W| (both of the unsoftened fp64 sample, before the one rounding to float32)."""
    q, v, m = _plummer64(n, seed)
    s = {k: q[i].astype(np.float32) for i, k in enumerate(Q)}
    s.update({k: v[i].astype(np.float32) for i, k in enumerate(V)})
    s["m"] = m.astype(np.float32)
    return s


@lru_cache(maxsize=None)
def system(name, n):
    """System(g, state, soft, dt) of SYSTEMS[name] with n bodies; treat the arrays as read-only (shared between tests)."""
    g, length, mass, soft = SYSTEMS[name]
    q, v, m = _plummer64(n, seed_of(name, n))
    mass = 1.0 / n if mass is None else mass
    vscale = np.sqrt(g * mass * n / length)
    s = {k: (q[i] * length).astype(np.float32) for i, k in enumerate(Q)}
    s.update({k: (v[i] * vscale).astype(np.float32) for i, k in enumerate(V)})
    s["m"] = np.full(n, mass, np.float32)
    for x in s.values():
        x.setflags(write=False)
    return System(np.float32(g), s, np.float32(soft), np.float32(CROSSING * length / vscale / 64.0))


# ------------------------------------------------------------------------------------------------------------------ truth
def gm32(sy):
    """float32(g) * float32(m) rounded to float32: what murbhip_upload stores."""
    return np.float32(sy.g) * np.asarray(sy.state["m"], np.float32)


def acc_jerk_f64(sy, want_abs=False):
    """fp64 (a, j[, sum of |jerk terms|]) of a system, each (3, n)."""
    a, j, ab = H._evaluate(H._stack(sy.state, Q), H._stack(sy.state, V), gm32(sy).astype(np.float64), np.float64(sy.soft),
                           want_abs=want_abs)
    return (a, j, ab) if want_abs else (a, j)


def acc_jerk_f32(sy, nsplit=128):
    """The honest float32 yardstick: the same formulas and the same gm in numpy float32, `nsplit` partial sums per body."""
    a, j, _ = H._evaluate(H._stack(sy.state, Q, np.float32), H._stack(sy.state, V, np.float32), gm32(sy), sy.soft,
                          dtype=np.float32, nsplit=nsplit)
    return a, j


def acc_f32_cubed_first(sy, nsplit=128, block=128):
    """float32 accelerations (3, n) with the pair factor formed as gm * ((inv * inv) * inv)."""
    f = np.float32
    q, gm = H._stack(sy.state, Q, f), gm32(sy)
    n = q.shape[1]
    soft2 = f(sy.soft) * f(sy.soft)
    bounds = [(n * k) // nsplit for k in range(nsplit + 1)]
    a = np.zeros((3, n), f)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for i0 in range(0, n, block):
            d = q[:, None, :] - q[:, i0:i0 + block, None]
            inv = f(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2)
            s = gm[None, :] * ((inv * inv) * inv)
            for k in range(3):
                t = s * d[k]
                out = np.zeros(t.shape[0], f)
                for lo, hi in zip(bounds[:-1], bounds[1:]):
                    if hi > lo:
                        out = out + t[:, lo:hi].sum(1, dtype=f)
                a[k, i0:i0 + block] = out
    return a


def rel_err(test, truth):
    """Per body |test - truth| / |truth| of (3, n) vectors, in fp64."""
    t = np.stack([np.asarray(c, np.float64) for c in test])
    r = np.stack([np.asarray(c, np.float64) for c in truth])
    return np.sqrt(((t - r) ** 2).sum(0)) / np.maximum(np.sqrt((r ** 2).sum(0)), np.finfo(np.float64).tiny)


def energy_f64(sy, state=None, block=256):
    """(kinetic, potential) in fp64: sum 1/2 m v^2 and -sum_{i<j} g m_i m_j / sqrt(r_ij^2 + soft^2) (include/murbhip.h)."""
    s = sy.state if state is None else state
    q, v, m = H._stack(s, Q), H._stack(s, V), np.asarray(sy.state["m"], np.float64)
    soft2 = np.float64(sy.soft) ** 2
    n, tot = q.shape[1], 0.0
    for i0 in range(0, n, block):
        d = q[:, None, :] - q[:, i0:i0 + block, None]
        r2 = (d * d).sum(0) + soft2
        np.fill_diagonal(r2[:, i0:], np.inf)
        tot += ((m[None, :] * m[i0:i0 + block, None]) / np.sqrt(r2)).sum()
    return float((0.5 * m * (v * v).sum(0)).sum()), float(-0.5 * np.float64(sy.g) * tot)


def moments_f64(sy, state=None):
    """P = sum m v, L = sum m q x v, Mq = sum m q, M, and the sums of the term magnitudes the errors are measured against."""
    s = sy.state if state is None else state
    q, v, m = H._stack(s, Q), H._stack(s, V), np.asarray(sy.state["m"], np.float64)
    qn, vn = np.sqrt((q * q).sum(0)), np.sqrt((v * v).sum(0))
    want = {"P": (m * v).sum(1), "L": (m * np.cross(q.T, v.T).T).sum(1), "Mq": (m * q).sum(1), "M": float(m.sum())}
    scale = {"P": (m * vn).sum(), "L": (m * qn * vn).sum(), "Mq": (m * qn).sum(), "M": float(m.sum())}
    return want, scale


# ------------------------------------------------------------------------------------------------------- fixed-step schemes
def _acc(q, gm, soft, dtype):
    return H._evaluate(q, None, gm, soft, dtype=dtype, nsplit=1 if dtype is np.float64 else 128)[0]


def euler(sy, steps, dtype=np.float64):
    """"integrator" 0 (include/murbhip.h): k = a dt, q += (v + k/2) dt, v += k.  dtype float64: every operation in fp64 and
    nothing rounded; float32: the device's arithmetic — k and v in fp32, the position update in fp64 rounded once."""
    f = dtype
    q, v = H._stack(sy.state, Q, f), H._stack(sy.state, V, f)
    gm, dt = gm32(sy).astype(f), f(sy.dt)
    for _ in range(steps):
        k = _acc(q, gm, f(sy.soft), f) * dt
        q = (q.astype(np.float64) + (v.astype(np.float64) + k.astype(np.float64) * 0.5) * np.float64(dt)).astype(f)
        v = v + k
    return q, v


def leapfrog(sy, steps, dtype=np.float64):
    """"integrator" 1: kick-drift-kick with one force evaluation per step and the closing half kick at the read-out."""
    f = dtype
    q, v = H._stack(sy.state, Q, f), H._stack(sy.state, V, f)
    gm, dt = gm32(sy).astype(f), f(sy.dt)
    for it in range(steps):
        h = f(0.5) * dt if it == 0 else f(0.5) * (dt + dt)
        v = v + _acc(q, gm, f(sy.soft), f) * h
        q = (q.astype(np.float64) + v.astype(np.float64) * np.float64(dt)).astype(f)
    v = v + _acc(q, gm, f(sy.soft), f) * (f(0.5) * dt)
    return q, v


def hermite(sy, steps, dtype=np.float64):
    """"integrator" 2 through hermite_ref's predictor and corrector; float32: the sweep in numpy float32 and q, v, a, j rounded
    at the device's stores (hermite_ref's state32)."""
    f32 = dtype is np.float32
    if not f32:
        out = H.hermite_f64(sy.state, steps, np.float64(sy.soft), sy.dt, gm=gm32(sy))
        return H._stack(out, Q), H._stack(out, V)
    q, v = H._stack(sy.state, Q), H._stack(sy.state, V)
    gm = gm32(sy).astype(dtype)
    rnd = H._r32 if f32 else (lambda x: x)

    def ev(qq, vv):
        a, j, _ = H._evaluate(qq, vv, gm, dtype(sy.soft), dtype=dtype, nsplit=128 if f32 else 1)
        return a.astype(np.float64), j.astype(np.float64)

    a0, j0 = ev(q, v)
    for _ in range(steps):
        qp, vp = H.predict(q, v, a0, j0, sy.dt)
        a1, j1 = ev(rnd(qp), rnd(vp))
        q, v = H.correct(q, v, a0, j0, a1, j1, sy.dt, f32)
        a0, j0 = a1, j1
    return q, v


SCHEMES = {0: euler, 1: leapfrog, 2: hermite}


# ---------------------------------------------------------------------------------------------------------------- rescaling
def rescale(sy, a, bm, bg, c):
    """(system, exponents): lengths and softening x 2^a, masses x 2^bm, g x 2^bg, velocities x 2^c, dt x 2^(a-c); the binary
    exponents by which the results change exactly: acc, jerk, ke, pe, and the moments P, L, Mq, M."""
    s = {k: np.ldexp(sy.state[k], a) for k in Q}
    s.update({k: np.ldexp(sy.state[k], c) for k in V})
    s["m"] = np.ldexp(sy.state["m"], bm)
    for k, x in s.items():
        assert x.dtype == np.float32 and np.array_equal(np.ldexp(x, -{"q": a, "v": c, "m": bm}[k[0]]), sy.state[k]), k
    out = System(np.ldexp(sy.g, bg), s, np.ldexp(sy.soft, a), np.ldexp(sy.dt, a - c))
    exps = {"acc": bg + bm - 2 * a, "jerk": bg + bm + c - 3 * a, "ke": bm + 2 * c, "pe": bg + 2 * bm - a,
            "P": bm + c, "L": bm + a + c, "Mq": bm + a, "M": bm}
    return out, exps


def ranges(sy, block=256):
    """name -> (smallest, largest) non-zero magnitude in fp64 over all pairs (the self pairs included where the kernels
    evaluate them) of the intermediates of the one-sided order, of the per-body sums and of the pair-potential term."""
    q, v = H._stack(sy.state, Q), H._stack(sy.state, V)
    gm = gm32(sy).astype(np.float64)
    soft2 = np.float64(sy.soft) ** 2
    n = q.shape[1]
    out, total = {}, 0.0

    def see(name, x):
        x = np.abs(x[x != 0])
        if x.size:
            lo, hi = out.get(name, (np.inf, 0.0))
            out[name] = (min(lo, float(x.min())), max(hi, float(x.max())))

    for name, x in (("q", q), ("v", v), ("gm", gm), ("soft2", np.array([soft2]))):
        see(name, x)
    for i0 in range(0, n, block):
        d = q[:, None, :] - q[:, i0:i0 + block, None]
        w = v[:, None, :] - v[:, i0:i0 + block, None]
        r2 = (d * d).sum(0) + soft2
        inv = 1.0 / np.sqrt(r2)
        inv2 = inv * inv
        gi = gm[None, :] * inv
        s = gi * inv2
        dw = (d * w).sum(0)
        c = -3.0 * (dw * inv2)
        t = w + c * d
        for name, x in (("r2", r2), ("inv2", inv2), ("gm*inv", gi), ("s", s), ("s*d", s * d), ("d.w", dw), ("c", c),
                        ("acc", (s * d).sum(2)), ("jerk", (s * t).sum(2)), ("phi", gi.sum(1)),
                        ("pair potential", gi * gm[i0:i0 + block, None])):
            see(name, x)
        total += float((gi * gm[i0:i0 + block, None]).sum())
    out["pair potential, summed"] = (total, total)     # all terms are positive: no partial sum of them is larger
    return out


def _shift(r, a, bm, bg, c):
    """ranges() of a rescaled system from those of its base: every magnitude moves by an exact power of two."""
    gm_e = bg + bm
    e = {"q": a, "v": c, "gm": gm_e, "soft2": 2 * a, "r2": 2 * a, "inv2": -2 * a, "gm*inv": gm_e - a, "s": gm_e - 3 * a,
         "s*d": gm_e - 2 * a, "d.w": a + c, "c": c - a, "acc": gm_e - 2 * a,
         "jerk": gm_e - 3 * a + c, "phi": gm_e - a, "pair potential": 2 * gm_e - a, "pair potential, summed": 2 * gm_e - a}
    return {k: (np.ldexp(lo, e[k]), np.ldexp(hi, e[k])) for k, (lo, hi) in r.items()}


def in_range(sy=None, r=None):
    """True when every magnitude of ranges(sy) (or of the given ranges) lies inside [2^-118, 2^120]."""
    r = ranges(sy) if r is None else r
    return all(LO <= lo and hi <= HI for lo, hi in r.values())


@lru_cache(maxsize=None)
def base_ranges(name, n):
    return ranges(system(name, n))


def ladder_in_range(n, name="henon"):
    """The ladder tuples whose rescaled system (of SYSTEMS[name] with n bodies) satisfies in_range."""
    r = base_ranges(name, n)
    return [t for t in ladder() if in_range(r=_shift(r, *t))]

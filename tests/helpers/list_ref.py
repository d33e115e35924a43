"""The field of listed bodies (murblist_of / murblist_at / murbsplit_of), restated from include/murblist.h, and the inputs that
tests/test_list_host.py (CPU) and tests/test_list_gpu.py (GPU) share.  numpy only; nothing here touches a device.

    point p, list idx[offsets[p]:offsets[p + 1]], every entry j used exactly as given:
    d = q_j - p    w = v_j - pv    r2 = |d|^2 + soft^2
    a_p = sum G m_j d r2^(-3/2)     j_p = sum G m_j (w - 3 (d.w) d / r2) r2^(-3/2)     phi_p = sum G m_j r2^(-1/2)

No skip: a body in its own list counts (d = 0: G m / soft to phi, nothing to a), a duplicate counts twice.

The bound is tests/helpers/field_ref.py's, unchanged (scaled_errors / check are its functions): a point's error is scaled by the
sum of the magnitudes of its terms and bounded by C * 2^-24 with C = 4 x what a plain numpy float32 evaluation of the same lists
(every term in float32, a list's terms added in order in float32) attains against fp64 — the largest figure over the points of
the case, per quantity, computed on the CPU and never from a device's output.

RULES names deliberately wrong readings of the definition, for the tests that show the inputs tell them apart."""
import numpy as np

import field_ref as F
import hermite_ref as H

Q, V, KEYS = F.Q, F.V, F.KEYS
SOFT = F.SOFT
U24 = F.U24
STEP = 128   # entries of a lane step
RULES = ("own body skipped although listed", "a duplicate counted once", "the slot past the end counted")


def csr(lists):
    """(offsets uint64, idx int32) of a sequence of lists."""
    lens = np.array([len(x) for x in lists], np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    idx = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return offsets, idx.astype(np.int32)


def lists_of(offsets, idx):
    o = np.asarray(offsets, np.int64)
    return [np.asarray(idx[o[p]:o[p + 1]], np.int64) for p in range(o.shape[0] - 1)]


def complement(n, bodies, offsets, idx):
    """(offsets, idx): per listed body every other body not in its list, ascending, the body itself left out (the restatement of
    murbhip.complement_lists, written independently: set difference per body)."""
    out = []
    for b, mine in zip(np.asarray(bodies, np.int64), lists_of(offsets, idx)):
        out.append(np.array(sorted(set(range(n)) - set(int(x) for x in mine) - {int(b)}), np.int32))
    return csr(out)


def _apply_rule(lists, own, rule):
    if rule is None:
        return lists
    assert rule in RULES, rule
    out = []
    for p, mine in enumerate(lists):
        mine = np.asarray(mine, np.int64)
        if rule == RULES[0] and own is not None and own[p] >= 0:
            mine = mine[mine != own[p]]
        elif rule == RULES[1]:
            _, first = np.unique(mine, return_index=True)
            mine = mine[np.sort(first)]
        elif rule == RULES[2] and len(mine) % STEP:
            mine = np.concatenate([mine, np.full(STEP - len(mine) % STEP, mine[-1], np.int64)])   # the last entry, counting
        out.append(mine)
    return out


def _segments(terms, offsets, dtype):
    """Per list the sum of its terms in order, in `dtype` (np.add.reduceat adds sequentially); an empty list gives 0."""
    o = np.asarray(offsets, np.int64)
    out = np.zeros(o.shape[0] - 1, dtype)
    full = np.diff(o) > 0
    if full.any():
        out[full] = np.add.reduceat(np.asarray(terms, dtype), o[:-1][full], dtype=dtype)
    return out


def _eval(points, pvel, offsets, idx, q, v, gm, soft, dtype, want_abs):
    points = np.asarray(points, dtype).reshape(3, -1)
    count = points.shape[1]
    pvel = np.zeros((3, count), dtype) if pvel is None else np.asarray(pvel, dtype).reshape(3, -1)
    o = np.asarray(offsets, np.int64)
    j = np.asarray(idx, np.int64)
    assert o.shape == (count + 1,) and o[0] == 0 and j.shape == (int(o[-1]),)
    who = np.repeat(np.arange(count), np.diff(o))
    q, v, gm = np.asarray(q, dtype), np.asarray(v, dtype), np.asarray(gm, dtype)
    soft2 = dtype(soft) * dtype(soft)
    d = q[:, j] - points[:, who]
    w = v[:, j] - pvel[:, who]
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
        inv = dtype(1.0) / np.sqrt(r2)
        inv2 = inv * inv
        g = gm[j] * inv
        s = g * inv2
        c = dtype(-3.0) * ((d[0] * w[0] + d[1] * w[1] + d[2] * w[2]) * inv2)
        ta = [s * d[k] for k in range(3)]
        tj = [s * (w[k] + c * d[k]) for k in range(3)]
        a = np.stack([_segments(ta[k], o, dtype) for k in range(3)])
        jk = np.stack([_segments(tj[k], o, dtype) for k in range(3)])
        phi = _segments(g, o, dtype)
        ab = {}
        if want_abs:
            norm = lambda t: np.sqrt(sum(np.asarray(x, np.float64) ** 2 for x in t))    # noqa: E731
            ab = {"a": _segments(norm(ta), o, np.float64), "j": _segments(norm(tj), o, np.float64),
                  "phi": _segments(np.asarray(g, np.float64), o, np.float64)}
    return a, jk, phi, ab


def list_f64(points, pvel, offsets, idx, state, soft, rule=None, own=None):
    """fp64 (a (3, P), j (3, P), phi (P), abs) of the listed bodies of `state` at `points` moving with `pvel` (None: at rest).
    rule: None, or one of RULES (own: per point the body it sits on, or -1)."""
    if rule is not None:
        offsets, idx = csr(_apply_rule(lists_of(offsets, idx), own, rule))
    return _eval(points, pvel, offsets, idx, H._stack(state, Q), H._stack(state, V), H._gm(state), soft, np.float64, True)


def list_f32(points, pvel, offsets, idx, state, soft):
    """The same formula in plain numpy float32, a list's terms added in order."""
    a, j, phi, _ = _eval(points, pvel, offsets, idx, H._stack(state, Q, np.float32), H._stack(state, V, np.float32),
                         H._gm(state, np.float32), soft, np.float32, False)
    return a, j, phi


def bound_of(points, pvel, offsets, idx, state, soft, ref=None):
    """(ref, C): list_f64's result and, per quantity, C of the bound in units of 2^-24 (field_ref.bound_of's rule)."""
    ref = list_f64(points, pvel, offsets, idx, state, soft) if ref is None else ref
    e = F.scaled_errors(list_f32(points, pvel, offsets, idx, state, soft), ref)
    return ref, {k: 4.0 * float(np.max(v, initial=0.0)) / U24 for k, v in e.items()}


check = F.check
scaled_errors = F.scaled_errors


def add_refs(x, y):
    """The fp64 reference of two disjoint source lists together: values and magnitudes add."""
    return x[0] + y[0], x[1] + y[1], x[2] + y[2], {k: x[3][k] + y[3][k] for k in x[3]}


def as_tuple(d):
    """(a (3, P), j (3, P), phi) of a dict with KEYS, in fp64."""
    return (np.stack([d[k] for k in KEYS[:3]]).astype(np.float64), np.stack([d[k] for k in KEYS[3:6]]).astype(np.float64),
            np.asarray(d["phi"], np.float64))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
system = F.system
body_points = F.body_points
RADII = (0.0, 0.05, 0.1, 0.2, 0.45)
LENGTHS = (1, 2, 3, 127, 128, 129, 255, 256, 257)   # and n - 1


def radii(n):
    """One radius per body, cycling through RADII."""
    return np.array(RADII, np.float32)[np.arange(n) % len(RADII)]


def neighbours_f32(s, h, soft):
    """(offsets, idx) of include/murbnbr.h's rule restated in float32: body j != i is listed for i if and only if
    fma-free r2 = dx^2 + dy^2 + dz^2 + soft2 <= (float)(h^2 + soft2).  The sweeps form r2 with fmas, so a pair within an ulp of the
    sphere may differ: good for counting list lengths on the CPU, not for bit comparisons."""
    q = H._stack(s, Q, np.float32)
    n = q.shape[1]
    soft2 = np.float32(soft) * np.float32(soft)
    thr = (np.asarray(h, np.float64) ** 2 + np.float64(soft2)).astype(np.float32)
    thr = np.broadcast_to(thr, (n,))
    out = []
    for i in range(n):
        d = q - q[:, i:i + 1]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + soft2
        near = r2 <= thr[i]
        near[i] = False
        out.append(np.flatnonzero(near).astype(np.int32))
    return csr(out)


def permutation(n, seed=41):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


def prefix_lists(n):
    """Hand-made lists of LENGTHS and n - 1 entries as prefixes of a fixed permutation: not ascending."""
    perm = permutation(n)
    return [perm[:k] for k in LENGTHS + (n - 1,)]

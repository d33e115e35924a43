"""numpy restatement of the minimum-spanning-tree read-out, written from the text of include/murbmst.h, not from the device or
host code.

Over an (n, n) fp32 r2 matrix (+inf on the diagonal) and a mask: Kruskal under the key (r2, min(i, j), max(i, j)); the
foreign-nearest rule by a stable argmin; one Boruvka round with the rules of the header and with deliberately wrong ones;
single-linkage groups; an edge's fp64 length; and a tie grid for small n."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nearest_ref as NR      # noqa: E402

INVALID = -2000   # MURBHIP_E_INVALID


def tie_grid(n, seed=1):
    """(state dict, soft, q_int): n cells of a full cubic grid of spacing 1 (nearest_ref.dense_side(n) cells a side, coordinates
    from 3 up) chosen and ordered by a seeded permutation, softening 0.5, so every r2 is exact in fp32 and nearly every body has
    several nearest bodies at r2 = 1.25: nearest_ref.dense_lattice's construction without its special bodies and its
    n >= 2049 floor."""
    rng = np.random.default_rng(seed)
    side = NR.dense_side(n)
    g = np.arange(side, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1) + 3
    q = cells[:, rng.permutation(side ** 3)[:n]].copy()
    v = rng.standard_normal((3, n)).astype(np.float32)
    m = rng.uniform(1.0, 2.0, n).astype(np.float32)
    s = {"qx": q[0].astype(np.float32), "qy": q[1].astype(np.float32), "qz": q[2].astype(np.float32),
         "vx": v[0], "vy": v[1], "vz": v[2], "m": m}
    return s, np.float32(0.5), q


class _Sets:
    def __init__(self, n):
        self.up = np.arange(n)

    def find(self, a):
        while self.up[a] != a:
            self.up[a] = self.up[self.up[a]]
            a = self.up[a]
        return a

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.up[max(a, b)] = min(a, b)   # the root is the set's smallest index
        return True


def kruskal(r2, member=None):
    """(i, j, r2, label): the minimum spanning forest of the members under the key (r2, min, max): edges with i < j ascending by
    the key, pairs at r2 = +inf never joined; label the smallest member index of a body's component, -1 outside the mask."""
    n = r2.shape[0]
    inside = np.ones(n, bool) if member is None else np.asarray(member) != 0
    who = np.flatnonzero(inside)
    a, b = np.triu_indices(len(who), 1)
    i, j = who[a], who[b]
    w = r2[i, j]
    keep = w < np.inf
    i, j, w = i[keep], j[keep], w[keep]
    order = np.lexsort((j, i, w))
    sets = _Sets(n)
    ei, ej, er2 = [], [], []
    for k in order:
        if len(ei) == len(who) - 1:
            break
        if sets.union(i[k], j[k]):
            ei.append(i[k]); ej.append(j[k]); er2.append(w[k])
    label = np.array([sets.find(x) if inside[x] else -1 for x in range(n)], np.int32)
    return np.array(ei, np.int32), np.array(ej, np.int32), np.array(er2, np.float32), label


def foreign(r2, label, bodies=None, highest=False):
    """(partner int32, r2 float32) of the listed bodies (None: all): the minimum by (r2, index) over the bodies j with
    label[j] >= 0 and label[j] != label[i]; -1 / +inf for a body with label < 0, and where there is none or only +inf.
    highest: the deliberately wrong rule "the highest index wins a tie"."""
    label = np.asarray(label)
    rows = np.arange(r2.shape[0]) if bodies is None else np.asarray(bodies, np.int64)
    m = r2[rows].astype(np.float32).copy()
    m[:, label < 0] = np.inf
    m[label[rows][:, None] == label[None, :]] = np.inf
    m[label[rows] < 0] = np.inf
    if highest:
        j = m.shape[1] - 1 - np.argmin(m[:, ::-1], 1)
    else:
        j = np.argmin(m, 1)   # the first of equal values: the lowest index
    best = m[np.arange(len(rows)), j]
    none = ~(best < np.inf)
    return np.where(none, -1, j).astype(np.int32), np.where(none, np.inf, best).astype(np.float32)


def boruvka_round(label, partner, r2, by_r2_alone=False):
    """(label, i, j, r2) of one round by the header's rules, or None where an edge would close a cycle.  by_r2_alone: the
    deliberately wrong rule "the component's minimum by r2 alone, the first body seen"."""
    label = np.asarray(label).copy()
    n = len(label)
    best = {}
    for i in range(n):
        if label[i] < 0 or partner[i] < 0:
            continue
        e = (np.float32(r2[i]), min(i, int(partner[i])), max(i, int(partner[i])))
        have = best.get(label[i])
        if have is None or (e[0] < have[0] if by_r2_alone else e < have):
            best[label[i]] = e
    chosen = sorted(set(best.values()))
    sets = _Sets(n)
    first = {}
    for a in range(n):
        if label[a] >= 0:
            sets.union(a, first.setdefault(label[a], a))
    for _, a, b in chosen:
        if not sets.union(a, b):
            return None
    out = np.array([sets.find(a) if label[a] >= 0 else label[a] for a in range(n)], np.int32)
    return (out, np.array([e[1] for e in chosen], np.int32), np.array([e[2] for e in chosen], np.int32),
            np.array([e[0] for e in chosen], np.float32))


def start_labels(n, member=None):
    inside = np.ones(n, bool) if member is None else np.asarray(member) != 0
    return np.where(inside, np.arange(n), -1).astype(np.int32)


def sort_edges(i, j, r2):
    order = np.lexsort((j, i, r2))
    return np.asarray(i)[order], np.asarray(j)[order], np.asarray(r2)[order]


def groups(n, i, j, r2, thr):
    """Single-linkage labels: the components under the edges with r2 <= thr, each under its smallest body index."""
    sets = _Sets(n)
    for a, b, w in zip(i, j, r2):
        if w <= thr:
            sets.union(int(a), int(b))
    return np.array([sets.find(a) for a in range(n)], np.int32)


def lengths(s, i, j):
    """fp64 edge lengths from the fp32 coordinates: sqrt((dx dx + dy dy) + dz dz) with d = (double)q_j - (double)q_i."""
    d = [s[k].astype(np.float64)[j] - s[k].astype(np.float64)[i] for k in ("qx", "qy", "qz")]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def total(values):
    """The sum in edge order, one addition at a time."""
    t = 0.0
    for v in values:
        t += float(v)
    return t

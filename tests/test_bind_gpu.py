"""MI355X: the bound-pair read-out (include/murbbind.h) through the C ABI, the Python interface and the plugin.  Lattices: the
partner index against tests/helpers/bind_ref.py for every body under every chunk count and launch cut, the h bits across the
cuts.  Floats (a Plummer sphere with a planted binary and a planted triple): the fp64 key bounds, the pair list, the elements
bit for bit on the device's own list, the census.  The calls as observers, and the refused calls."""
import ctypes as C
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bind_ref as B          # noqa: E402
import knn_ref as K           # noqa: E402
import nearest_ref as NR      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
TOL_F64_MAX = 2e-6       # tests/test_gpu_parity.py, forces
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
_fp, _ip, _dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)


def make_sim(gpu, s, soft, g=None, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft) if g is None else gpu.Simulation(len(s["m"]), soft=soft, g=g)
    for k, v in opts.items():
        (sim.set_field_option if k in gpu.FIELD_OPTIONS else sim.set_option)(k, v)
    sim.upload(s)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32 if x.dtype.itemsize == 4 else np.int64)


def same(a, b):
    """Two (partner, h) results, bit for bit."""
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def same_binaries(a, b):
    keys = ("i", "j") + B.ELEMENT_KEYS
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys) and \
        all(a["census"][k] == b["census"][k] or (a["census"][k] != a["census"][k] and b["census"][k] != b["census"][k]) for k in a["census"])


@lru_cache(maxsize=None)
def lattice(n):
    """(state, soft, g, q_int, v_int, lattice_stats) of bind_ref.bind_lattice(n): CPU only, computed once."""
    s, soft, g, q, v = B.bind_lattice(n)
    return s, soft, g, q, v, B.lattice_stats(q, v)


@lru_cache(maxsize=None)
def planted():
    return B.planted(3000)


def check_lattice(n, got, st, what):
    """partner equals the rule's index for EVERY body; h is within the force bound of the class's fp64 key; mutual pairs share
    their h bit for bit; body 0 next to the origin has a real partner."""
    partner, h = got
    bad = np.nonzero(partner != st["idx"])[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], partner[bad[:5]], st["idx"][bad[:5]])
    err = np.abs(h.astype(np.float64) - st["key"]) / st["scale"]
    print(f"{what}: largest |h - fp64 key| / (w2 / 2 + gs / rs) = {err.max():.3e} (bound {TOL_F64_MAX:.0e})")
    assert err.max() <= TOL_F64_MAX, what
    mutual, bound = B.pair_lists(partner, h)
    assert 2 * len(mutual) >= 0.4 * n and np.array_equal(bits(h[mutual[:, 0]]), bits(h[mutual[:, 1]])), what
    assert 0 < partner[0] < n, "body 0 picked the padding"


# ------------------------------------------------------------------------------------------------------------------ 1. lattices
def test_lattice_2049_every_chunk_count(gpu):
    """bind_lattice(2049): 5 tiles, the last of one body.  Under "field_chunks" 0, 2 and 5 partner equals the restatement's index
    for every body (ties across tiles included), and the h bits are the same under all three."""
    s, soft, g, _, _, st = lattice(2049)
    results = []
    for chunks in (0, 2, 5):
        with make_sim(gpu, s, soft, g=g, field_chunks=chunks) as sim:
            results.append(sim.bound_partner_of())
        check_lattice(2049, results[-1], st, f"n=2049 chunks={chunks}")
    assert same(results[0], results[1]) and same(results[0], results[2])


def test_lattice_5121_six_launches(gpu):
    """bind_lattice(5121) with "field_batch" 1 024: six launches, the last a ragged group of one body, under "field_chunks" 1 and
    11; and one launch of the default batch: the same indices and the same h bits."""
    s, soft, g, _, _, st = lattice(5121)
    assert gpu.field_layout(5121, 11, 1024, 5121)["batches"] == 6
    results = []
    for opts in ({"field_chunks": 1, "field_batch": 1024}, {"field_chunks": 11, "field_batch": 1024}, {}):
        with make_sim(gpu, s, soft, g=g, **opts) as sim:
            results.append(sim.bound_partner_of())
        check_lattice(5121, results[-1], st, f"n=5121 {opts}")
    assert same(results[0], results[1]) and same(results[0], results[2])


def test_padding_is_never_a_candidate(gpu):
    """A probe of G m = 100 at rest on the origin, where the padding slots lie at rest: their h = -100 / soft would be the
    smallest by far (tests/test_bind_host.py pins that).  The partner is a real body, the one the fp64 key names."""
    s, soft, g, q, v, _ = lattice(2049)
    key = 0.5 * (v.astype(np.float64) ** 2).sum(0) - 101.0 / np.sqrt((q.astype(np.float64) ** 2).sum(0) + 0.25)
    with make_sim(gpu, s, soft, g=g) as sim:
        partner, h = sim.bound_partner_at(np.zeros((3, 1), np.float32), masses=[100.0])
    assert partner[0] == key.argmin() and abs(h[0] - key.min()) <= TOL_F64_MAX * abs(key.min()) and h[0] > -200.0


# ------------------------------------------------------------------------------------------------------------------- 2. small n
@pytest.mark.parametrize("n", (1, 2, 3, 7, 16, 17))
def test_small_n(gpu, n):
    rng = np.random.default_rng(n)
    q = rng.permutation(40)[:n][None, :] * np.array([[1], [3], [7]]) + 2      # distinct integer points
    v = rng.integers(-1, 2, size=(3, n))
    s = {"m": np.ones(n, np.float32)}
    for keys, arr in ((Q, q), (V, v)):
        for k, c in zip(keys, arr):
            s[k] = c.astype(np.float32)
    with make_sim(gpu, s, np.float32(0.5), g=1.0) as sim:
        partner, h = sim.bound_partner_of()
        b = sim.binaries()
    if n == 1:
        assert partner.tolist() == [-1] and np.isposinf(h).all(), "a lone body"
        assert b["census"]["pairs"] == 0 and len(b["i"]) == 0 and math.isnan(b["census"]["a_min"]) and b["census"]["hardest_i"] == -1
        return
    st = B.lattice_stats(q, v)
    assert st["gap"].min() >= 1e-3, "the input leaves the partner undetermined"
    assert np.array_equal(partner, st["idx"]), (partner, st["idx"])
    assert (np.abs(h - st["key"]) <= TOL_F64_MAX * st["scale"]).all()
    _, bound = B.pair_lists(partner, h)
    assert np.array_equal(b["i"], bound[:, 0]) and np.array_equal(b["j"], bound[:, 1]) and b["census"]["pairs"] == len(bound)


def test_two_bodies_receding_fast(gpu):
    """Each is the other's partner with h > 0: mutual, not bound.  The pair list is empty and the census reports no bound pair."""
    s = {k: np.zeros(2, np.float32) for k in Q + V}
    s["qx"][1], s["vx"][1], s["m"] = 1.0, 10.0, np.ones(2, np.float32)
    with make_sim(gpu, s, np.float32(0.01), g=1.0) as sim:
        partner, h = sim.bound_partner_of()
        b = sim.binaries()
    assert partner.tolist() == [1, 0] and (h > 0).all() and bits(h)[0] == bits(h)[1]
    assert abs(h[0] - (50.0 - 2.0 / math.sqrt(1.0001))) <= TOL_F64_MAX * (50.0 + 2.0)
    c = b["census"]
    assert len(b["i"]) == 0 and c["pairs"] == 0 and c["mutual_pairs"] == 1 and c["bound_bodies"] == 0 and c["energy_sum"] == 0.0
    assert math.isnan(c["hardest_energy"]) and math.isnan(c["a_min"]) and c["hardest_i"] == -1 and c["hardest_j"] == -1


# --------------------------------------------------------------------------------------------------------------- 3. independence
def test_subsets_points_and_skip(gpu):
    s, soft, g, q, v, st = lattice(2049)
    n = 2049
    P, W = np.stack([s[c] for c in Q]), np.stack([s[c] for c in V])
    sub = np.array([5, 5, n - 1, 0, 14, 600, 1100, 10, 11, 2048, 17, 5], np.int32)
    with make_sim(gpu, s, soft, g=g, field_chunks=3) as sim:
        full = sim.bound_partner_of()
        part = sim.bound_partner_of(sub)
        assert same(part, (full[0][sub], full[1][sub])), "a subset with repeats"
        own = sim.bound_partner_at(P, W, s["m"], skip=np.arange(n, dtype=np.int32))
        assert same(own, full), "probes at the bodies' own (q, v, m) with themselves skipped"
        few = sim.bound_partner_at(P[:, sub], W[:, sub], s["m"][sub], skip=sub)
        assert same(few, part), "... a few of them, in another place of the call"
        # no body skipped: the lowest body with the probe's own position and velocity is found (h = -gs / soft: d = 0, w = 0)
        anyone = sim.bound_partner_at(P, W, s["m"], skip=np.full(n, -1, np.int32))
        assert same(sim.bound_partner_at(P, W, s["m"]), anyone), "skip NULL is skip = -1 for every point"
        state = np.concatenate([q, v]).T
        first = np.array([np.nonzero((state[:i + 1] == state[i]).all(1))[0][0] for i in range(n)])
        assert np.array_equal(anyone[0], first) and (np.abs(anyone[1] + 2.0 / 0.5) <= TOL_F64_MAX * 2.0 / 0.5).all()
        assert anyone[0][11] in (10, 11)
    check_lattice(n, full, st, "n=2049 chunks=3")
    with make_sim(gpu, s, soft, g=g, field_chunks=5, field_batch=256) as sim:
        assert same(sim.bound_partner_of(), full), "the bits under another cut, in another context"
        assert same(sim.bound_partner_of(sub), part)


def test_massless_probe(gpu):
    """m NULL: gs = gm_j alone, the same bits as masses of 0; a massive probe adds its own gm; velocities NULL: at rest."""
    s = {k: np.zeros(2, np.float32) for k in Q + V}
    s["qx"][1], s["vy"][1], s["m"] = 3.0, 0.5, np.array([2.0, 0.0], np.float32)
    p = np.array([[0.0], [4.0], [0.0]], np.float32)
    with make_sim(gpu, s, np.float32(0.5), g=1.0) as sim:
        bare = sim.bound_partner_at(p)
        zero = sim.bound_partner_at(p, np.zeros((3, 1), np.float32), [0.0])
        heavy = sim.bound_partner_at(p, masses=[1.0])
        moving = sim.bound_partner_at(p, np.array([[0.0], [0.5], [0.0]], np.float32))
    assert same(bare, zero) and bare[0][0] == 0
    assert abs(bare[1][0] + 2.0 / math.sqrt(16.25)) <= TOL_F64_MAX * 2.0 / math.sqrt(16.25), "gs = gm_j"
    assert heavy[0][0] == 0 and abs(heavy[1][0] + 3.0 / math.sqrt(16.25)) <= TOL_F64_MAX * 3.0 / math.sqrt(16.25), "gs = gm_j + gm_p"
    # moving with the massless body 1: against body 0, h = 0.125 - 2 / sqrt(16.25) = -0.371; against body 1, w = 0, gs = 0: h = +0
    assert moving[0][0] == 0 and moving[1][0] < 0


# --------------------------------------------------------------------------------------------------------------------- 4. floats
def check_state(sim, s, g, soft, what, elements=True):
    """Every body's chosen partner against the fp64 key matrix of the state `s`, with no exclusions; the pair list against the
    call's own arrays; the elements against bind_ref on the device's own list, bit for bit; the census.

    The bound on a choice, asserted in two forms.  As include/murbbind.h's arithmetic gives it: the device takes p over the
    fp64 minimum j only if its fp32 h(p) <= h(j); each fp32 value lies within TOL_F64_MAX of its fp64 key relative to that
    pair's own scale w2 / 2 + gs / rs, so key(p) - key(j) is at most TOL_F64_MAX * (scale(p) + scale(j)), 2 * TOL_F64_MAX
    relative to the mean of the two pairs' scales.  And with one scale, the chosen pair's own: key(p) - key(j) is at most
    2 * TOL_F64_MAX * scale(p).  Neither implies the other where the two scales differ, so both must hold."""
    n = len(s["m"])
    rows = np.arange(n)
    partner, h = sim.bound_partner_of()
    key, scale = B.key_matrix(s, g, soft)
    best = key.argmin(1)
    assert ((partner >= 0) & (partner < n) & (partner != rows)).all(), what
    excess = (key[rows, partner] - key[rows, best]) / (scale[rows, partner] + scale[rows, best])
    own = (key[rows, partner] - key[rows, best]) / scale[rows, partner]
    err = np.abs(h.astype(np.float64) - key[rows, partner]) / scale[rows, partner]
    print(f"{what}: choice off by at most {excess.max():.3e} of both scales' sum (bound {TOL_F64_MAX:.0e}), {own.max():.3e} of its own "
          f"scale (bound {2 * TOL_F64_MAX:.0e}), h by {err.max():.3e} (bound {TOL_F64_MAX:.0e}); "
          f"{(partner != best).sum()} bodies chose another than the fp64 minimum")
    assert excess.max() <= TOL_F64_MAX and own.max() <= 2 * TOL_F64_MAX and err.max() <= TOL_F64_MAX, what
    b = sim.binaries()
    mutual, bound = B.pair_lists(partner, h)
    assert np.array_equal(b["i"], bound[:, 0]) and np.array_equal(b["j"], bound[:, 1]), what
    assert np.array_equal(bits(h[bound[:, 0]]), bits(h[bound[:, 1]])), what
    c = b["census"]
    assert c["pairs"] == len(bound) and c["mutual_pairs"] == len(mutual) and c["bound_bodies"] == int((h < 0).sum()), what
    if not elements:
        return partner, h, b
    want = B.state_elements(s, g, soft, bound)
    have = np.stack([b[k] for k in B.ELEMENT_KEYS], 1)
    assert ((bits(have) == bits(want)) | (np.isnan(have) & np.isnan(want))).all(), what
    ref = B.census(partner, h, bound, want)
    assert abs(c["energy_sum"] - ref[1]) <= 1e-12 * math.fsum(np.abs(want[:, 4])), (what, c["energy_sum"], ref[1])
    assert (c["hardest_i"], c["hardest_j"]) == (int(ref[2]), int(ref[3])) and c["hardest_energy"] == ref[4] and c["a_min"] == ref[5], what
    return partner, h, b


def test_plummer_with_planted_binary_and_triple(gpu):
    s, soft, g, info = planted()
    with make_sim(gpu, s, soft, g=g) as sim:
        partner, h, b = check_state(sim, s, g, soft, "plummer + planted")
    pairs = set(zip(b["i"].tolist(), b["j"].tolist()))
    assert info["binary"] in pairs and info["inner"] in pairs
    outer = info["outer"]
    assert partner[outer] in info["inner"] and h[outer] < 0 and outer not in b["i"] and outer not in b["j"]
    k = b["i"].tolist().index(info["binary"][0])
    assert abs(b["a"][k] - 0.01) < 1e-3 and abs(b["e"][k] - 0.5) < 0.05 and b["r"][k] > 5 * float(soft)
    assert b["census"]["hardest_i"] == info["inner"][0] and b["census"]["pairs"] >= 2


# --------------------------------------------------------------------------------------------------------------- 5. after steps
def test_after_steps_and_evolve(gpu):
    """The same checks on the state download_state returns after Hermite steps, after evolve, and after steps of "integrator" 0.
    Under "integrator" 1 in flight the device's velocities lag the positions by half a step and download_state returns
    synchronised ones, so only what does not need the half-step velocities is compared: the indices are valid, mutual pairs share
    their h bits, and the pair list and the counts follow from the call's own arrays."""
    s, soft, g, _ = planted()
    with make_sim(gpu, s, soft, g=g, integrator=2) as sim:
        sim.steps(2.0 ** -12, 3)
        now = dict(sim.state(), m=s["m"])
        assert not np.array_equal(now["qx"], s["qx"])
        check_state(sim, now, g, soft, "after 3 Hermite steps")
        out = sim.evolve(2.0 ** -9, max_steps=8)
        assert out["steps"] >= 1
        check_state(sim, dict(sim.state(), m=s["m"]), g, soft, "after evolve")
    with make_sim(gpu, s, soft, g=g) as sim:      # "integrator" 0
        sim.steps(2.0 ** -12, 3)
        check_state(sim, dict(sim.state(), m=s["m"]), g, soft, "after 3 steps, integrator 0")
    with make_sim(gpu, s, soft, g=g, integrator=1) as sim:
        sim.steps(2.0 ** -12, 3)
        partner, h = sim.bound_partner_of()
        b = sim.binaries()
        n = len(s["m"])
        assert ((partner >= 0) & (partner < n) & (partner != np.arange(n))).all()
        mutual, bound = B.pair_lists(partner, h)
        assert np.array_equal(bits(h[mutual[:, 0]]), bits(h[mutual[:, 1]]))
        assert np.array_equal(b["i"], bound[:, 0]) and np.array_equal(b["j"], bound[:, 1])
        assert b["census"]["pairs"] == len(bound) and b["census"]["mutual_pairs"] == len(mutual) and b["census"]["bound_bodies"] == int((h < 0).sum())


def test_options_that_ride_in_the_records_are_not_read(gpu):
    """With "contact" on, the radii ride in the velocity records' spare lanes: the read-out's bits do not change.  Nor with
    "nearest" or "potential" on."""
    s, soft, g, _ = planted()
    with make_sim(gpu, s, soft, g=g) as sim:
        want = sim.bound_partner_of()
    for opts in ({"integrator": 2, "contact": 1}, {"integrator": 2, "nearest": 1}, {"integrator": 2, "potential": 1}):
        with make_sim(gpu, s, soft, g=g, **opts) as sim:
            if "contact" in opts:
                sim.upload_radii(np.full(len(s["m"]), 0.01, np.float32))
            sim.compute_acc_jerk()
            assert same(sim.bound_partner_of(), want), opts


# ------------------------------------------------------------------------------------------------------------------ 6. observers
def test_observers_leave_the_run_alone(gpu):
    """A run with the three calls interleaved leaves every later bit unchanged: state, a / j, knn_of, field_of; and each call
    returns the same bits as when it is the only observer at that point."""
    s, soft, g, _ = planted()
    p = np.stack([s[c] for c in Q])[:, :50] + np.float32(0.01)
    who = np.arange(0, 3000, 37, dtype=np.int32)
    seen = {}

    def run(probe):
        calls = (lambda sim: sim.bound_partner_of(), lambda sim: sim.binaries(),
                 lambda sim: sim.bound_partner_at(p, masses=np.ones(50, np.float32)))

        def look(sim, at):
            if probe == "all":
                seen[at] = tuple(call(sim) for call in calls)
            elif probe is not None and at == 2:      # one of the three, alone in the whole run, behind the second pair of steps
                seen["only", probe] = calls[probe](sim)
        with make_sim(gpu, s, soft, g=g, integrator=2) as sim:
            look(sim, 0)
            for k in range(2):
                sim.steps(2.0 ** -12, 2)
                look(sim, 1 + k)
            out = sim.evolve(2.0 ** -10, max_steps=6)
            look(sim, 3)
            st = sim.state()
            f = sim.field_of(who)
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.jerk()) + list(sim.knn_of(who, k=6)) + [f[k] for k in sorted(f)]
            return [bits(x) for x in rec], out

    (a, out_a), (b, out_b) = run(None), run("all")
    assert out_a == out_b
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for which in range(3):      # each call in a context that has seen no other observer, not even itself
        (c, out_c) = run(which)
        assert out_c == out_a and all(np.array_equal(x, y) for x, y in zip(a, c)), which
    assert same(seen["only", 0], seen[2][0]), "bound_partner_of: the same bits as the only observer"
    assert same_binaries(seen["only", 1], seen[2][1]), "binaries: the same bits as the only observer"
    assert same(seen["only", 2], seen[2][2]), "bound_partner_at: the same bits as the only observer"
    assert len(seen[2][1]["i"]) >= 2, "the comparison needs pairs"


def test_refusals(gpu):
    s, soft = NR.lattice(600)
    n = 600
    lib = gpu.lib()
    P = [np.ascontiguousarray(s[c][:20] + np.float32(0.5)) for c in Q]
    W = [np.ascontiguousarray(s[c][:20]) for c in V]
    m = np.ones(20, np.float32)
    skip = np.full(20, -1, np.int32)
    partner, h = np.zeros(20, np.int32), np.zeros(20, np.float32)
    fp = lambda x: x.ctypes.data_as(_fp) if x is not None else None      # noqa: E731
    ip = lambda x: x.ctypes.data_as(_ip) if x is not None else None      # noqa: E731

    def at(count=20, pos=P, vel=W, mass=m, sk=skip):
        return lib.murbbind_at(sim._h, count, *[fp(x) for x in pos], *[fp(x) for x in vel], fp(mass), ip(sk), ip(partner), fp(h))

    def of(bodies, count=None):
        b = np.ascontiguousarray(bodies, np.int32)
        return lib.murbbind_of(sim._h, len(b) if count is None else count, ip(b), ip(partner), fp(h))

    def pairs(capacity=0, arrays=(None, None, None), count=True, out=True):
        cnt, out8 = C.c_ulong(12345), (C.c_double * 8)(*([77.0] * 8))
        i, j, e = arrays
        rc = lib.murbbind_pairs(sim._h, ip(i), ip(j), e.ctypes.data_as(_dp) if e is not None else None, capacity,
                                C.byref(cnt) if count else None, out8 if out else None)
        return rc, cnt.value, list(out8)

    def refused(code, rc, what):
        """The call returned its code, and a following call returns what it returned before."""
        assert rc == code, (what, rc)
        assert same(sim.bound_partner_at(np.stack(P), np.stack(W), m, skip), before) and same(sim.bound_partner_of(np.arange(16)), bodies_before), what
        assert same_binaries(sim.binaries(), binaries_before), what

    with gpu.Simulation(n, soft=soft) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE and pairs()[0] == E_STATE, "before the first upload"
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        assert lib.murbbind_at(None, 20, *[fp(x) for x in P], *[fp(x) for x in W], fp(m), None, ip(partner), fp(h)) == E_INVALID, "no context"
        sim.upload(s)
        before = sim.bound_partner_at(np.stack(P), np.stack(W), m, skip)
        bodies_before = sim.bound_partner_of(np.arange(16))
        binaries_before = sim.binaries()
        refused(E_INVALID, at(pos=[None, P[1], P[2]]), "one position array missing")
        for hole in range(3):
            for keep in range(3):
                vel = [None] * 3
                vel[keep] = W[keep]
                refused(E_INVALID, at(vel=vel), "one velocity array of three")
            vel = list(W)
            vel[hole] = None
            refused(E_INVALID, at(vel=vel), "two velocity arrays of three")
        refused(E_INVALID, lib.murbbind_of(sim._h, 3, None, ip(partner), fp(h)), "all bodies, but count != n")
        for bad in (np.nan, np.inf, -np.inf):
            for arr in P + W:
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate or velocity of {bad}")
        for bad in (-1.0, -0.5, np.nan, np.inf):
            mm = m.copy()
            mm[3] = bad
            refused(E_INVALID, at(mass=mm), f"a mass of {bad}")
        for bad in (-2, n, 2 ** 31 - 1):
            sk = skip.copy()
            sk[19] = bad
            refused(E_INVALID, at(sk=sk), f"skip entry {bad}")
        for bad in (-1, n, -2 ** 31):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
        refused(E_INVALID, pairs(count=False)[0], "no count")
        refused(E_INVALID, pairs(out=False)[0], "no out8")
        have = len(binaries_before["i"])
        assert have >= 2, "the capacity rule needs pairs"
        i, j, e = np.full(have, -7, np.int32), np.full(have, -7, np.int32), np.full((have, 6), -7.0)
        refused(E_INVALID, pairs(have, (i, None, e))[0], "some but not all of i, j, elems")
        rc, cnt, out8 = pairs(have - 1, (i, j, e))
        assert rc == E_INVALID and cnt == have and out8[0] == have and out8[7] >= have, "the capacity rule: count and out8 filled"
        assert (i == -7).all() and (j == -7).all() and (e == -7.0).all(), "... and the arrays untouched"
        rc, cnt, out8 = pairs()
        assert rc == 0 and cnt == have and out8[0] == have, "NULL arrays ask for the count and out8 alone"
        rc, cnt, _ = pairs(have + 5, (i, j, e))
        assert rc == 0 and cnt == have and np.array_equal(i, binaries_before["i"]) and np.array_equal(j, binaries_before["j"])
        assert at(vel=[None] * 3, mass=None, sk=None) == 0 and of([n - 1, 0]) == 0
        assert lib.murbbind_at(sim._h, 20, *[fp(x) for x in P], *[fp(x) for x in W], fp(m), None, None, None) == 0, "either output may be NULL"
        assert lib.murbbind_of(sim._h, 2, ip(np.array([1, 2], np.int32)), None, None) == 0


def test_open_block_and_two_shards_are_refused(gpu):
    s, soft = K.plummer(3000)

    def run(probe):
        with make_sim(gpu, s, soft, g=1.0, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, sim.bound_partner_of) == E_STATE and code_of(gpu, sim.binaries) == E_STATE
                assert code_of(gpu, lambda: sim.bound_partner_at(np.zeros((3, 2), np.float32))) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(x) for x in sim.bound_partner_of()]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    d, soft_d, g, _, _, _ = lattice(2049)
    with gpu.Simulation(2049, soft=soft_d, g=g, devices=[0, 0]) as sim:
        sim.upload(d)
        assert code_of(gpu, sim.bound_partner_of) == E_STATE and code_of(gpu, sim.binaries) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the sweep launches as spans of the kind "bind" (40 points under "field_batch" 16: three launches; the
    600 bodies of binaries(): 38), outside the force_* figures and the field's spans."""
    s, soft = NR.lattice(600)

    def run(level, bind):
        with make_sim(gpu, s, soft, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if bind:
                sim.bound_partner_of(np.arange(40))
                sim.bound_partner_at(np.zeros((3, 3), np.float32))
                sim.binaries()
            sim.field_of([0, 1])
            return {k: sim.info(k) for k in ("span_bind_count", "span_bind_ms_avg", "span_field_count", "span_knn_count", "force_launches")}

    with_it, without = run(2, True), run(2, False)
    assert with_it["span_bind_count"] == 3 + 1 + 2 * 38 and with_it["span_bind_ms_avg"] > 0
    assert without["span_bind_count"] == 0 == without["span_bind_ms_avg"] and with_it["span_knn_count"] == 0
    assert with_it["span_field_count"] == without["span_field_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)["span_bind_count"] == 0


# ---------------------------------------------------------------------------------------------------------------------- 7. plugin
def test_plugin_binaries(gpu):
    """HostSim.binaries() (SimulationNBodyHIP::binaries) equals Simulation.binaries() of the same bodies, after an iteration too."""
    n, soft, dt = 2049, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt) as host:
        for _ in range(2):
            st = host.state()
            got = host.binaries()
            with gpu.Simulation(n, soft=soft) as sim:
                sim.upload(st)
                want = sim.binaries()
                partner, h = sim.bound_partner_of()
            assert same_binaries(got, want)
            _, bound = B.pair_lists(partner, h)
            assert np.array_equal(got["i"], bound[:, 0]) and got["census"]["pairs"] == len(bound)
            print(f"galaxy n={n}: {got['census']}")
            host.step(1)

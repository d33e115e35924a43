"""MI355X: the nearest body of another label and the minimum spanning tree (include/murbmst.h) through the C ABI, the Python
interface and the plugin.  The sweep against knn_of bit for bit and against tests/helpers/mst_ref.py under random labels, the tree
against Kruskal as an exact edge set, the groups against friends-of-friends, the mass segregation ratio, the calls as observers,
and the refused calls."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import knn_ref as K           # noqa: E402
import mst_ref as R           # noqa: E402
import nearest_ref as NR      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
SHAPES = (1, 2, 3, 127, 128, 129, 511, 512, 513, 1024, 1025, 1664, 2049)   # both sides of a lane step, a tile and four tiles
_fp, _ip, _dp, _bp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)


def make_sim(gpu, s, soft, g=1.0, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft, g=g)
    for k, v in opts.items():
        (sim.set_field_option if k in gpu.FIELD_OPTIONS else sim.set_option)(k, v)
    sim.upload(s)
    return sim


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.int32, 8: np.int64}[x.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_pair(a, b):
    return same(a[0], b[0]) and same(a[1], b[1])


def tiles_of(n):
    return (n + 511) // 512


def settings(n):
    """Every "field_chunks" from 1 to the tile count, each with the default "field_batch" and with 16 (several launches)."""
    return [dict(field_chunks=c, **batch) for c in range(1, tiles_of(n) + 1) for batch in ({}, {"field_batch": 16})]


@lru_cache(maxsize=None)
def fixture(kind, n):
    """(state, soft, fp32 r2 matrix with +inf on the diagonal, or None for the Plummer sphere).  Do not modify."""
    if kind == "plummer":
        s, soft = K.plummer(n)
        return s, soft, None
    if kind == "lattice":
        s, soft = NR.lattice(n)
        q = np.stack([s[k].astype(np.int64) for k in ("qx", "qy", "qz")])
    elif kind == "grid":
        s, soft, q = R.tie_grid(n)
    else:
        s, soft, q = NR.dense_lattice(n)
    return s, soft, NR.r2_matrix(q, np.float32(soft) * np.float32(soft))


@lru_cache(maxsize=None)
def kruskal_of(kind, n):
    return R.kruskal(fixture(kind, n)[2])


def library_r2(sim, n):
    """The library's own r2 matrix: every pair's r2 from neighbours_of with a radius that holds everything."""
    offsets, idx, r2 = sim.neighbours_of(h=1e6)
    m = np.full((n, n), np.inf, np.float32)
    rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
    m[rows, idx] = r2
    assert len(idx) == n * (n - 1)
    return m


def random_labels(n, groups, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, max(groups, 1), n).astype(np.int32)
    lab[rng.random(n) < 0.4] = -1 - rng.integers(0, 3)
    return lab


CASES = [(kind, n) for kind in ("lattice", "grid", "plummer") for n in SHAPES] + [("dense", 2049)]


# ----------------------------------------------------------------------------------------------------------- 1. against knn
@pytest.mark.parametrize("kind,n", CASES)
def test_foreign_of_own_labels_is_knn(gpu, kind, n):
    """label[i] = i: foreign_nearest equals knn_of(k = 1) bit for bit under every chunk count and both launch cuts."""
    s, soft, r2 = fixture(kind, n)
    first = None
    for opts in settings(n):
        with make_sim(gpu, s, soft, **opts) as sim:
            got = sim.foreign_nearest(np.arange(n))
            idx, w = sim.knn_of(k=1)
        assert same_pair(got, (idx[:, 0], w[:, 0])), (opts, np.nonzero(got[0] != idx[:, 0])[0][:5])
        first = first or got
        assert same_pair(got, first), opts
    if r2 is not None:
        assert same_pair(first, R.foreign(r2, np.arange(n)))


# -------------------------------------------------------------------------------------------------------- 2. random labels
@pytest.mark.parametrize("kind,n", CASES)
def test_random_labels_against_the_reference(gpu, kind, n):
    """2, 7 and n // 3 groups with 40 % of the bodies outside, under every chunk count: exactly the reference's (partner, r2), on
    the Plummer sphere with the reference run on the library's own r2 matrix; one label everywhere gives -1 / +inf; a shuffled
    list with repeats returns each body's own bits."""
    s, soft, r2 = fixture(kind, n)
    rng = np.random.default_rng(n)
    who = rng.integers(0, n, n + 5).astype(np.int32)
    wanted = {}   # the reference of a label set, computed once: the settings must not change a bit
    for opts in settings(n):
        with make_sim(gpu, s, soft, **opts) as sim:
            if r2 is None:
                r2 = library_r2(sim, n)
                if n > 1:   # the matrix is knn_of's: its rows sorted give knn_of's values
                    kk = min(8, n - 1)
                    assert same(np.sort(r2, 1)[:, :kk], sim.knn_of(k=kk)[1])
            for groups in (2, 7, n // 3):
                lab = random_labels(n, groups, seed=groups)
                if groups not in wanted:
                    wanted[groups] = R.foreign(r2, lab)
                got, want = sim.foreign_nearest(lab), wanted[groups]
                assert same_pair(got, want), (opts, groups, np.nonzero(got[0] != want[0])[0][:5])
                assert np.all(got[0][lab < 0] == -1) and np.all(np.isinf(got[1][lab < 0]))
                listed = sim.foreign_nearest(lab, who)
                assert same_pair(listed, (want[0][who], want[1][who])), (opts, groups)
            alone = sim.foreign_nearest(np.full(n, 3))
            assert np.all(alone[0] == -1) and np.all(np.isinf(alone[1]))


# ------------------------------------------------------------------------------------------------------------- 3. the tree
def check_tree(gpu, sim, s, n, want, r2):
    t = sim.spanning_tree()
    assert same(t["i"], want[0]) and same(t["j"], want[1]) and same(t["r2"], want[2]), "Kruskal's edge list, exactly"
    assert same(t["label"], want[3])
    assert same(t["length"], R.lengths(s, want[0], want[1])), "the fp64 length formula, exactly"
    assert (t["members"], t["edges"], t["components"]) == (n, n - 1, 1)
    assert t["rounds"] <= int(np.ceil(np.log2(n)))
    if n > 1:
        assert t["total_length"] == R.total(t["length"]) and t["mean_length"] == t["total_length"] / (n - 1)
        assert t["longest_length"] == t["length"].max()
    else:
        assert t["total_length"] == 0.0 and t["mean_length"] != t["mean_length"] and t["longest_length"] == 0.0
    # the whole call is foreign_nearest + mst_round chained from Python, round by round
    lab, ei, ej, ew, rounds = R.start_labels(n), [], [], [], 0
    while len(ei) < n - 1:
        partner, w = sim.foreign_nearest(lab)
        if r2 is not None:
            assert same_pair((partner, w), R.foreign(r2, lab)), rounds
        lab, i, j, w, added = gpu.mst_round(lab, partner, w)
        assert added > 0
        rounds += 1
        ei += list(i); ej += list(j); ew += list(w)
    chained = R.sort_edges(np.array(ei, np.int32), np.array(ej, np.int32), np.array(ew, np.float32))
    assert same(chained[0], t["i"]) and same(chained[1], t["j"]) and same(chained[2], t["r2"]) and rounds == t["rounds"]
    assert same(lab, t["label"])
    return t


@pytest.mark.parametrize("kind,n", [c for c in CASES if c[0] != "plummer"])
def test_tree_against_kruskal(gpu, kind, n):
    s, soft, r2 = fixture(kind, n)
    want = kruskal_of(kind, n)
    first = None
    for opts in settings(n)[::2] + settings(n)[-1:]:   # every chunk count, and the last with several launches
        with make_sim(gpu, s, soft, **opts) as sim:
            t = check_tree(gpu, sim, s, n, want, r2) if first is None else sim.spanning_tree()
        first = first or t
        assert all(same(t[k], first[k]) for k in ("i", "j", "r2", "length", "label")) and t["rounds"] == first["rounds"], opts
    print(kind, n, "rounds", first["rounds"], "total length", first["total_length"])


@pytest.mark.parametrize("n", SHAPES)
def test_tree_of_a_plummer_sphere(gpu, n):
    """Kruskal over the library's own r2 matrix."""
    s, soft, _ = fixture("plummer", n)
    with make_sim(gpu, s, soft) as sim:
        r2 = library_r2(sim, n)
        check_tree(gpu, sim, s, n, R.kruskal(r2), r2)


@pytest.mark.parametrize("kind,n", [("lattice", 513), ("lattice", 1664), ("grid", 1025), ("dense", 2049)])
def test_masked_tree_is_the_tree_of_the_members(gpu, kind, n):
    """Under a mask of 60 % the tree equals the reference's, and the tree of a second context that holds the members alone, with
    its indices mapped back.  A mask of one member and of none gives no edge."""
    s, soft, r2 = fixture(kind, n)
    mask = np.random.default_rng(n).random(n) < 0.6
    who = np.flatnonzero(mask)
    want = R.kruskal(r2, mask)
    with make_sim(gpu, s, soft, field_chunks=tiles_of(n)) as sim:
        t = sim.spanning_tree(member=mask)
        one = np.zeros(n, bool)
        one[n // 2] = True
        single, nobody = sim.spanning_tree(member=one), sim.spanning_tree(member=np.zeros(n, bool))
    assert same(t["i"], want[0]) and same(t["j"], want[1]) and same(t["r2"], want[2]) and same(t["label"], want[3])
    assert (t["members"], t["edges"], t["components"]) == (len(who), len(who) - 1, 1) and t["rounds"] <= int(np.ceil(np.log2(len(who))))
    with make_sim(gpu, {k: v[who] for k, v in s.items()}, soft) as sub:
        u = sub.spanning_tree()
    back = R.sort_edges(who[u["i"]].astype(np.int32), who[u["j"]].astype(np.int32), u["r2"])
    assert same(back[0], t["i"]) and same(back[1], t["j"]) and same(back[2], t["r2"])
    assert same(np.sort(u["length"]), np.sort(t["length"]))
    assert (single["members"], single["edges"], single["components"], single["rounds"]) == (1, 0, 1, 0)
    assert single["label"][n // 2] == n // 2 and np.all(np.delete(single["label"], n // 2) == -1)
    assert (nobody["members"], nobody["edges"], nobody["components"], nobody["rounds"]) == (0, 0, 0, 0) and np.all(nobody["label"] == -1)


def test_capacity_too_small(gpu):
    """A capacity below the edge count: MURBHIP_E_INVALID, the edge arrays untouched, out8 and label complete.  Any edge array
    may be NULL."""
    n = 513
    s, soft, _ = fixture("grid", n)
    want = kruskal_of("grid", n)
    lib = gpu.lib()
    with make_sim(gpu, s, soft) as sim:
        for cap in (0, 1, n - 2):
            i, j = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
            w, ln = np.full(n, -7, np.float32), np.full(n, -7, np.float64)
            label, out8 = np.full(n, -7, np.int32), (C.c_double * 8)(*([77.0] * 8))
            rc = lib.murbmst_of(sim._h, None, cap, i.ctypes.data_as(_ip), j.ctypes.data_as(_ip), w.ctypes.data_as(_fp),
                                ln.ctypes.data_as(_dp), label.ctypes.data_as(_ip), out8)
            assert rc == E_INVALID, cap
            assert np.all(i == -7) and np.all(j == -7) and np.all(w == -7) and np.all(ln == -7)
            assert same(label, want[3]) and list(out8)[:3] == [n, n - 1, 1] and out8[4] > 0 and out8[7] == 0.0
        out8 = (C.c_double * 8)()
        assert lib.murbmst_of(sim._h, None, 0, None, None, None, None, None, out8) == 0 and out8[1] == n - 1, "no edge array: no capacity"
        j = np.zeros(n - 1, np.int32)
        assert lib.murbmst_of(sim._h, None, n - 1, None, j.ctypes.data_as(_ip), None, None, None, out8) == 0 and same(j, want[1])


# -------------------------------------------------------------------------------------------------------------- 4. groups
@pytest.mark.parametrize("kind,n", [("grid", 513), ("lattice", 1025), ("dense", 2049), ("plummer", 1664)])
def test_groups_against_friends_of_friends(gpu, kind, n):
    """mst_groups(thr(b)) of the tree of all bodies equals fof_groups(neighbours_of(h = b)) for five linking lengths; on the grids
    b = 1 and b = sqrt(2) sit exactly on a tie."""
    s, soft, _ = fixture(kind, n)
    lengths = {"grid": (0.5, 1.0, np.sqrt(2.0), 1.2, 2.0), "dense": (0.5, 1.0, np.sqrt(2.0), 1.2, 2.0),
               "lattice": (1.0, 30.0, 60.0, 90.0, 200.0), "plummer": (0.02, 0.05, 0.1, 0.2, 0.5)}[kind]
    with make_sim(gpu, s, soft) as sim:
        t = sim.spanning_tree()
        counts = []
        for b in lengths:
            offsets, idx, _ = sim.neighbours_of(h=b)
            want = gpu.fof_groups(offsets, idx)
            got = gpu.mst_groups(n, t["i"], t["j"], t["r2"], gpu.neighbour_threshold(b, soft))
            assert same(got, want), b
            counts.append(len(set(got)))
    print(kind, n, "groups at", lengths, counts)
    assert counts[0] > counts[-1]


# ---------------------------------------------------------------------------------------------------- 5. mass segregation
def test_mass_segregation_ratio(gpu):
    """1 025 bodies of a Plummer sphere, the 20 heaviest in the centre: the ratio equals the reference's over the same seeded sets
    (the edge sets exactly, the lengths to 1e-12 relative) and is above 1."""
    n, n_mst, sets, seed = 1025, 20, 12, 4
    s, soft = K.plummer(n)
    s = {k: v.copy() for k, v in s.items()}
    centre = np.array([40.0, -25.0, 10.0])
    d = np.sqrt(sum((s[k].astype(np.float64) - c) ** 2 for k, c in zip(("qx", "qy", "qz"), centre)))
    heavy = np.argsort(d, kind="stable")[:n_mst]
    s["m"][heavy] = np.float32(5.0 / n)
    with make_sim(gpu, s, soft) as sim:
        r2 = library_r2(sim, n)
        got = sim.mass_segregation_ratio(n_mst, sets=sets, seed=seed)
        mask = np.zeros(n, bool)
        mask[heavy] = True
        tree = sim.spanning_tree(member=mask)
        with pytest.raises(ValueError):
            sim.mass_segregation_ratio(1)
    want_heavy = np.sort(np.lexsort((np.arange(n), -s["m"].astype(np.float64)))[:n_mst])
    assert np.array_equal(want_heavy, np.sort(heavy))
    ref = R.kruskal(r2, mask)
    assert same(tree["i"], ref[0]) and same(tree["j"], ref[1]), "the massive tree's edge set"
    massive = R.total(R.lengths(s, ref[0], ref[1]))
    rng = np.random.default_rng(seed)
    randoms = []
    for _ in range(sets):
        m = np.zeros(n, bool)
        m[rng.choice(np.arange(n), n_mst, replace=False)] = True
        e = R.kruskal(r2, m)
        randoms.append(R.total(R.lengths(s, e[0], e[1])))
    randoms = np.array(randoms)
    assert abs(got["length_massive"] - massive) <= 1e-12 * massive
    assert np.all(np.abs(got["lengths_random"] - randoms) <= 1e-12 * randoms)
    assert abs(got["ratio"] - randoms.mean() / massive) <= 1e-12 * got["ratio"]
    assert abs(got["sigma"] - randoms.std() / massive) <= 1e-12 * got["sigma"]
    print(f"ratio {got['ratio']:.3f} +- {got['sigma']:.3f}")
    assert got["ratio"] > 1.0


# -------------------------------------------------------------------------------------------------- 6. observer and refusals
@pytest.mark.parametrize("nearest", (0, 1))
def test_observers_leave_the_run_alone(gpu, nearest):
    """step; spanning_tree; foreign_nearest; step under "integrator" 2: every later bit (state, acc, nearest(), knn_of,
    neighbours_of) is what it is without the two read-outs, and each returns the bits it returns as the only observer."""
    n = 1025
    s, soft, _ = fixture("plummer", n)
    lab = random_labels(n, 7, seed=1)
    seen = {}

    def run(probe):
        with make_sim(gpu, s, soft, integrator=2, nearest=nearest) as sim:
            sim.steps(2.0 ** -10, 1)
            if probe in ("both", "tree"):
                seen[probe, "tree"] = sim.spanning_tree()
            if probe in ("both", "foreign"):
                seen[probe, "foreign"] = sim.foreign_nearest(lab)
            sim.steps(2.0 ** -10, 1)
            sim.sync()
            st = sim.state()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.knn_of(k=3)) + list(sim.neighbours_of(h=0.2))
            if nearest:
                rec += list(sim.nearest())
            return [bits(x) for x in rec]

    plain = run(None)
    for probe in ("both", "tree", "foreign"):
        assert all(np.array_equal(x, y) for x, y in zip(plain, run(probe))), probe
    assert all(same(seen["both", "tree"][k], seen["tree", "tree"][k]) for k in ("i", "j", "r2", "length", "label"))
    assert same_pair(seen["both", "foreign"], seen["foreign", "foreign"])


def test_refusals(gpu):
    n = 600
    s, soft, _ = fixture("plummer", n)
    lib = gpu.lib()
    lab = random_labels(n, 7, seed=2)
    partner, w = np.zeros(n, np.int32), np.zeros(n, np.float32)
    ptr = lambda x, t: x.ctypes.data_as(t) if x is not None else None      # noqa: E731

    def foreign(bodies=None, count=None, label=lab, out_p=partner, out_w=w, ctx=True):
        b = None if bodies is None else np.ascontiguousarray(bodies, np.int32)
        count = (n if b is None else len(b)) if count is None else count
        return lib.murbforeign_of(sim._h if ctx else None, count, ptr(b, _ip), ptr(label, _ip), ptr(out_p, _ip), ptr(out_w, _fp))

    def tree(out=True):
        out8 = (C.c_double * 8)(*([77.0] * 8))
        return lib.murbmst_of(sim._h, None, 0, None, None, None, None, None, out8 if out else None), list(out8)

    def refused(code, rc, what):
        """The call returned its code, and the following calls return what they returned before."""
        assert rc == code, (what, rc)
        assert same_pair(sim.foreign_nearest(lab), before) and same(sim.spanning_tree()["i"], tree_before["i"]), what

    with gpu.Simulation(n, soft=soft, g=1.0) as sim:
        assert foreign() == E_STATE and foreign([0, 1]) == E_STATE and tree()[0] == E_STATE, "before the first upload"
        assert foreign([0], count=0) == 0, "count 0 does nothing, in every state"
        assert foreign(ctx=False) == E_INVALID, "no context"
        sim.upload(s)
        before, tree_before = sim.foreign_nearest(lab), sim.spanning_tree()
        refused(E_INVALID, foreign(label=None), "no labels")
        refused(E_INVALID, foreign(out_p=None), "no partner")
        refused(E_INVALID, foreign(out_w=None), "no r2")
        refused(E_INVALID, foreign(count=3), "all bodies, but count != n")
        for bad in (-1, n, -2 ** 31, 2 ** 31 - 1):
            refused(E_INVALID, foreign([0, bad, 1]), f"body index {bad}")
        rc, out8 = tree(out=False)
        refused(E_INVALID, rc, "no out8")
        assert foreign([n - 1, 0, 0]) == 0 and tree()[0] == 0
        with pytest.raises(ValueError):
            sim.foreign_nearest(lab[:-1])
        with pytest.raises(ValueError):
            sim.spanning_tree(member=np.ones(n - 1, bool))


def test_open_block_and_two_shards_are_refused(gpu):
    n = 600
    s, soft, _ = fixture("plummer", n)
    lab = np.arange(n)

    def code_of(call):
        with pytest.raises(gpu.MurbHipError) as e:
            call()
        return e.value.code

    def run(probe):
        with make_sim(gpu, s, soft, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(sim.spanning_tree) == E_STATE and code_of(lambda: sim.foreign_nearest(lab)) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(x) for x in sim.foreign_nearest(lab)]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    with gpu.Simulation(n, soft=soft, g=1.0, devices=[0, 0]) as sim:
        sim.upload(s)
        assert code_of(sim.spanning_tree) == E_STATE and code_of(lambda: sim.foreign_nearest(lab)) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the sweep launches as spans of the kind "mst" (40 points under "field_batch" 16: three launches; a tree
    of 600 bodies: 38 a round), outside the force_* figures and the other read-outs' spans."""
    s, soft, _ = fixture("plummer", 600)

    def run(level, mst):
        with make_sim(gpu, s, soft, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            rounds = 0
            if mst:
                sim.foreign_nearest(np.arange(600), np.arange(40))
                rounds = sim.spanning_tree()["rounds"]
            sim.knn_of([0, 1], k=1)
            return rounds, {k: sim.info(k) for k in ("span_mst_count", "span_mst_ms_avg", "span_knn_count", "span_pot_count", "force_launches")}

    (rounds, with_it), (_, without) = run(2, True), run(2, False)
    assert rounds >= 1 and with_it["span_mst_count"] == 3 + rounds * 38 and with_it["span_mst_ms_avg"] > 0
    assert without["span_mst_count"] == 0 == without["span_mst_ms_avg"] and with_it["span_pot_count"] == 0
    assert with_it["span_knn_count"] == without["span_knn_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)[1]["span_mst_count"] == 0


# ------------------------------------------------------------------------------------------------------------------ 7. plugin
def test_plugin_spanning_tree(gpu):
    """HostSim.spanning_tree() (SimulationNBodyHIP::spanningTree) equals Simulation.spanning_tree() of the same bodies, after an
    iteration too."""
    n, soft, dt = 2049, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt) as host:
        for _ in range(2):
            st = host.state()
            got = host.spanning_tree()
            with gpu.Simulation(n, soft=soft) as sim:
                sim.upload(st)
                want = sim.spanning_tree()
            assert all(same(got[k], want[k]) for k in ("i", "j", "r2", "length")) and all(got[k] == want[k] for k in gpu.MST_KEYS)
            print(f"galaxy n={n}: edges {got['edges']}, rounds {got['rounds']}, mean length {got['mean_length']:.3e}")
            host.step(1)

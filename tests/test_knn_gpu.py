"""MI355X: the k-nearest-neighbour read-out (include/murbknn.h) through the C ABI, the Python interface, the plugin and
murb-hip.  Lattices: bit equality with tests/helpers/knn_ref.py under every chunk count and launch cut.  Floats (a Plummer
sphere): the r2 bounds and the list properties, column 0 against the Hermite sweeps' nearest neighbour.  Densities and the
centre against fp64 restatements on the device's own lists.  The calls as observers, and the refused calls."""
import ctypes as C
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import knn_ref as K           # noqa: E402
import nearest_ref as NR      # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
Q = ("qx", "qy", "qz")
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)


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


def same(a, b):
    """Two (idx, r2) results, bit for bit."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def bits(x):
    return np.ascontiguousarray(x).view(np.int32 if x.dtype.itemsize == 4 else np.int64)


@lru_cache(maxsize=None)
def dense(n):
    """(state, soft, q_int, soft2) of nearest_ref.dense_lattice(n): CPU only, computed once."""
    s, soft, q = NR.dense_lattice(n)
    return s, soft, q, np.float32(soft) * np.float32(soft)


@lru_cache(maxsize=None)
def dense_ref(n, k):
    _, _, q, soft2 = dense(n)
    return K.knn(q, soft2, k)


@lru_cache(maxsize=None)
def plummer():
    s, soft = K.plummer(3000)
    return s, soft


# ------------------------------------------------------------------------------------------------------------------ 1. lattices
@pytest.mark.parametrize("k", (1, 6, 8, 32))
def test_dense_lattice_every_chunk_count(gpu, k):
    """dense_lattice(2049): 5 tiles, the last of one body.  idx and r2 equal the restatement's under "field_chunks" 0, 2 and 5."""
    s, soft, _, _ = dense(2049)
    want = dense_ref(2049, k)
    for chunks in (0, 2, 5):
        with make_sim(gpu, s, soft, field_chunks=chunks) as sim:
            got = sim.knn_of(k=k)
        bad = np.nonzero((got[0] != want[0]).any(1) | (got[1] != want[1]).any(1))[0]
        assert same(got, want), (chunks, bad[:5], got[0][bad[:2]], want[0][bad[:2]])


@pytest.mark.parametrize("chunks", (1, 11))
def test_dense_lattice_eleven_tiles_six_launches(gpu, chunks):
    """dense_lattice(5121), k = 6, "field_batch" 1 024: six launches, the last a ragged group of one body."""
    s, soft, _, _ = dense(5121)
    want = dense_ref(5121, 6)
    with make_sim(gpu, s, soft, field_chunks=chunks, field_batch=1024) as sim:
        assert gpu.field_layout(5121, chunks, 1024, 5121)["batches"] == 6
        got = sim.knn_of(k=6)
    assert same(got, want)


# ------------------------------------------------------------------------------------------------------------------- 2. small n
@pytest.mark.parametrize("n", (1, 2, 3, 7, 16, 17))
def test_small_n_has_tails(gpu, n):
    rng = np.random.default_rng(n)
    q = rng.permutation(40)[:n][None, :] * np.array([[1], [3], [7]]) + 2      # distinct integer points
    s = {"qx": q[0].astype(np.float32), "qy": q[1].astype(np.float32), "qz": q[2].astype(np.float32),
         "vx": np.zeros(n, np.float32), "vy": np.zeros(n, np.float32), "vz": np.zeros(n, np.float32), "m": np.ones(n, np.float32)}
    want = K.knn(q, np.float32(0.25), 6)
    with make_sim(gpu, s, np.float32(0.5)) as sim:
        got = sim.knn_of(k=6)
    assert same(got, want)
    tail = max(0, 6 - (n - 1))
    assert tail == 0 or ((got[0][:, 6 - tail:] == -1).all() and np.isposinf(got[1][:, 6 - tail:]).all())


def test_lattice_513_known_answers(gpu):
    s, soft = NR.lattice(513)
    q = np.stack([s[c] for c in Q]).astype(np.int64)
    soft2 = np.float32(soft) * np.float32(soft)
    with make_sim(gpu, s, soft) as sim:
        got = sim.knn_of(k=3)
    assert same(got, K.knn(q, soft2, 3))
    assert got[0][20].tolist() == [21, 300, 468] and got[0][30].tolist() == [100, 512, 413]
    assert got[0][5][0] == 400 and got[1][5][0] == soft2


# --------------------------------------------------------------------------------------------------------------- 3. independence
def test_subsets_points_and_skip(gpu):
    s, soft, q, soft2 = dense(2049)
    n = 2049
    rng = np.random.default_rng(2)
    sub = rng.integers(0, n, 333).astype(np.int32)
    sub[:5] = (7, 7, 2048, 0, 7)
    p = np.stack([s[c] for c in Q])
    with make_sim(gpu, s, soft) as sim:
        everyone = sim.knn_of(k=8)
        part = sim.knn_of(sub, k=8)
        at_self = sim.knn_at(p, k=8, skip=np.arange(n, dtype=np.int32))
        at_none = sim.knn_at(p, k=8)
        at_sub = sim.knn_at(p[:, sub], k=8, skip=sub)
    assert same(part, (everyone[0][sub], everyone[1][sub]))
    assert same(at_self, everyone) and same(at_sub, part)
    want = K.knn_at(q, soft2, 8, q, np.full(n, -1))
    assert same(at_none, want)
    lead = at_none[0][:, 0]      # the body itself leads, or a lower body on the same point
    assert (at_none[1][:, 0] == soft2).all() and (lead <= np.arange(n)).all() and (lead == np.arange(n)).sum() >= n - 5


# -------------------------------------------------------------------------------------------------------------------- 4. padding
def test_padding_is_never_a_candidate(gpu):
    s, soft, q, soft2 = dense(2049)
    p = np.zeros((3, 40), np.float32)
    p[0, 1:] = np.arange(39) * 0.25
    with make_sim(gpu, s, soft) as sim:
        idx, r2 = sim.knn_at(p, k=32)
    assert (idx >= 0).all() and (idx < 2049).all()
    assert idx[0][0] == 0 and r2[0][0] == np.float32(3.0) + soft2      # body 0 at (1, 1, 1)


# --------------------------------------------------------------------------------------------------------------------- 5. floats
def check_float_lists(idx, r2, state, soft, what):
    """The r2 bounds and the list properties of lists of every body of `state`."""
    n, k = idx.shape
    ref = K.r2_f64(state, soft)
    rows = np.arange(n)[:, None]
    assert (idx >= 0).all() and (idx < n).all() and (idx != rows).all(), what
    assert all(len(set(r)) == k for r in idx.tolist()), what + ": duplicates"
    asc = (r2[:, 1:] > r2[:, :-1]) | ((r2[:, 1:] == r2[:, :-1]) & (idx[:, 1:] > idx[:, :-1]))
    assert asc.all(), what + ": not ascending in (r2, index)"
    pair = ref[rows, idx]
    e_pair = np.abs(r2.astype(np.float64) - pair) / pair
    stat = np.sort(ref, axis=1)[:, :k]
    e_stat = np.abs(pair - stat) / stat
    print(f"{what}: r2 against its pair's fp64 r2 {e_pair.max():.2e}; the pair against the order statistic {e_stat.max():.2e}")
    assert e_pair.max() <= 1e-6 and e_stat.max() <= 1e-6, what


@pytest.mark.parametrize("k", (6, 32))
def test_plummer_lists(gpu, k):
    s, soft = plummer()
    with make_sim(gpu, s, soft, g=1.0) as sim:
        check_float_lists(*sim.knn_of(k=k), s, soft, f"plummer k={k}")


def test_column_0_is_the_sweeps_nearest_and_calls_read_the_current_state(gpu):
    s, soft = plummer()
    with make_sim(gpu, s, soft, g=1.0, integrator=2, nearest=1) as sim:
        sim.compute_acc_jerk()
        nn, nr2 = sim.nearest()
        idx, r2 = sim.knn_of(k=6)
        assert np.array_equal(idx[:, 0], nn) and np.array_equal(bits(r2[:, 0]), bits(nr2))
        out = sim.evolve(2.0 ** -7, max_steps=20)
        assert out["steps"] >= 1
        now = dict(sim.state(), m=s["m"])
        assert not np.array_equal(now["qx"], s["qx"])
        idx, r2 = sim.knn_of(k=6)
        check_float_lists(idx, r2, now, soft, "after evolve")
        sim.compute_acc_jerk()
        nn, nr2 = sim.nearest()
        assert np.array_equal(idx[:, 0], nn) and np.array_equal(bits(r2[:, 0]), bits(nr2))
    with make_sim(gpu, s, soft, g=1.0) as sim:      # "integrator" 0
        sim.steps(2.0 ** -7, 5)
        now = dict(sim.state(), m=s["m"])
        assert not np.array_equal(now["qx"], s["qx"])
        check_float_lists(*sim.knn_of(k=6), now, soft, "after 5 steps")


# ------------------------------------------------------------------------------------------------------- 6. density and centre
def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(a == b, 0, d)


@pytest.mark.parametrize("which", ("plummer", "dense"))
def test_density_and_centre(gpu, which):
    """rho against the restatement on the device's own lists to 1 ulp; out8 against an fp64 restatement on the device's own rho
    to 1e-12 relative (X: relative to sum rho |q| / S1), the counts exact.  The dense lattice has bodies on one point: with k = 2
    the three of the triple are left out."""
    if which == "plummer":
        (s, soft), g, ks = plummer(), 1.0, (6, 32)
    else:
        (s, soft, _, _), g, ks = dense(2049), None, (2, 6)
    soft2 = np.float32(soft) * np.float32(soft)
    n = len(s["m"])
    q = np.stack([s[c] for c in Q])
    with make_sim(gpu, s, soft, g=g) as sim:
        for k in ks:
            idx, r2 = sim.knn_of(k=k)
            rho = sim.density(k=k)
            assert ulps(rho, K.density(idx, r2, s["m"], soft2)).max() <= 1, k
            sub = np.array([5, 5, n - 1, 0, 14], np.int32)
            assert np.array_equal(bits(sim.density(k=k, bodies=sub)), bits(rho[sub]))
            c = sim.density_centre(k=k)
            want, scale = K.centre(rho, q)
            assert c["used"] == int(want[6]) and c["left_out"] == int(want[7]) and c["used"] + c["left_out"] == n
            assert np.abs(c["x"] - want[:3]).max() <= 1e-12 * scale
            for key, w in (("r_core", want[3]), ("rho_core", want[4]), ("rho_sum", want[5])):
                assert abs(c[key] - w) <= 1e-12 * abs(w), (key, c[key], w)
            if which == "dense" and k == 2:
                assert c["left_out"] == 3 and np.isposinf(rho[list(NR.DENSE_TRIPLE)]).all()
            if which == "plummer":      # the sphere's centre, within a fraction of its scale length
                assert np.abs(c["x"] - np.array([40.0, -25.0, 10.0])).max() < 0.25 and 0.1 < c["r_core"] < 1.0


def test_centre_without_any_density_is_nan(gpu):
    """Three bodies with k = 6: every rho is +0, S1 = 0: five NaN, the counts, and the call returns 0."""
    s = {k: np.arange(3, dtype=np.float32) for k in Q + ("vx", "vy", "vz")}
    s["m"] = np.ones(3, np.float32)
    with make_sim(gpu, s, np.float32(0.5)) as sim:
        c = sim.density_centre()
        assert (sim.density() == 0).all()
    assert np.isnan(c["x"]).all() and np.isnan(c["r_core"]) and np.isnan(c["rho_core"])
    assert c["rho_sum"] == 0 and c["used"] == 3 and c["left_out"] == 0


# ------------------------------------------------------------------------------------------------------------------ 7. observers
def test_observers_leave_the_run_alone(gpu):
    s, soft = plummer()
    p = np.stack([s[c] for c in Q])[:, :50] + np.float32(0.01)

    def run(probe):
        def look(sim):
            if probe:
                sim.knn_of(k=6)
                sim.density_centre()
                sim.knn_at(p, k=8)
        with make_sim(gpu, s, soft, g=1.0, integrator=2) as sim:
            look(sim)
            for _ in range(3):
                sim.steps(2.0 ** -9, 2)
                look(sim)
            out = sim.evolve(2.0 ** -7, max_steps=10)
            look(sim)
            st = sim.state()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.jerk())
            return [bits(x) for x in rec], out

    (a, out_a), (b, out_b) = run(False), run(True)
    assert out_a == out_b
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_field_and_tidal_bits_survive_a_knn_call(gpu):
    s, soft = plummer()
    who = np.arange(0, 3000, 7, dtype=np.int32)
    with make_sim(gpu, s, soft, g=1.0) as sim:
        f0, t0 = sim.field_of(who), sim.tidal_of(who)
        sim.knn_of(k=32)
        sim.density_centre()
        f1, t1 = sim.field_of(who), sim.tidal_of(who)
    assert all(np.array_equal(bits(f0[k]), bits(f1[k])) for k in f0) and all(np.array_equal(bits(t0[k]), bits(t1[k])) for k in t0)


# -------------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(gpu):
    s, soft = NR.lattice(600)
    n = 600
    lib = gpu.lib()
    P = [np.ascontiguousarray(s[c][:20] + np.float32(0.5)) for c in Q]
    skip = np.full(20, -1, np.int32)
    idx, r2 = np.zeros((20, 6), np.int32), np.zeros((20, 6), np.float32)
    rho, out8 = np.zeros(20, np.float32), (C.c_double * 8)()
    fp = lambda x: x.ctypes.data_as(_fp)      # noqa: E731
    ip = lambda x: x.ctypes.data_as(_ip)      # noqa: E731

    def at(k=6, count=20, pos=None, sk=skip):
        pos = [fp(x) for x in P] if pos is None else pos
        return lib.murbknn_at(sim._h, k, count, *pos, ip(sk) if sk is not None else None, ip(idx), fp(r2))

    def of(bodies, k=6, count=None):
        b = np.ascontiguousarray(bodies, np.int32)
        return lib.murbknn_of(sim._h, k, len(b) if count is None else count, ip(b), ip(idx), fp(r2))

    def rho_of(bodies, k=6):
        b = np.ascontiguousarray(bodies, np.int32)
        return lib.murbdensity_of(sim._h, k, len(b), ip(b), fp(rho))

    def refused(code, rc, what):
        """The call returned its code, and a following call returns what it returned before."""
        assert rc == code, (what, rc)
        assert same(sim.knn_at(np.stack(P), k=6, skip=skip), before) and same(sim.knn_of(np.arange(16), k=6), bodies_before), what
        now = sim.density_centre()
        assert all(np.array_equal(bits(np.asarray(now[key], np.float64)), bits(np.asarray(centre_before[key], np.float64))) for key in now), what

    with gpu.Simulation(n, soft=soft) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE and rho_of([0, 1]) == E_STATE, "before the first upload"
        assert lib.murbdensity_centre(sim._h, 6, out8) == E_STATE
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        assert lib.murbknn_at(None, 6, 20, *[fp(x) for x in P], None, ip(idx), fp(r2)) == E_INVALID, "no context"
        sim.upload(s)
        before = sim.knn_at(np.stack(P), k=6, skip=skip)
        bodies_before = sim.knn_of(np.arange(16), k=6)
        centre_before = sim.density_centre()
        for k in (0, -1, 33):
            refused(E_INVALID, at(k=k), f"knn_at, k = {k}")
            refused(E_INVALID, of([0, 1], k=k), f"knn_of, k = {k}")
        for k in (0, 1, 33):
            refused(E_INVALID, rho_of([0, 1], k=k), f"density_of, k = {k}")
            refused(E_INVALID, lib.murbdensity_centre(sim._h, k, out8), f"density_centre, k = {k}")
        refused(E_INVALID, lib.murbdensity_centre(sim._h, 6, None), "no out8")
        refused(E_INVALID, at(pos=[None, fp(P[1]), fp(P[2])]), "one position array missing")
        refused(E_INVALID, lib.murbknn_of(sim._h, 6, 3, None, ip(idx), fp(r2)), "all bodies, but count != n")
        for bad in (np.nan, np.inf, -np.inf):
            for arr in P:
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate of {bad}")
        for bad in (-2, n, 2 ** 31 - 1):
            sk = skip.copy()
            sk[19] = bad
            refused(E_INVALID, at(sk=sk), f"skip entry {bad}")
        for bad in (-1, n, -2 ** 31):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
            refused(E_INVALID, rho_of([0, bad, 1]), f"density, body index {bad}")
        assert at(sk=None) == 0 and of([n - 1, 0]) == 0 and rho_of([n - 1, 0]) == 0
        assert lib.murbknn_at(sim._h, 6, 20, *[fp(x) for x in P], None, None, None) == 0, "idx and r2 may be NULL"


def test_open_block_and_two_shards_are_refused(gpu):
    s, soft = plummer()

    def run(probe):
        with make_sim(gpu, s, soft, g=1.0, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, lambda: sim.knn_of(k=6)) == E_STATE
                assert code_of(gpu, lambda: sim.knn_at(np.zeros((3, 2), np.float32))) == E_STATE
                assert code_of(gpu, sim.density) == E_STATE and code_of(gpu, sim.density_centre) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(x) for x in sim.knn_of(k=6)]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    d, soft_d, _, _ = dense(2049)
    with gpu.Simulation(2049, soft=soft_d, devices=[0, 0]) as sim:
        sim.upload(d)
        assert code_of(gpu, lambda: sim.knn_of(k=6)) == E_STATE and code_of(gpu, sim.density_centre) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the sweep launches as spans of the kind "knn" (40 points under "field_batch" 16: three launches),
    outside the force_* figures and the field's spans."""
    s, soft = NR.lattice(600)

    def run(level, knn):
        with make_sim(gpu, s, soft, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            if knn:
                sim.knn_of(np.arange(40), k=6)
                sim.density(bodies=[1, 2, 3])
            sim.field_of([0, 1])
            return {k: sim.info(k) for k in ("span_knn_count", "span_knn_ms_avg", "span_field_count", "force_launches")}

    with_it, without = run(2, True), run(2, False)
    assert with_it["span_knn_count"] == 4 and with_it["span_knn_ms_avg"] > 0 and without["span_knn_count"] == 0 == without["span_knn_ms_avg"]
    assert with_it["span_field_count"] == without["span_field_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)["span_knn_count"] == 0


# ---------------------------------------------------------------------------------------------------------------------- 9. layers
def test_tracking_density_plugin_and_driver(gpu, tmp_path):
    """`--im hip+tracking+density`: the three density_center columns equal HostSim.density_centre() of the state each of three
    iterations starts from, at n = 2 049; energy and angular momentum are hip+tracking's, whose own columns stay the centre of
    mass; murb-hip writes the same rows."""
    n, iters, soft, dt = 2049, 3, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt, tracking=True, density_centre=True) as sim:
        want = []
        for _ in range(iters):
            want.append(sim.density_centre()["x"])
            sim.step(1)
        hist = sim.history()
    with gpu.HostSim(n, "galaxy", soft, dt, tracking=True) as sim:
        sim.step(iters)
        plain = sim.history()
        s = sim.state()
    assert np.array_equal(hist["density_center"], np.array(want)) and np.isfinite(hist["density_center"]).all()
    assert np.array_equal(hist["energy"], plain["energy"]) and np.array_equal(hist["ang_momentum"], plain["ang_momentum"])
    assert not np.array_equal(hist["density_center"], plain["density_center"])
    m = s["m"].astype(np.float64)
    com = np.array([(m * s[c]).sum() / m.sum() for c in Q])      # of the end state: the columns are still a centre of mass
    assert np.abs(plain["density_center"][-1] - com).max() <= 1e-3 * np.abs(s["qx"]).max()
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    rows = {}
    for tag in ("hip+tracking+density", "hip+tracking"):
        csv = tmp_path / (tag + ".csv")
        r = subprocess.run([exe, "-n", str(n), "-i", str(iters), "--nv", "--im", tag, "--soft", str(soft), "--dt", str(dt), "--csv", str(csv)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"(--im  ): {tag}" in r.stdout
        lines = csv.read_text().splitlines()
        assert lines[0] == "iteration,energy,ang_momentum,density_center_x,density_center_y,density_center_z" and len(lines) == iters + 1
        rows[tag] = np.array([[float(x) for x in line.split(",")[1:]] for line in lines[1:]])
    for tag, h in (("hip+tracking+density", hist), ("hip+tracking", plain)):
        assert np.array_equal(rows[tag][:, 2:], h["density_center"]), tag      # the CSV holds max_digits10 digits
        assert np.allclose(rows[tag][:, 0], h["energy"], rtol=1e-5, atol=0), tag

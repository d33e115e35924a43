"""GPU: nearest neighbours from the Hermite sweeps (option "nearest") and the encounter stop of murbhip_evolve /
murbhip_evolve_block, through the C ABI and the plugin.

Yardstick: tests/helpers/nearest_ref.py (numpy, written from include/murbhip.h, pinned by tests/test_nearest_host.py): exact
integer arithmetic on a lattice, where every r2 is exact in fp32 and indices and bits must match; fp64 candidate sets
elsewhere.  The 1e-6 of the candidate sets and of r2: an fp32 r2 is one rounding per difference, squared, plus three fused
adds, at most 5 x 2^-24 = 3e-7 relative, for either candidate."""
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_adaptive_ref as A   # noqa: E402
import hermite_block_ref as B      # noqa: E402
import hermite_ref as H            # noqa: E402
import nearest_ref as N            # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
ETA, ETA_START = 0.02, 0.01
RADIUS = 3e10     # between the binary's pericentre (1e10 m) and apocentre (1.9e11 m) separations; the field bodies of
                  # cluster(256) are 5e10 m and more from each other


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hermite_sim(gpu, s, soft, nearest=1, **opts):
    sim = gpu.Simulation(len(s["qx"]), soft=soft)
    sim.set_option("integrator", 2)
    sim.set_option("nearest", nearest)
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.upload(s)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def assert_candidates(idx, r2, q, soft2, rows=None, what=""):
    """Every index lies in the fp64 candidate set of its body and r2 is within 1e-6 of the fp64 minimum."""
    best, cand = N.nearest(q, soft2)
    rows = np.arange(q.shape[1]) if rows is None else np.asarray(rows)
    assert ((idx[rows] >= 0) & (idx[rows] < q.shape[1])).all(), what + ": an index is out of range (a body was left out)"
    assert cand[rows, idx[rows]].all(), what + ": an index is not among the nearest bodies"
    err = np.abs(r2[rows].astype(np.float64) - best[rows]) / best[rows]
    print(f"{what}: largest relative r2 error {err.max():.3e}")
    assert err.max() <= 1e-6, what


# ------------------------------------------------------------------------------------------------------------- 1. exact lattice
@pytest.mark.parametrize("n", [1, 2, 513, 1024, 2049])
def test_exact_lattice(gpu, n):
    """Integer coordinates, soft 0.5: idx and r2 equal the restatement bit for bit for "jsplit" 1, 3 and 8, and among the three;
    accelerations and jerks are those of "nearest" 0, bit for bit."""
    s, soft = N.lattice(n)
    q = np.stack([s[k] for k in Q])
    want_idx, want_r2 = N.nearest(q, 0.25, exact=True)
    if n >= 513:      # the lattice holds what it is meant to
        assert want_idx[8] == 7 and s["m"][7] == 0.0 and want_idx[20] == 21 and want_idx[30] == 100
        assert want_idx[5] == 400 and want_idx[400] == 5 and want_r2[5] == np.float32(0.25)
        assert want_r2[0] > 3 * 300.0 ** 2
    plain = {}
    for jsplit in (1, 3, 8):
        with hermite_sim(gpu, s, soft, nearest=0, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            plain[jsplit] = (np.stack(sim.acc()), np.stack(sim.jerk()))
            assert code_of(gpu, sim.nearest) == E_STATE
        with hermite_sim(gpu, s, soft, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            idx, r2 = sim.nearest()
            a, j = np.stack(sim.acc()), np.stack(sim.jerk())
        assert np.array_equal(idx, want_idx), f"jsplit {jsplit}: indices differ at {np.flatnonzero(idx != want_idx)[:8]}"
        assert np.array_equal(bits(r2), bits(want_r2)), f"jsplit {jsplit}: r2 differs"
        assert np.array_equal(bits(a), bits(plain[jsplit][0])) and np.array_equal(bits(j), bits(plain[jsplit][1])), \
            f"jsplit {jsplit}: the forces changed with the option"
    if n > 1:      # r2(i, j) == r2(j, i) bit for bit: a body's neighbour has a neighbour at most as far
        assert (r2[idx] <= r2).all()


# --------------------------------------------------------------------------------------------------------------------- 2. galaxy
def test_galaxy_2049(gpu):
    n, soft = 2049, np.float32(2e8)
    with gpu.Simulation(n, soft=soft) as sim:
        sim.set_option("integrator", 2)
        sim.set_option("nearest", 1)
        sim.init_bodies("galaxy")
        sim.compute_acc_jerk()
        idx, r2 = sim.nearest()
        st = sim.state()
        sim.step(0.0)         # a step keeps the neighbours of its predicted end state: with dt = 0 that is the same state
        idx1, r21 = sim.nearest()
    q = np.stack([st[k] for k in Q])
    assert_candidates(idx, r2, q, float(soft) ** 2, what="galaxy 2049")
    assert (idx != np.arange(n)).all()
    sym = r2[idx] <= r2      # the neighbour's own nearest is at most as far: r2(i, j) == r2(j, i) bit for bit
    assert sym.all()
    assert np.array_equal(idx1, idx) and np.array_equal(bits(r21), bits(r2))


# --------------------------------------------------------------------------------------------------------- 3. block step replay
@lru_cache(maxsize=None)
def cluster(n):
    return B.cluster(n)


def snapshot(sim):
    st = sim.state()
    return {"q": np.stack([st[k] for k in Q]), "v": np.stack([st[k] for k in V]), "a": np.stack(sim.acc()),
            "j": np.stack(sim.jerk()), "ticks": sim.block_state()[0], "levels": sim.block_state()[1], "nn": sim.nearest()}


def test_block_step_replay(gpu):
    """cluster(256), one block step per call: the active bodies' values are the restatement's nearest at the predicted
    positions, the inactive bodies' (idx, r2) do not change by a bit, and "block_units" 16 and 1280 give the same bits."""
    s, period = cluster(256)
    dt_max, kmax, soft2 = float(np.float32(period / 2.0)), 12, float(np.float32(B.SOFT)) ** 2
    sims = [hermite_sim(gpu, s, B.SOFT, block_units=u) for u in (16, 1280)]
    try:
        for sim in sims:
            sim.compute_acc_jerk()
        idx, r2 = sims[0].nearest()
        assert_candidates(idx, r2, np.stack([s[k] for k in Q]), soft2, what="starting evaluation")
        assert idx[0] == 1 and idx[1] == 0
        partial, before = 0, None      # a snapshot needs ticks and levels: they exist behind the first call
        for step in range(24):
            outs = [sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=1) for sim in sims]
            assert outs[0] == outs[1]
            snaps = [snapshot(sim) for sim in sims]
            for k in ("q", "v", "a", "j"):
                assert np.array_equal(bits(snaps[0][k]), bits(snaps[1][k])), f"step {step}: {k} differs between the unit counts"
            assert np.array_equal(snaps[0]["nn"][0], snaps[1]["nn"][0]) and np.array_equal(bits(snaps[0]["nn"][1]), bits(snaps[1]["nn"][1]))
            now = snaps[0]
            if before is not None:
                t_next, act = B.next_time(before["ticks"], before["levels"], kmax)
                qp, _ = B.predict_all(before["q"], before["v"], before["a"], before["j"], before["ticks"], t_next, dt_max, kmax)
                assert act.sum() == outs[0]["max_active"]
                partial += int(act.sum() < 256)
                assert_candidates(now["nn"][0], now["nn"][1], H._r32(qp), soft2, rows=np.flatnonzero(act), what=f"step {step}")
                assert np.array_equal(now["nn"][0][~act], before["nn"][0][~act]), f"step {step}: an inactive body's index changed"
                assert np.array_equal(bits(now["nn"][1][~act]), bits(before["nn"][1][~act])), f"step {step}: an inactive body's r2 changed"
            before = now
        assert partial >= 10, "the replay saw too few partial active sets"
    finally:
        for sim in sims:
            sim.close()


# ------------------------------------------------------------------------------------------------------------ 4. encounter stops
@lru_cache(maxsize=None)
def cluster_at_apocentre(n=256):
    """cluster(n) with its binary moved to apocentre (separation a (1 + e) = 1.9e11 m): it then falls towards pericentre."""
    s, period = B.cluster(n)
    s = {k: v.copy() for k, v in s.items()}
    e, a, m = 0.9, 1e11, 1e30
    mu = float(H.G) * 2.0 * m
    r = a * (1.0 + e)
    vrel = np.sqrt(mu * (1.0 - e) / r)
    s["qx"][:2] = (-r / 2, r / 2)
    s["vy"][:2] = (-vrel / 2, vrel / 2)
    return s, period


def full_state(sim):
    st = sim.state()
    return np.stack([st[k] for k in Q + V] + list(sim.acc()) + list(sim.jerk()))


def test_encounter_stop_shared_steps(gpu):
    s, period = cluster_at_apocentre()
    thr = N.threshold(RADIUS, np.float32(B.SOFT) ** 2)
    runs = {}
    for batch in (1, 64):
        with hermite_sim(gpu, s, B.SOFT, evolve_batch=batch) as sim:
            sim.set_encounter(RADIUS)
            out = sim.evolve(period, eta=ETA, eta_start=ETA_START)
            enc = sim.encounters()
            idx, r2 = sim.nearest()
            runs[batch] = (out, enc, full_state(sim), idx, r2)
            assert sim.info("encounter_count") == enc["count"]
    out, enc, state, idx, r2 = runs[1]
    print(f"stopped after {out['steps']} steps at t = {out['time']:.6e} s of {period:.6e}; pairs {list(zip(enc['i'], enc['j']))}")
    assert 1 < out["steps"] and out["time"] < period
    assert enc["count"] == 2 and list(enc["i"]) == [0, 1] and list(enc["j"]) == [1, 0]
    assert enc["time"] == out["time"] and (enc["r2"] <= thr).all()
    assert np.array_equal(bits(enc["r2"]), bits(r2[:2])) and r2.min() <= thr
    out64, enc64, state64, idx64, r264 = runs[64]
    assert out64 == out and np.array_equal(bits(state64), bits(state)) and np.array_equal(idx64, idx)
    assert np.array_equal(bits(r264), bits(r2)) and enc64["count"] == 2 and enc64["time"] == enc["time"]
    for k in ("i", "j"):
        assert np.array_equal(enc64[k], enc[k])
    assert np.array_equal(bits(enc64["r2"]), bits(enc["r2"]))
    # the same upload without a radius: one step earlier nobody is that close, at the stopping step somebody is
    with hermite_sim(gpu, s, B.SOFT) as sim:
        early = sim.evolve(period, eta=ETA, eta_start=ETA_START, max_steps=out["steps"] - 1)
        r2_early = sim.nearest()[1]
        assert sim.encounters()["count"] == 0
    with hermite_sim(gpu, s, B.SOFT) as sim:
        same = sim.evolve(period, eta=ETA, eta_start=ETA_START, max_steps=out["steps"])
        r2_same = sim.nearest()[1]
        assert np.array_equal(bits(full_state(sim)), bits(state))
    print(f"smallest r2 one step earlier {r2_early.min():.6e}, at the stop {r2_same.min():.6e}, threshold {thr:.6e}")
    assert early["steps"] == out["steps"] - 1 and r2_early.min() > thr
    assert same["steps"] == out["steps"] and same["time"] == out["time"] and r2_same.min() <= thr


def test_encounter_stop_block_steps(gpu):
    s, period = cluster_at_apocentre()
    dt_max, kmax = float(np.float32(period)), 12
    thr = N.threshold(RADIUS, np.float32(B.SOFT) ** 2)
    with hermite_sim(gpu, s, B.SOFT) as sim:
        sim.set_encounter(RADIUS)
        out = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        enc = sim.encounters()
        idx, r2 = sim.nearest()
        print(f"stopped after {out['steps']} block steps at t = {out['time']:.6e} s of {dt_max:.6e}; pairs {list(zip(enc['i'], enc['j']))}")
        assert not out["synchronised"] and 0.0 < out["time"] < dt_max and out["steps"] > 1
        assert enc["count"] >= 1 and set(enc["i"]) <= {0, 1} and enc["time"] == out["time"]
        assert all(idx[i] == j for i, j in zip(enc["i"], enc["j"])) and (enc["r2"] <= thr).all()
        assert np.array_equal(bits(enc["r2"]), bits(r2[enc["i"]]))
        assert code_of(gpu, sim.energy) == E_STATE      # the block is open
        assert code_of(gpu, lambda: sim.set_option("nearest", 0)) == E_STATE
        sim.set_encounter(0.0)
        rest = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        assert rest["synchronised"] and sim.encounters()["count"] == 0
        end = full_state(sim)
        end_nn = sim.nearest()
        steps = out["steps"] + rest["steps"]
    with hermite_sim(gpu, s, B.SOFT) as sim:      # never had a radius
        whole = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        assert whole["synchronised"] and whole["steps"] == steps
        assert np.array_equal(bits(full_state(sim)), bits(end))
        assert np.array_equal(sim.nearest()[0], end_nn[0]) and np.array_equal(bits(sim.nearest()[1]), bits(end_nn[1]))
    # the step before the stop had nobody that close among the bodies that took it: stopping one step earlier finds no hit
    with hermite_sim(gpu, s, B.SOFT) as sim:
        sim.set_encounter(RADIUS)
        early = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=out["steps"] - 1)
        assert early["steps"] == out["steps"] - 1 and sim.encounters()["count"] == 0


# ------------------------------------------------------------------------------------------------------------------ 5. state rules
def test_state_rules(gpu):
    s, soft = N.lattice(513)
    with gpu.Simulation(513, soft=soft) as sim:
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            assert code_of(gpu, lambda: sim.set_option("nearest", 1)) == E_STATE
        sim.set_option("integrator", 2)
        assert code_of(gpu, lambda: sim.set_option("nearest", 2)) == E_INVALID
        assert code_of(gpu, lambda: sim.set_option("nearest", -1)) == E_INVALID
        assert code_of(gpu, lambda: sim.set_encounter(1.0)) == E_STATE        # needs "nearest" 1
        sim.set_encounter(0.0)
        for bad in (-1.0, float("inf"), float("nan")):
            assert code_of(gpu, lambda: sim.set_encounter(bad)) == E_INVALID
        assert sim.info("nearest") == 0 and sim.info("encounter_count") == 0
        bytes0 = sim.info("device_bytes")
        sim.set_option("nearest", 1)
        assert sim.info("nearest") == 1
        assert code_of(gpu, lambda: sim.set_option("integrator", 0)) == E_STATE   # "nearest" belongs to the Hermite sweeps
        assert code_of(gpu, sim.nearest) == E_STATE                           # nothing uploaded
        sim.upload(s)
        assert code_of(gpu, sim.nearest) == E_STATE                           # no evaluation yet
        assert sim.encounters()["count"] == 0
        sim.compute_acc_jerk()
        idx, r2 = sim.nearest()
        assert sim.info("device_bytes") > bytes0                              # the buffers are counted
        idx_only = np.zeros(513, np.int32)
        import ctypes as C
        assert gpu.lib().murbhip_download_nearest(sim._h, idx_only.ctypes.data_as(C.POINTER(C.c_int)), None) == 0
        assert np.array_equal(idx_only, idx)
        sim.upload(s)
        assert code_of(gpu, sim.nearest) == E_STATE                           # the bodies changed
        sim.step(1.0)
        idx1, r21 = sim.nearest()                                             # a step keeps them
        assert (idx1 >= 0).all()
        sim.set_encounter(2.0)
        assert code_of(gpu, lambda: sim.set_option("nearest", 0)) == E_STATE  # a radius is set
        sim.step(1.0)                                                         # murbhip_step never stops
        sim.set_encounter(0.0)
        sim.set_option("nearest", 0)                                          # drops the remembered evaluation
        assert code_of(gpu, sim.nearest) == E_STATE and code_of(gpu, sim.jerk) == E_STATE
        sim.compute_acc_jerk()
        assert code_of(gpu, sim.nearest) == E_STATE
        sim.set_option("nearest", 1)
        assert code_of(gpu, sim.nearest) == E_STATE and code_of(gpu, sim.jerk) == E_STATE
        sim.compute_acc_jerk()
        assert (sim.nearest()[0] >= 0).all()
    with gpu.Simulation(4096, soft=np.float32(2e8), devices=[0, 0], exchange="copy") as two:     # two shards on one device
        assert code_of(gpu, lambda: two.set_option("nearest", 1)) == E_STATE


# ------------------------------------------------------------------------------------------------------------------------ 6. plugin
@pytest.mark.parametrize("integrator", [3, 4])
def test_plugin_matches_the_c_abi(gpu, integrator):
    """HostSim(integrator=3 / 4, encounter=R), one iteration, against the same calls through the C ABI on the same bodies: the
    same pairs, count and time.  R is the median nearest-neighbour distance of the start, so that about half of the bodies have
    met their neighbour when the first substep ends."""
    n, soft, dt = 1024, np.float32(2e8), np.float32(3600.0)
    s = gpu.init_bodies(n, "galaxy")
    with hermite_sim(gpu, s, soft) as sim:
        sim.compute_acc_jerk()
        radius = float(np.sqrt(np.median(sim.nearest()[1].astype(np.float64)) - float(soft) ** 2))
        sim.set_encounter(radius)
        if integrator == 3:
            out = sim.evolve(float(dt), eta=0.02, eta_start=0.01, dt_min=0.0, dt_max=float(dt), max_steps=1000000)
        else:
            out = sim.evolve_block(float(dt), blocks=1, eta=0.02, eta_start=0.01, kmax=12)
        want = sim.encounters()
    assert 0 < want["count"] <= n and want["time"] == out["time"]
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=integrator, encounter=radius) as host:
        host.step(1)
        got = host.encounters()
    assert got["count"] == want["count"] and got["time"] == want["time"]
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["j"], want["j"]) and np.array_equal(bits(got["r2"]), bits(want["r2"]))
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=2) as fixed:
        assert fixed.encounters() is None
    with pytest.raises(ValueError):
        gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=2, encounter=radius)


@pytest.mark.parametrize("im", ["hip+hermite+adaptive", "hip+hermite+block"])
def test_cli_stops_at_an_encounter(im):
    """--renc larger than the system: every body that takes the first substep has met its neighbour when it ends, so the first
    iteration prints one `encounter:` line per such body, sorted by body, and is the last; the final line is the usual one.
    Shared steps: all 600 bodies take it.  Block steps: only the active set of the first block step does (the bodies at the
    deepest starting level), and the run's own count of body-steps says how many those are."""
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    r = subprocess.run([exe, "-n", "600", "-i", "5", "--nv", "--im", im, "--renc", "1e30"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"^encounter: (\d+) (\d+) ([0-9.e+-]+) ([0-9.e+-]+)$", r.stdout, re.M)
    took = [int(x[0]) for x in lines]
    if im == "hip+hermite+block":
        m = re.search(r"Block steps: (\d+) block steps, (\d+) body-steps", r.stdout)
        assert m and int(m.group(1)) == 1 and 1 <= len(lines) == int(m.group(2)) <= 600, r.stdout[-2000:]
        assert took == sorted(set(took)) and took[-1] < 600
    else:
        assert took == list(range(600)), r.stdout[-2000:]
        assert re.search(r"Adaptive steps: 1 substeps", r.stdout), r.stdout[-500:]
    assert "last tracked iteration" not in r.stdout      # one iteration ran: the history has one row, no drift to report
    assert all(int(i) != int(j) and float(d) >= 0.0 and 0.0 < float(t) <= 3600.0 for i, j, d, t in lines)
    assert re.search(r"^Entire simulation took [0-9.e+-]+ ms \([0-9.e+-]+ FPS\)$", r.stdout, re.M), r.stdout[-500:]
    plain = subprocess.run([exe, "-n", "600", "-i", "2", "--nv", "--im", im], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "encounter:" not in plain.stdout
    bad = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", "hip+hermite", "--renc", "1.0"], capture_output=True, text=True,
                         timeout=60)
    assert bad.returncode != 0 and "--renc" in bad.stdout

"""GPU: contacts by radii from the Hermite sweeps (option "contact") and the contact stop of murbhip_evolve /
murbhip_evolve_block, through the C ABI, the plugin and murb-hip.

Yardstick: tests/helpers/contact_ref.py (numpy, written from include/murbhip.h, pinned by tests/test_contact_host.py): exact
arithmetic on a lattice with half-integer radii, where every gap2 is exact in fp32 and indices and bits must match; fp64
candidate sets elsewhere, with the bound 1e-6 (r2 + s^2): at most 6 fp32 roundings on the r2 side and 3 on the s^2 side, each
2^-24, stay below 4e-7 of r2 + s^2."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import contact_ref as CR           # noqa: E402
import hermite_block_ref as B      # noqa: E402
import hermite_ref as H            # noqa: E402
import nearest_ref as N            # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
Q, V = ("qx", "qy", "qz"), ("vx", "vy", "vz")
ETA, ETA_START = 0.02, 0.01


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def contact_sim(gpu, s, soft, radii=None, contact=1, **opts):
    sim = gpu.Simulation(len(s["qx"]), soft=soft)
    sim.set_option("integrator", 2)
    sim.set_option("contact", contact)
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.upload(s)
    if radii is not None:
        sim.upload_radii(radii)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def assert_candidates(idx, gap2, q, radii, soft2, rows=None, what=""):
    ok, err = CR.check_candidates(idx, gap2, q, radii, soft2, rows)
    print(f"{what}: largest gap2 error {err:.3e} of the bound 1e-6 (r2 + s^2)")
    assert ok, what + ": an index is not among the accepted contact partners"
    assert err <= 1.0, what


def full_state(sim):
    st = sim.state()
    return np.stack([st[k] for k in Q + V] + list(sim.acc()) + list(sim.jerk()))


# ------------------------------------------------------------------------------------------------------------- 1. exact lattice
@pytest.mark.parametrize("n", [1, 2, 513, 1024, 2049])
def test_exact_lattice(gpu, n):
    """Integer coordinates, half-integer radii, soft 0.5: (idx, gap2) equal the restatement bit for bit for "jsplit" 1, 3 and 8,
    and among the three; accelerations and jerks are those of "contact" 0, bit for bit."""
    s, soft, radii = CR.lattice(n)
    q = np.stack([s[k] for k in Q])
    want_idx, want_gap2 = CR.contact(q, radii, 0.25)
    if n >= 513:      # the lattice holds what it is meant to
        assert want_idx[30] == n - 1 and want_gap2[30] == -3.25 and want_gap2[20] == 0.0 and want_idx[20] == 21
        assert want_gap2[5] == -1.0 and want_gap2[7] == 0.75 and want_gap2[100] == 5.75
    for jsplit in (1, 3, 8):
        with contact_sim(gpu, s, soft, radii, contact=0, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            plain = (np.stack(sim.acc()), np.stack(sim.jerk()))
            assert code_of(gpu, sim.contact) == E_STATE
        with contact_sim(gpu, s, soft, radii, jsplit=jsplit) as sim:
            sim.compute_acc_jerk()
            idx, gap2 = sim.contact()
            a, j = np.stack(sim.acc()), np.stack(sim.jerk())
        assert np.array_equal(idx, want_idx), f"jsplit {jsplit}: indices differ at {np.flatnonzero(idx != want_idx)[:8]}"
        assert np.array_equal(bits(gap2), bits(want_gap2)), f"jsplit {jsplit}: gap2 differs at {np.flatnonzero(bits(gap2) != bits(want_gap2))[:8]}"
        assert np.array_equal(bits(a), bits(plain[0])) and np.array_equal(bits(j), bits(plain[1])), \
            f"jsplit {jsplit}: the forces changed with the option"
    if n > 1:      # gap2(i, j) == gap2(j, i) bit for bit: a body's partner has a partner at most as far
        assert (gap2[idx] <= gap2).all()


# --------------------------------------------------------------------------------------------------------------------- 2. galaxy
def test_galaxy_2049(gpu):
    """Galaxy bodies with radii drawn from [0, 3 x the median nearest-neighbour distance] (seed 1): most bodies touch another,
    and for most the partner is not the nearest body."""
    n, soft = 2049, np.float32(2e8)
    soft2 = float(soft) ** 2
    s = gpu.init_bodies(n, "galaxy")
    q = np.stack([s[k] for k in Q])
    nn_best, nn_cand = N.nearest(q, soft2)
    median = float(np.sqrt(np.median(nn_best) - soft2))
    radii = np.random.default_rng(1).uniform(0.0, 3.0 * median, n).astype(np.float32)
    g, best, _ = CR.candidates(q, radii, soft2)
    assert (best <= 0).sum() >= 100 and (~nn_cand[np.arange(n), g.argmin(1)]).sum() >= 100      # the restatement first
    with contact_sim(gpu, s, soft, radii) as sim:
        sim.compute_acc_jerk()
        idx, gap2 = sim.contact()
        sim.step(0.0)         # a step keeps the partners of its predicted end state: with dt = 0 that is the same state
        idx1, gap21 = sim.contact()
    assert_candidates(idx, gap2, q, radii, soft2, what="galaxy 2049")
    assert (gap2 <= 0).sum() >= 100 and (~nn_cand[np.arange(n), idx]).sum() >= 100
    assert (gap2[idx] <= gap2).all()
    assert np.array_equal(idx1, idx) and np.array_equal(bits(gap21), bits(gap2))


# --------------------------------------------------------------------------------------------------------- 3. block step replay
@lru_cache(maxsize=None)
def cluster(n):
    return B.cluster(n)


def cluster_radii(n=256):
    """The binary has none; the field bodies, 5.5e10 m and more from each other, up to 6e10 m: about 40 of them overlap."""
    r = np.random.default_rng(1).uniform(0.0, 6e10, n).astype(np.float32)
    r[:2] = 0.0
    return r


def snapshot(sim):
    st = sim.state()
    return {"q": np.stack([st[k] for k in Q]), "v": np.stack([st[k] for k in V]), "a": np.stack(sim.acc()),
            "j": np.stack(sim.jerk()), "ticks": sim.block_state()[0], "levels": sim.block_state()[1], "cp": sim.contact()}


def test_block_step_replay(gpu):
    """cluster(256), one block step per call: the active bodies' values are the restatement's at the predicted positions, the
    inactive bodies' (cp, gap2) do not change by a bit, and "block_units" 16 and 1280 give the same bits."""
    s, period = cluster(256)
    radii = cluster_radii()
    dt_max, kmax, soft2 = float(np.float32(period / 2.0)), 12, float(np.float32(B.SOFT)) ** 2
    sims = [contact_sim(gpu, s, B.SOFT, radii, block_units=u) for u in (16, 1280)]
    try:
        for sim in sims:
            sim.compute_acc_jerk()
        idx, gap2 = sims[0].contact()
        assert_candidates(idx, gap2, np.stack([s[k] for k in Q]), radii, soft2, what="starting evaluation")
        assert (gap2[2:] <= 0).sum() >= 10, "no field bodies overlap"
        partial, before = 0, None      # a snapshot needs ticks and levels: they exist behind the first call
        for step in range(24):
            outs = [sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=1) for sim in sims]
            assert outs[0] == outs[1]
            snaps = [snapshot(sim) for sim in sims]
            for k in ("q", "v", "a", "j"):
                assert np.array_equal(bits(snaps[0][k]), bits(snaps[1][k])), f"step {step}: {k} differs between the unit counts"
            assert np.array_equal(snaps[0]["cp"][0], snaps[1]["cp"][0]) and np.array_equal(bits(snaps[0]["cp"][1]), bits(snaps[1]["cp"][1]))
            now = snaps[0]
            if before is not None:
                t_next, act = B.next_time(before["ticks"], before["levels"], kmax)
                qp, _ = B.predict_all(before["q"], before["v"], before["a"], before["j"], before["ticks"], t_next, dt_max, kmax)
                assert act.sum() == outs[0]["max_active"]
                partial += int(act.sum() < 256)
                assert_candidates(now["cp"][0], now["cp"][1], H._r32(qp), radii, soft2, rows=np.flatnonzero(act), what=f"step {step}")
                assert np.array_equal(now["cp"][0][~act], before["cp"][0][~act]), f"step {step}: an inactive body's partner changed"
                assert np.array_equal(bits(now["cp"][1][~act]), bits(before["cp"][1][~act])), f"step {step}: an inactive body's gap2 changed"
            before = now
        assert partial >= 10, "the replay saw too few partial active sets"
    finally:
        for sim in sims:
            sim.close()


# -------------------------------------------------------------------------------------------------------------- 4. contact stops
@lru_cache(maxsize=None)
def cluster_at_apocentre(n=256):
    """cluster(n) with its binary moved to apocentre (separation a (1 + e) = 1.9e11 m): it then falls towards pericentre
    (1e10 m).  With R[0] = 2e10 and R[1] = 1e10 the two touch at 3e10 m; nobody else has a radius."""
    s, period = B.cluster(n)
    s = {k: v.copy() for k, v in s.items()}
    e, a, m = 0.9, 1e11, 1e30
    mu = float(H.G) * 2.0 * m
    r = a * (1.0 + e)
    vrel = np.sqrt(mu * (1.0 - e) / r)
    s["qx"][:2] = (-r / 2, r / 2)
    s["vy"][:2] = (-vrel / 2, vrel / 2)
    radii = np.zeros(n, np.float32)
    radii[0], radii[1] = 2e10, 1e10
    return s, period, radii


def test_contact_stop_shared_steps(gpu):
    s, period, radii = cluster_at_apocentre()
    runs = {}
    for batch in (1, 64):
        with contact_sim(gpu, s, B.SOFT, radii, contact=2, evolve_batch=batch) as sim:
            out = sim.evolve(period, eta=ETA, eta_start=ETA_START)
            hit = sim.contacts()
            idx, gap2 = sim.contact()
            runs[batch] = (out, hit, full_state(sim), idx, gap2)
            assert sim.info("contact_count") == hit["count"] and sim.info("contact") == 2
            assert sim.encounters()["count"] == 0
    out, hit, state, idx, gap2 = runs[1]
    print(f"stopped after {out['steps']} steps at t = {out['time']:.6e} s of {period:.6e}; pairs {list(zip(hit['i'], hit['j']))}")
    assert 1 < out["steps"] and out["time"] < period
    assert hit["count"] == 2 and list(hit["i"]) == [0, 1] and list(hit["j"]) == [1, 0]
    assert hit["time"] == out["time"] and (hit["gap2"] <= 0).all()
    assert np.array_equal(bits(hit["gap2"]), bits(gap2[:2])) and gap2.min() <= 0
    out64, hit64, state64, idx64, gap264 = runs[64]
    assert out64 == out and np.array_equal(bits(state64), bits(state)) and np.array_equal(idx64, idx)
    assert np.array_equal(bits(gap264), bits(gap2)) and hit64["count"] == 2 and hit64["time"] == hit["time"]
    for k in ("i", "j"):
        assert np.array_equal(hit64[k], hit[k])
    assert np.array_equal(bits(hit64["gap2"]), bits(hit["gap2"]))
    # the same upload with "contact" 1: one step earlier nobody touches, at the stopping step somebody does
    with contact_sim(gpu, s, B.SOFT, radii) as sim:
        early = sim.evolve(period, eta=ETA, eta_start=ETA_START, max_steps=out["steps"] - 1)
        gap2_early = sim.contact()[1]
        assert sim.contacts()["count"] == 0
    with contact_sim(gpu, s, B.SOFT, radii) as sim:
        same = sim.evolve(period, eta=ETA, eta_start=ETA_START, max_steps=out["steps"])
        gap2_same = sim.contact()[1]
        assert np.array_equal(bits(full_state(sim)), bits(state)) and sim.contacts()["count"] == 0
    print(f"smallest gap2 one step earlier {gap2_early.min():.6e}, at the stop {gap2_same.min():.6e}")
    assert early["steps"] == out["steps"] - 1 and gap2_early.min() > 0
    assert same["steps"] == out["steps"] and same["time"] == out["time"] and gap2_same.min() <= 0


def test_contact_stop_block_steps(gpu):
    s, period, radii = cluster_at_apocentre()
    dt_max, kmax = float(np.float32(period)), 12
    with contact_sim(gpu, s, B.SOFT, radii, contact=2) as sim:
        out = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        hit = sim.contacts()
        idx, gap2 = sim.contact()
        print(f"stopped after {out['steps']} block steps at t = {out['time']:.6e} s of {dt_max:.6e}; pairs {list(zip(hit['i'], hit['j']))}")
        assert not out["synchronised"] and 0.0 < out["time"] < dt_max and out["steps"] > 1
        assert hit["count"] >= 1 and set(hit["i"]) <= {0, 1} and hit["time"] == out["time"]
        assert all(idx[i] == j for i, j in zip(hit["i"], hit["j"])) and (hit["gap2"] <= 0).all()
        assert np.array_equal(bits(hit["gap2"]), bits(gap2[hit["i"]]))
        assert code_of(gpu, sim.energy) == E_STATE      # the block is open
        assert code_of(gpu, lambda: sim.set_option("contact", 0)) == E_STATE      # the option is locked
        assert code_of(gpu, lambda: sim.upload_radii(radii)) == E_STATE
        sim.set_option("contact", 1)                    # only the stop goes: the block stays open
        rest = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        assert rest["synchronised"] and sim.contacts()["count"] == 0
        end = full_state(sim)
        end_cp = sim.contact()
        steps = out["steps"] + rest["steps"]
    with contact_sim(gpu, s, B.SOFT, radii) as sim:      # never stopped
        whole = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax)
        assert whole["synchronised"] and whole["steps"] == steps
        assert np.array_equal(bits(full_state(sim)), bits(end))
        assert np.array_equal(sim.contact()[0], end_cp[0]) and np.array_equal(bits(sim.contact()[1]), bits(end_cp[1]))
    # the step before the stop had nobody touching among the bodies that took it: stopping one step earlier finds no hit
    with contact_sim(gpu, s, B.SOFT, radii, contact=2) as sim:
        early = sim.evolve_block(dt_max, eta=ETA, eta_start=ETA_START, kmax=kmax, max_steps=out["steps"] - 1)
        assert early["steps"] == out["steps"] - 1 and sim.contacts()["count"] == 0


# ------------------------------------------------------------------------------------------------------------------ 6. state rules
def test_state_rules(gpu):
    s, soft, radii = CR.lattice(513)
    fp = C.POINTER(C.c_float)
    with gpu.Simulation(513, soft=soft) as sim:
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            assert code_of(gpu, lambda: sim.set_option("contact", 1)) == E_STATE
        sim.set_option("integrator", 2)
        assert code_of(gpu, lambda: sim.set_option("contact", 3)) == E_INVALID
        assert code_of(gpu, lambda: sim.set_option("contact", -1)) == E_INVALID
        assert sim.info("contact") == 0 and sim.info("contact_count") == 0
        assert gpu.lib().murbhip_upload_radii(sim._h, None) == E_INVALID
        for bad in (-1.0, float("inf"), float("nan")):
            wrong = radii.copy()
            wrong[100] = bad
            assert code_of(gpu, lambda: sim.upload_radii(wrong)) == E_INVALID
        bytes0 = sim.info("device_bytes")
        sim.set_option("contact", 1)
        assert sim.info("contact") == 1
        assert code_of(gpu, lambda: sim.set_option("integrator", 0)) == E_STATE   # "contact" belongs to the Hermite sweeps
        assert code_of(gpu, lambda: sim.set_option("nearest", 1)) == E_STATE      # they exclude each other
        assert code_of(gpu, sim.contact) == E_STATE                           # nothing uploaded
        sim.upload(s)
        assert code_of(gpu, sim.contact) == E_STATE                           # no evaluation yet
        assert code_of(gpu, lambda: sim.masses(with_radii=True)) == E_STATE   # no radii were ever set
        assert sim.contacts()["count"] == 0
        sim.compute_acc_jerk()
        idx0, gap20 = sim.contact()                                           # radii are 0 until first set: the nearest body
        nn_idx, nn_r2 = N.nearest(np.stack([s[k] for k in Q]), 0.25, exact=True)
        assert np.array_equal(idx0, nn_idx) and np.array_equal(bits(gap20), bits(nn_r2 - np.float32(0.25)))
        sim.upload_radii(radii)
        assert code_of(gpu, sim.contact) == E_STATE and code_of(gpu, sim.jerk) == E_STATE   # the evaluation was dropped
        assert np.array_equal(sim.masses(with_radii=True)[1], radii)
        sim.compute_acc_jerk()
        idx, gap2 = sim.contact()
        want_idx, want_gap2 = CR.contact(np.stack([s[k] for k in Q]), radii, 0.25)
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(gap2), bits(want_gap2))
        assert sim.info("device_bytes") > bytes0                              # the buffers are counted
        idx_only = np.zeros(513, np.int32)
        assert gpu.lib().murbhip_download_contact(sim._h, idx_only.ctypes.data_as(C.POINTER(C.c_int)), None) == 0
        assert np.array_equal(idx_only, idx)
        gap2_only = np.zeros(513, np.float32)
        assert gpu.lib().murbhip_download_contact(sim._h, None, gap2_only.ctypes.data_as(fp)) == 0
        assert np.array_equal(bits(gap2_only), bits(gap2))
        sim.upload(s)                                                         # radii survive an upload
        assert code_of(gpu, sim.contact) == E_STATE                           # the bodies changed
        assert np.array_equal(sim.masses(with_radii=True)[1], radii)
        sim.step(0.0)                                                         # a step keeps them, at its predicted end state: dt = 0, the same state
        idx1, gap21 = sim.contact()
        assert np.array_equal(idx1, want_idx) and np.array_equal(bits(gap21), bits(want_gap2))
        sim.step(1.0)                                                         # (the lattice's masses throw the bodies far apart in a second)
        assert (sim.contact()[0] >= 0).all()
        sim.upload(s)
        sim.compute_acc_jerk()
        sim.set_option("contact", 2)                                          # 1 <-> 2 keeps the evaluation
        assert np.array_equal(sim.contact()[0], want_idx) and np.array_equal(bits(sim.contact()[1]), bits(want_gap2))
        sim.step(1.0)
        sim.set_option("contact", 1)
        sim.contact()
        sim.set_option("contact", 0)                                          # drops the remembered evaluation
        assert code_of(gpu, sim.contact) == E_STATE and code_of(gpu, sim.jerk) == E_STATE
        sim.set_option("nearest", 1)
        assert code_of(gpu, lambda: sim.set_option("contact", 1)) == E_STATE  # ... in both directions
        sim.upload(s)
        sim.compute_acc_jerk()                                                # the lanes are 0 again: the nearest bodies
        assert np.array_equal(sim.nearest()[0], nn_idx) and np.array_equal(bits(sim.nearest()[1]), bits(nn_r2))
        sim.set_option("nearest", 0)
        sim.set_option("contact", 1)
        sim.init_bodies("galaxy")                                             # replaces the radii with the scheme's
        scheme_r = gpu.init_bodies(513, "galaxy")["r"]
        assert np.array_equal(sim.masses(with_radii=True)[1], scheme_r)
        sim.compute_acc_jerk()
        st = sim.state()
        assert_candidates(*sim.contact(), np.stack([st[k] for k in Q]), scheme_r, float(soft) ** 2, what="scheme radii")
    with gpu.Simulation(4096, soft=np.float32(2e8), devices=[0, 0], exchange="copy") as two:     # two shards on one device
        assert code_of(gpu, lambda: two.set_option("contact", 1)) == E_STATE
        assert code_of(gpu, lambda: two.upload_radii(np.zeros(4096, np.float32))) == E_STATE


# ------------------------------------------------------------------------------------------------------------------------ 7. plugin
@pytest.mark.parametrize("integrator", [3, 4])
def test_plugin_matches_the_c_abi(gpu, integrator):
    """HostSim(integrator=3 / 4, contact=True, rscale=f), one iteration, against the same calls through the C ABI on the same
    bodies: the same pairs, count and time.  f is the median over the bodies of distance / (R_i + R_cp) at the start with the
    scheme's own radii, so that about half of the bodies touch their partner."""
    n, soft, dt = 1024, np.float32(2e8), np.float32(3600.0)
    s = gpu.init_bodies(n, "galaxy")
    with contact_sim(gpu, s, soft, s["r"]) as sim:
        sim.compute_acc_jerk()
        idx, gap2 = sim.contact()
        ssum = s["r"].astype(np.float64) + s["r"][idx].astype(np.float64)
        rscale = float(np.float32(np.median(np.sqrt(gap2.astype(np.float64) + ssum ** 2) / ssum)))
        sim.upload_radii((s["r"] * np.float32(rscale)).astype(np.float32))
        sim.set_option("contact", 2)
        if integrator == 3:
            out = sim.evolve(float(dt), eta=0.02, eta_start=0.01, dt_min=0.0, dt_max=float(dt), max_steps=1000000)
        else:
            out = sim.evolve_block(float(dt), blocks=1, eta=0.02, eta_start=0.01, kmax=12)
        want = sim.contacts()
    print(f"rscale {rscale:.4e}: {want['count']} bodies touch")
    assert 0 < want["count"] <= n and want["time"] == out["time"]
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=integrator, contact=True, rscale=rscale) as host:
        host.step(1)
        got = host.contacts()
        assert host.encounters()["count"] == 0
    assert got["count"] == want["count"] and got["time"] == want["time"]
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["j"], want["j"]) and np.array_equal(bits(got["gap2"]), bits(want["gap2"]))
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=integrator) as plain:
        assert plain.contacts() is None
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=2) as fixed:
        assert fixed.contacts() is None
    with pytest.raises(ValueError):
        gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=2, contact=True)
    with pytest.raises(ValueError):
        gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=integrator, contact=True, encounter=1e9)


# --------------------------------------------------------------------------------------------------------------------------- 8. CLI
@pytest.mark.parametrize("im", ["hip+hermite+adaptive", "hip+hermite+block"])
def test_cli_stops_at_a_contact(im):
    """--collide --rscale 1000: the galaxy's largest radii, 1.25e9 m, then exceed the 4e8 m system, so every body that takes
    the first substep touches another when it ends: the first iteration prints one `contact:` line per such body, sorted by
    body, and is the last.  Shared steps: all 600 bodies take it.  Block steps: only the first active set does, and the run's
    own count of body-steps says how many those are."""
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    r = subprocess.run([exe, "-n", "600", "-i", "5", "--nv", "--im", im, "--collide", "--rscale", "1000"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = re.findall(r"^contact: (\d+) (\d+) ([0-9.e+-]+) ([0-9.e+-]+)$", r.stdout, re.M)
    took = [int(x[0]) for x in lines]
    if im == "hip+hermite+block":
        m = re.search(r"Block steps: (\d+) block steps, (\d+) body-steps", r.stdout)
        assert m and int(m.group(1)) == 1 and 1 <= len(lines) == int(m.group(2)) <= 600, r.stdout[-2000:]
        assert took == sorted(set(took)) and took[-1] < 600
    else:
        assert took == list(range(600)), r.stdout[-2000:]
        assert re.search(r"Adaptive steps: 1 substeps", r.stdout), r.stdout[-500:]
    assert "last tracked iteration" not in r.stdout      # one iteration ran: the history has one row, no drift to report
    assert all(int(i) != int(j) and float(g) <= 0.0 and 0.0 < float(t) <= 3600.0 for i, j, g, t in lines)
    assert re.search(r"^Entire simulation took [0-9.e+-]+ ms \([0-9.e+-]+ FPS\)$", r.stdout, re.M), r.stdout[-500:]
    plain = subprocess.run([exe, "-n", "600", "-i", "2", "--nv", "--im", im], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "contact:" not in plain.stdout
    bad = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", "hip+hermite", "--collide"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--collide" in bad.stdout
    both = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", im, "--collide", "--renc", "1e9"], capture_output=True, text=True,
                          timeout=60)
    assert both.returncode != 0 and "--collide" in both.stdout
    scale = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", im, "--collide", "--rscale", "-2"], capture_output=True, text=True,
                           timeout=60)
    assert scale.returncode != 0 and "--rscale" in scale.stdout

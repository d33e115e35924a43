"""MI355X: the potential read-out and the bound members (include/murbbound.h) through the C ABI, the Python interface and the
plugin.  The field rule and the zero-mass rule bit for bit, the fp64 bound, unbinding one round at a time against
tests/helpers/bound_ref.py, the whole call against chained rounds, the summary, small systems, the calls as observers, and the
refused calls."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import bound_ref as R         # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
TOL_F64_MAX = R.TOL_F64_MAX       # tests/test_gpu_parity.py, forces
Q, V = R.Q, R.V
_fp, _ip, _dp, _bp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)


def make_sim(gpu, s, soft=R.SOFT, g=R.G, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft, g=g)
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
    return x.view({1: np.uint8, 4: np.int32, 8: np.int64}[x.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def same_run(a, b):
    """Two bound_members results: member, e and V bit for bit, and the summary."""
    keys = [k for k in a if k not in ("member", "e", "v", "centre")]
    return same(a["member"], b["member"]) and same(a["e"], b["e"]) and same(a["v"], b["v"]) and same(a["centre"], b["centre"]) and \
        all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in keys)


@lru_cache(maxsize=None)
def sphere(n, seed=1):
    """A Plummer sphere of n bodies (bound_ref.plummer), fp32.  Do not modify."""
    q, v, m = R.plummer(n, np.random.default_rng(seed))
    return R._state(q, v, m)


def within_tolerance(phi, want, what):
    err = np.abs(phi.astype(np.float64) - want) / np.where(want > 0, want, 1.0)
    print(f"{what}: largest |phi - fp64| / phi = {err.max():.3e} (bound {TOL_F64_MAX:.0e})")
    assert err.max() <= TOL_F64_MAX, what


def formula_e(s, v, phi):
    """The header's e from the fp32 phi and V, one fp64 operation at a time (numpy contracts nothing)."""
    w = [s[k].astype(np.float64) - v[c] for c, k in enumerate(V)]
    return 0.5 * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) - phi.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ 1. field rule
def test_field_rule_2049_every_chunk_count(gpu):
    """n = 2049 (five tiles, one body in the last), "field_chunks" 1 .. 5, "field_batch" 512 (five launches, the last a group of
    one point): murbpot_of equals murbfield_of's phi bit for bit for every body, and murbpot_at equals murbfield_at's for points
    with skip entries -1, 0, 511, 512, 2048: on the bodies they skip, and one that does not sit on the body it skips.  Every
    value is within TOL_F64_MAX of fp64."""
    n = 2049
    s = sphere(n)
    skip = np.array([-1, 0, 511, 512, 2048, 512, 0, 2048], np.int32)
    on = np.array([7, 0, 511, 512, 2048], np.int32)
    p = np.stack([np.concatenate([s[c][on], np.float32([0.3, -0.2, 0.1])]) for c in Q])      # the last three sit on no body
    want_of = R.potential(s)
    want_at = R.potential(s, points=p, skip=skip)
    everyone = np.arange(n, dtype=np.int32)
    for chunks in range(1, 6):
        with make_sim(gpu, s, field_chunks=chunks, field_batch=512) as sim:
            assert gpu.field_layout(n, chunks, 512, n)["batches"] == 5
            got, field = sim.potential_of(), sim.field_of(everyone)["phi"]
            assert same(got, field), (chunks, np.nonzero(bits(got) != bits(field))[0][:5])
            assert same(sim.potential_of(on), field[on])
            got_at, field_at = sim.potential_at(p, skip), sim.field_at(p, skip=skip)["phi"]
            assert same(got_at, field_at), (chunks, got_at, field_at)
            assert same(sim.potential_at(p), sim.field_at(p)["phi"]), "no skip entries at all"
        within_tolerance(got, want_of, f"n=2049 chunks={chunks} of")
        within_tolerance(got_at, want_at, f"n=2049 chunks={chunks} at")


@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 511, 512, 513))
def test_field_rule_small_n(gpu, n):
    s = sphere(n, seed=n)
    p = np.float32([[0.1, 0.0], [0.2, 0.0], [-0.3, 0.0]])
    p[:, 1] = [s[c][n - 1] for c in Q]
    skip = np.array([-1, n - 1], np.int32)
    with make_sim(gpu, s) as sim:
        got, field = sim.potential_of(), sim.field_of(np.arange(n, dtype=np.int32))["phi"]
        got_at, field_at = sim.potential_at(p, skip), sim.field_at(p, skip=skip)["phi"]
    assert same(got, field) and same(got_at, field_at), n
    within_tolerance(got, R.potential(s), f"n={n} of")
    within_tolerance(got_at, R.potential(s, points=p, skip=skip), f"n={n} at")
    if n == 1:
        assert bits(got).tolist() == [0], "a lone body: +0"


# -------------------------------------------------------------------------------------------------------------- 2. zero-mass rule
def test_zero_mass_rule(gpu):
    """Fixture A under a random mask against a second context of the same n whose bodies outside the mask were uploaded with
    mass 0: bit for bit, for bodies and for points with skip entries.  The all-zero mask gives +0 everywhere.  Under the mask
    the values are within TOL_F64_MAX of the masked fp64 sum."""
    s = R.fixture_a()
    n = len(s["m"])
    rng = np.random.default_rng(21)
    mask = rng.uniform(size=n) < 0.6
    mask[[0, 511, 512, n - 1]] = [True, False, True, False]
    skip = np.array([-1, 0, 511, 512, n - 1, 3], np.int32)
    p = np.stack([np.concatenate([s[c][[9, 0, 511, 512, n - 1]], np.float32([0.25])]) for c in Q])
    zeroed = dict(s, m=np.where(mask, s["m"], np.float32(0)))
    for chunks in (1, 3):
        with make_sim(gpu, s, field_chunks=chunks) as sim, make_sim(gpu, zeroed, field_chunks=chunks) as other:
            got, got_at = sim.potential_of(member=mask), sim.potential_at(p, skip, member=mask)
            assert same(got, other.potential_of()) and same(got_at, other.potential_at(p, skip)), chunks
            assert same(got, other.field_of(np.arange(n, dtype=np.int32))["phi"])
            some = np.array([n - 1, 5, 5, 512], np.int32)
            assert same(sim.potential_of(some, member=mask), got[some]), "a listed body need not be a member; twice is allowed"
            assert same(sim.potential_of(member=np.ones(n, bool)), sim.potential_of()), "the all-ones mask is no mask"
            nothing = sim.potential_of(member=np.zeros(n, bool))
            assert not bits(nothing).any() and not bits(sim.potential_at(p, skip, member=np.zeros(n, bool))).any(), "+0 everywhere"
            assert same(sim.potential_of(member=mask.astype(np.uint8) * 7), got), "any nonzero byte"
    within_tolerance(got, R.potential(s, member=mask), "fixture A, masked, of")
    within_tolerance(got_at, R.potential(s, member=mask, points=p, skip=skip), "fixture A, masked, at")


# ---------------------------------------------------------------------------------------------------------- 3. one round at a time
def chain(sim, s, start=None, limit=16):
    """bound_members with max_iter = 1, each call started from the call before's member: the list of results."""
    out, member = [], start
    for _ in range(limit):
        out.append(sim.bound_members(start=member, max_iter=1))
        member = out[-1]["member"]
        if out[-1]["converged"]:
            return out
    raise AssertionError("the chain did not converge")


@pytest.mark.parametrize("name", ("A", "B"))
def test_one_round_at_a_time(gpu, name):
    """Each round's set equals the reference round from the same start, bodies with reference |e| <= 2 * TOL_F64_MAX * phi left
    out (at most 2 a round; tests/test_bound_host.py asserts that the reference has none on these seeds).  The returned e is
    within TOL_F64_MAX * phi of the reference's evaluation against the returned set."""
    s = {"A": R.fixture_a, "B": R.fixture_b}[name]()
    n = len(s["m"])
    with make_sim(gpu, s) as sim:
        rounds = chain(sim, s)
    member = np.ones(n, bool)
    for t, got in enumerate(rounds):
        want, e, _, phi = R.one_round(s, member)
        band = R.in_band(e, phi)
        print(f"{name} round {t}: dropped {int(member.sum() - got['member'].sum())}, in the band {int(band.sum())}")
        assert band.sum() <= 2
        assert np.array_equal(got["member"][~band], want[~band]), (t, np.nonzero(got["member"] != want)[0][:8])
        assert not (got["member"] & ~member).any(), "bodies only ever leave"
        assert got["rounds"] == 1 and got["converged"] == (got["removed"] == 0) and got["removed"] == int(member.sum() - got["member"].sum())
        final_phi = R.potential(s, member=got["member"])
        final_e = R.energy(s, R.frame(s, got["member"]), final_phi)
        assert (np.abs(got["e"] - final_e) <= TOL_F64_MAX * final_phi + 1e-12).all(), t
        member = got["member"]
    assert len(rounds) >= 3 and rounds[-1]["removed"] == 0 and same(rounds[-1]["member"], rounds[-2]["member"])
    if name == "A":
        assert not member[R.A_SPHERE:].any() and member[:R.A_FAST].sum() <= 10, "the clump and the fast bodies leave"


# ------------------------------------------------------------------------------------------------------------------ 4. whole call
@pytest.mark.parametrize("name", ("A", "B"))
def test_whole_call(gpu, name):
    """One call with max_iter = K equals K chained single rounds bit for bit (member, e, V), for K too small to converge and for
    the whole run; converged and rounds say which.  e equals the header's formula recomputed in numpy from potential_of(member
    = S) and the returned V, exactly.  V, the centre, K and W are within 1e-12 relative of numpy's sums."""
    s = {"A": R.fixture_a, "B": R.fixture_b}[name]()
    n = len(s["m"])
    m64 = s["m"].astype(np.float64)
    with make_sim(gpu, s) as sim:
        rounds = chain(sim, s)
        whole = sim.bound_members()
        short = sim.bound_members(max_iter=2)
        exact = sim.bound_members(max_iter=len(rounds))
        for r in (whole, short):
            phi = sim.potential_of(member=r["member"])
            assert same(r["e"], formula_e(s, r["v"], phi)), "e is the formula of the fp32 phi and V"
            inside = r["member"]
            mass = m64[inside].sum()
            w2 = sum((s[k].astype(np.float64) - r["v"][c]) ** 2 for c, k in enumerate(V))
            want = {"mass": mass, "kinetic": (0.5 * m64 * w2)[inside].sum(),
                    "potential": -0.5 * (m64 * phi)[inside].sum()}
            for c, k in enumerate(V):
                want[k] = (m64 * s[k].astype(np.float64))[inside].sum() / mass
            for c, k in enumerate(("cx", "cy", "cz")):
                want[k] = (m64 * s[Q[c]].astype(np.float64))[inside].sum() / mass
            for k, x in want.items():
                assert abs(r[k] - x) <= 1e-12 * abs(x), (k, r[k], x)
            assert r["members"] == int(inside.sum()) and r["removed"] == n - r["members"]
            assert r["unbound_bodies"] == int((r["e"] >= 0).sum()) and abs(r["virial_ratio"] - r["kinetic"] / abs(r["potential"])) <= 1e-15
            assert (r["v"] == [r["vx"], r["vy"], r["vz"]]).all() and (r["centre"] == [r["cx"], r["cy"], r["cz"]]).all()
    assert len(rounds) >= 3
    assert whole["converged"] and whole["rounds"] == len(rounds) and same_run(whole, dict(rounds[-1], rounds=len(rounds), removed=whole["removed"]))
    assert same_run(exact, whole), "max_iter equal to the rounds needed: converged in the last one"
    assert not short["converged"] and short["rounds"] == 2
    second = rounds[1]
    assert same(short["member"], second["member"]) and same(short["e"], second["e"]) and same(short["v"], second["v"])
    assert whole["unbound_bodies"] <= n - whole["members"], "every member has e < 0; a body that left may have e < 0 against the final set"


# ------------------------------------------------------------------------------------------------------------- 5. start and frame
def test_start_and_frame_are_honoured(gpu):
    s = R.fixture_a()
    n = len(s["m"])
    with make_sim(gpu, s) as sim:
        clump = sim.bound_members(start=R.clump_mask())
        assert clump["members"] == R.A_CLUMP and np.array_equal(clump["member"], R.clump_mask()) and clump["converged"] and clump["rounds"] == 1
        assert np.abs(clump["v"] - [3.0, 0.0, 0.0]).max() < 0.1 and abs(clump["mass"] - 0.08) < 1e-6 and abs(clump["cx"] - 30.0) < 0.1
        assert clump["removed"] == 0
        want = R.unbind(s, start=R.clump_mask())
        assert (np.abs(clump["e"] - want["e"]) <= TOL_F64_MAX * want["phi"] + 1e-12).all(), "everyone's energy against the clump"
        rng = np.random.default_rng(4)
        start = rng.uniform(size=n) < 0.5
        part = sim.bound_members(start=start)
        assert not (part["member"] & ~start).any() and part["removed"] == int(start.sum()) - part["members"]
        assert np.array_equal(part["member"], R.unbind(s, start=start)["member"])
        assert same_run(part, sim.bound_members(start=start.astype(np.uint8) * 200)), "any nonzero byte"
        fixed = np.array([0.05, -0.02, 0.01])
        framed = sim.bound_members(frame_v=fixed)
        assert (framed["v"] == fixed).all() and framed["converged"]
        assert same(framed["e"], formula_e(s, fixed, sim.potential_of(member=framed["member"])))
        assert np.array_equal(framed["member"], R.unbind(s, frame_v=fixed)["member"])
        moving = sim.bound_members(frame_v=[3.0, 0.0, 0.0])      # the clump's frame, from all bodies: the sphere leaves
        assert moving["member"][R.A_SPHERE:].sum() >= 120 and moving["member"][:R.A_SPHERE].sum() == 0


# ------------------------------------------------------------------------------------------------------------ 6. small systems
def small(q, v, m):
    s = {"m": np.float32(m)}
    for keys, arr in ((Q, q), (V, v)):
        for c, k in enumerate(keys):
            s[k] = np.float32([row[c] for row in arr])
    return s


def test_small_systems(gpu):
    """n = 1: the lone body has e = 0 in its own frame and leaves, and the empty set converges (e then is 0.5 |v|^2, against
    nobody in the frame V = 0).  A bound pair is kept.  A fast receding pair is
    dropped in the first round and the empty set converges in the second, with NaN for the frame, the centre and the ratio.
    Massless members: a slow one near the pair stays and weighs nothing; a set of massless bodies alone has V = 0, phi = 0 and
    leaves."""
    with make_sim(gpu, small([[1, 2, 3]], [[4, 5, 6]], [1.0])) as sim:
        r = sim.bound_members()
        assert r["members"] == 0 and r["converged"] and r["rounds"] == 2 and r["removed"] == 1 and r["e"].tolist() == [38.5]
        assert r["unbound_bodies"] == 1 and np.isnan(r["v"]).all() and np.isnan(r["centre"]).all() and np.isnan(r["virial_ratio"])
    pair_q, pair_v = [[-0.5, 0, 0], [0.5, 0, 0]], [[0, -0.5, 0], [0, 0.5, 0]]
    with make_sim(gpu, small(pair_q, pair_v, [0.5, 0.5])) as sim:
        r = sim.bound_members()
        assert r["members"] == 2 and r["converged"] and r["rounds"] == 1 and r["mass"] == 1.0 and (r["v"] == 0).all() and (r["centre"] == 0).all()
        assert np.abs(r["e"] - (0.125 - 0.5 / np.sqrt(1.0 + 1e-4))).max() < 1e-6 and abs(r["virial_ratio"] - 0.5) < 1e-3
    with make_sim(gpu, small(pair_q, [[-10, 0, 0], [10, 0, 0]], [0.5, 0.5])) as sim:
        r = sim.bound_members()
        assert r["members"] == 0 and r["converged"] and r["rounds"] == 2 and r["removed"] == 2 and r["mass"] == 0.0
        assert np.isnan(r["v"]).all() and np.isnan(r["centre"]).all() and np.isnan(r["virial_ratio"]) and r["kinetic"] == 0.0
        assert (r["e"] == 50.0).all() and r["unbound_bodies"] == 2, "the final pass: against nobody, in the frame V = 0"
        r = sim.bound_members(max_iter=1)
        assert r["members"] == 0 and not r["converged"] and r["rounds"] == 1
    q = pair_q + [[0, 0.2, 0], [0, 40, 0]]
    with make_sim(gpu, small(q, pair_v + [[0.1, 0, 0], [0, 0, 0]], [0.5, 0.5, 0.0, 0.0])) as sim:
        r = sim.bound_members()
        assert r["member"].tolist() == [True, True, True, True] and r["mass"] == 1.0 and r["members"] == 4, "massless bodies in the well stay"
        assert (r["centre"] == 0).all()
        r = sim.bound_members(start=[0, 0, 1, 1])
        assert r["members"] == 0 and r["mass"] == 0.0 and r["e"][3] == 0.0 and r["e"][2] > 0, "massless bodies alone: phi = 0, V = 0"


# -------------------------------------------------------------------------------------------------------- 7. after steps, observers
def test_after_steps_and_evolve(gpu):
    """After steps under "integrator" 0 and 2, after evolve and after a synchronised evolve_block the call returns what a fresh
    context returns that was uploaded with the downloaded state, bit for bit.  Under "integrator" 1 in flight the device's
    velocities lag the positions by half a step and the download synchronises them, so there the result is checked against
    itself: it is a fixed point of one more round."""
    s = R.fixture_b()

    def fresh(st):
        with make_sim(gpu, dict(st, m=s["m"])) as other:
            return other.bound_members()
    with make_sim(gpu, s, integrator=2) as sim:
        sim.steps(2.0 ** -10, 3)
        assert same_run(sim.bound_members(), fresh(sim.state()))
        assert sim.evolve(2.0 ** -7, max_steps=8)["steps"] >= 1
        assert same_run(sim.bound_members(), fresh(sim.state()))
        assert sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)["synchronised"]
        assert same_run(sim.bound_members(), fresh(sim.state()))
    with make_sim(gpu, s) as sim:
        sim.steps(2.0 ** -10, 3)
        assert same_run(sim.bound_members(), fresh(sim.state()))
    with make_sim(gpu, s, integrator=1) as sim:
        sim.steps(2.0 ** -10, 3)
        r = sim.bound_members()
        again = sim.bound_members(start=r["member"], max_iter=1)
        assert r["converged"] and 1000 <= r["members"] <= 1190 and again["converged"] and same(again["member"], r["member"]) and same(again["e"], r["e"])


def test_options_that_ride_in_the_records_are_not_read(gpu):
    s = R.fixture_b()
    with make_sim(gpu, s) as sim:
        want, phi = sim.bound_members(), sim.potential_of()
    for opts in ({"integrator": 2, "contact": 1}, {"integrator": 2, "nearest": 1}, {"integrator": 2, "potential": 1}):
        with make_sim(gpu, s, **opts) as sim:
            if "contact" in opts:
                sim.upload_radii(np.full(len(s["m"]), 0.01, np.float32))
            sim.compute_acc_jerk()
            assert same_run(sim.bound_members(), want) and same(sim.potential_of(), phi), opts


def test_observers_leave_the_run_alone(gpu):
    """A run with the three calls interleaved leaves every later bit unchanged: state, a / j, field_of, knn_of, binaries; and
    each call returns the same bits as when it is the only observer at that point."""
    s = R.fixture_b()
    n = len(s["m"])
    p = np.stack([s[c][:40] + np.float32(0.01) for c in Q])
    mask = np.arange(n) % 3 != 0
    who = np.arange(0, n, 37, dtype=np.int32)
    seen = {}
    calls = (lambda sim: sim.potential_of(member=mask), lambda sim: sim.bound_members(),
             lambda sim: sim.potential_at(p, np.arange(40, dtype=np.int32)))

    def run(probe):
        def look(sim, at):
            if probe == "all":
                seen[at] = tuple(call(sim) for call in calls)
            elif probe is not None and at == 1:
                seen["only", probe] = calls[probe](sim)
        with make_sim(gpu, s, integrator=2) as sim:
            look(sim, 0)
            sim.steps(2.0 ** -10, 2)
            look(sim, 1)
            out = sim.evolve(2.0 ** -8, max_steps=6)
            look(sim, 2)
            st, f, b = sim.state(), sim.field_of(who), sim.binaries()
            rec = [st[k] for k in sorted(st)] + list(sim.acc()) + list(sim.jerk()) + list(sim.knn_of(who, k=6)) + [f[k] for k in sorted(f)] + \
                [b["i"], b["j"], b["h"]]
            return [bits(x) for x in rec], out
    (a, out_a), (b, out_b) = run(None), run("all")
    assert out_a == out_b and all(np.array_equal(x, y) for x, y in zip(a, b))
    for which in range(3):
        c, out_c = run(which)
        assert out_c == out_a and all(np.array_equal(x, y) for x, y in zip(a, c)), which
    assert same(seen["only", 0], seen[1][0]) and same_run(seen["only", 1], seen[1][1]) and same(seen["only", 2], seen[1][2])


# --------------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(gpu):
    s = sphere(600)
    n = 600
    lib = gpu.lib()
    P = [np.ascontiguousarray(s[c][:20] + np.float32(0.5)) for c in Q]
    skip = np.full(20, -1, np.int32)
    phi = np.zeros(20, np.float32)
    ptr = lambda x, t: x.ctypes.data_as(t) if x is not None else None      # noqa: E731

    def at(count=20, pos=P, sk=skip, out=phi):
        return lib.murbpot_at(sim._h, count, *[ptr(x, _fp) for x in pos], ptr(sk, _ip), None, ptr(out, _fp))

    def of(bodies, count=None, out=phi):
        b = np.ascontiguousarray(bodies, np.int32)
        return lib.murbpot_of(sim._h, len(b) if count is None else count, ptr(b, _ip), None, ptr(out, _fp))

    def members(max_iter=8, frame=None, out=True):
        out16 = (C.c_double * 16)(*([77.0] * 16))
        rc = lib.murbbound_members(sim._h, None, ptr(frame, _dp), max_iter, None, None, out16 if out else None)
        return rc, list(out16)

    def refused(code, rc, what):
        """The call returned its code, and a following call returns what it returned before."""
        assert rc == code, (what, rc)
        assert same(sim.potential_at(np.stack(P), skip), before) and same_run(sim.bound_members(), members_before), what

    with gpu.Simulation(n, soft=R.SOFT, g=R.G) as sim:
        assert at() == E_STATE and of([0, 1]) == E_STATE and members()[0] == E_STATE, "before the first upload"
        assert at(count=0) == 0 and of([0], count=0) == 0, "count 0 does nothing, in every state"
        assert lib.murbpot_at(None, 20, *[ptr(x, _fp) for x in P], None, None, ptr(phi, _fp)) == E_INVALID, "no context"
        sim.upload(s)
        before = sim.potential_at(np.stack(P), skip)
        members_before = sim.bound_members()
        refused(E_INVALID, at(pos=[None, P[1], P[2]]), "one position array missing")
        refused(E_INVALID, at(out=None), "no phi")
        refused(E_INVALID, of([0, 1], out=None), "no phi")
        refused(E_INVALID, lib.murbpot_of(sim._h, 3, None, None, ptr(phi, _fp)), "all bodies, but count != n")
        for bad in (np.nan, np.inf, -np.inf):
            for arr in P:
                keep = arr[7]
                arr[7] = bad
                rc = at()
                arr[7] = keep
                refused(E_INVALID, rc, f"a coordinate of {bad}")
            refused(E_INVALID, members(frame=np.array([0.0, bad, 0.0]))[0], f"a frame velocity of {bad}")
        for bad in (-2, n, 2 ** 31 - 1):
            sk = skip.copy()
            sk[19] = bad
            refused(E_INVALID, at(sk=sk), f"skip entry {bad}")
        for bad in (-1, n, -2 ** 31):
            refused(E_INVALID, of([0, bad, 1]), f"body index {bad}")
        for bad in (0, -1, 4097):
            rc, out16 = members(max_iter=bad)
            assert out16 == [77.0] * 16
            refused(E_INVALID, rc, f"max_iter {bad}")
        refused(E_INVALID, members(out=False)[0], "no out16")
        rc, out16 = members(max_iter=4096)
        assert rc == 0 and out16[0] == members_before["members"] and out16[15] == 0.0, "member and e may be NULL"
        assert at(sk=None) == 0 and of([n - 1, 0]) == 0
        with pytest.raises(ValueError):
            sim.potential_of(member=np.ones(n - 1, bool))
        with pytest.raises(ValueError):
            sim.bound_members(frame_v=[1.0, 2.0])


def test_open_block_and_two_shards_are_refused(gpu):
    s = R.fixture_b()
    n = len(s["m"])

    def run(probe):
        with make_sim(gpu, s, integrator=2) as sim:
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)
            assert not out["synchronised"]
            if probe:
                assert code_of(gpu, sim.potential_of) == E_STATE and code_of(gpu, sim.bound_members) == E_STATE
                assert code_of(gpu, lambda: sim.potential_at(np.zeros((3, 2), np.float32))) == E_STATE
            out = sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)
            assert out["synchronised"]
            st = sim.state()
            return [bits(st[k]) for k in sorted(st)] + [bits(sim.potential_of())]

    assert all(np.array_equal(x, y) for x, y in zip(run(False), run(True)))
    with gpu.Simulation(n, soft=R.SOFT, g=R.G, devices=[0, 0]) as sim:
        sim.upload(s)
        assert code_of(gpu, sim.potential_of) == E_STATE and code_of(gpu, sim.bound_members) == E_STATE


def test_span_kind(gpu):
    """"profile" 2 records the sweep launches as spans of the kind "pot" (40 points under "field_batch" 16: three launches; the
    600 bodies of a bound_members round: 38), outside the force_* figures and the field's spans."""
    s = sphere(600)

    def run(level, pot):
        with make_sim(gpu, s, field_batch=16) as sim:
            sim.set_option("profile", level)
            sim.compute_acc()
            rounds = 0
            if pot:
                sim.potential_of(np.arange(40))
                sim.potential_at(np.zeros((3, 3), np.float32))
                rounds = sim.bound_members()["rounds"]
            sim.field_of([0, 1])
            return rounds, {k: sim.info(k) for k in ("span_pot_count", "span_pot_ms_avg", "span_field_count", "span_bind_count", "force_launches")}

    (rounds, with_it), (_, without) = run(2, True), run(2, False)
    assert rounds >= 1 and with_it["span_pot_count"] == 3 + 1 + rounds * 38 and with_it["span_pot_ms_avg"] > 0
    assert without["span_pot_count"] == 0 == without["span_pot_ms_avg"] and with_it["span_bind_count"] == 0
    assert with_it["span_field_count"] == without["span_field_count"] == 1 and with_it["force_launches"] == without["force_launches"] >= 1
    assert run(1, True)[1]["span_pot_count"] == 0


# ----------------------------------------------------------------------------------------------------------------------- 9. plugin
def test_plugin_bound_members(gpu):
    """HostSim.bound_members() (SimulationNBodyHIP::boundMembers) equals Simulation.bound_members() of the same bodies, after an
    iteration too."""
    n, soft, dt = 2049, 2e8, 3600.0
    with gpu.HostSim(n, "galaxy", soft, dt) as host:
        for _ in range(2):
            st = host.state()
            got = host.bound_members()
            with gpu.Simulation(n, soft=soft) as sim:
                sim.upload(st)
                want = sim.bound_members()
            assert same_run(got, want)
            print(f"galaxy n={n}: members {got['members']}, rounds {got['rounds']}, K/|W| {got['virial_ratio']:.3f}")
            host.step(1)

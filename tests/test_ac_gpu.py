"""MI355X: the Ahmad-Cohen neighbour scheme (include/murbac.h) through the C ABI and the Python interface.  The begin state against
the read-outs it is defined by, n_irr = 1 against plain Hermite steps, every step's arithmetic restated in numpy from the device's
own list fields, the list fields against murblist_at on a context that holds the predicted state, values against
tests/helpers/ac_ref.py, energy, the read-outs as observers, batching, the refusals and the counters.  All comparisons but the two
against ac_ref are bit for bit."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ac_ref as A            # noqa: E402
import hermite_ref as H       # noqa: E402
import list_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
DT = np.float32(2.0 ** -13)   # a twentieth of the closest pairs' time scale sqrt(soft^3 / G m) of ac_ref.system; 16 steps move a body by 1e-3 of the box
STATE = A.Q + A.V
ACC = ("ax", "ay", "az")
JERK = ("jx", "jy", "jz")


def make_sim(gpu, s, integrator=2, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=A.SOFT)
    sim.set_option("integrator", integrator)
    for k, v in opts.items():
        if k in gpu.FIELD_OPTIONS:
            sim.set_field_option(k, v)
        elif k in gpu.NBR_OPTIONS:
            sim.set_neighbour_option(k, v)
        else:
            sim.set_option(k, v)
    sim.upload(s)
    return sim


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


@lru_cache(maxsize=None)
def system(n):
    """ac_ref.system(n).  Do not modify."""
    return A.system(n)


def snapshot(sim):
    """q, v, a0, j0 (3, n each) and the scheme's six planes, as the device holds them."""
    st = sim.state()
    out = {"q": np.stack([st[k] for k in A.Q]), "v": np.stack([st[k] for k in A.V]), "a0": np.stack(sim.acc()), "j0": np.stack(sim.jerk())}
    out.update(sim.ac_forces())
    return out


def same_snapshots(x, y):
    return all(same(x[k], y[k]) for k in x)


def radius_cases(n):
    """h = 0, the radii cycling through 0, 0.05, 0.1, 0.2, 0.45, and a radius that takes in every body of the unit cube."""
    return {"zero": 0.0, "cycle": A.radii(n), "all": 2.0}


def check_lengths(n):
    """The list lengths the cycling radii give, on the CPU: empty, of 1 to 2 entries, past 128 and past 256."""
    length = np.diff(R.neighbours_f32(system(n), A.radii(n), A.SOFT)[0].astype(np.int64))
    counts = [int(c) for c in ((length == 0).sum(), ((length >= 1) & (length <= 2)).sum(), (length > 128).sum(), (length > 256).sum())]
    if n == 1025:
        assert counts == [338, 127, 186, 70]
    assert min(counts) > 0, counts
    return length


# ------------------------------------------------------------------------------------------------------------------ 1. begin
@pytest.mark.parametrize("n", A.SIZES)
def test_begin_is_the_read_outs(gpu, n):
    """After ac_begin: the lists are neighbours_of's, (aI, jI) murbsplit_of's, (a0, j0) compute_acc_jerk's, aR and jR their fp32
    differences, a2R and a3R zero: bit for bit.  The second context never ran a scheme."""
    s, h = system(n), A.radii(n)
    check_lengths(n)
    with make_sim(gpu, s) as sim, make_sim(gpu, s) as ref:
        sim.ac_begin(h, 4)
        o, j = sim.ac_lists()
        ro, rj, _ = ref.neighbours_of(None, h)
        assert np.array_equal(o, ro) and np.array_equal(j, rj) and o.dtype == np.uint64 and j.dtype == np.int32
        f = sim.ac_forces()
        counts, irr = ref.irregular_field_of(None, h)
        assert np.array_equal(counts, np.diff(o))
        assert same(f["aI"], np.stack([irr[k] for k in ACC])) and same(f["jI"], np.stack([irr[k] for k in JERK]))
        ref.compute_acc_jerk()
        a0, j0 = np.stack(ref.acc()), np.stack(ref.jerk())
        assert same(np.stack(sim.acc()), a0) and same(np.stack(sim.jerk()), j0)
        assert same(f["aR"], a0 - f["aI"]) and same(f["jR"], j0 - f["jI"])
        assert not bits(f["a2R"]).any() and not bits(f["a3R"]).any()
        st = sim.ac_state()
        length = np.diff(o.astype(np.int64))
        assert st == {"n_irr": 4, "m": 0, "steps": 0, "regular_steps": 0, "entries": int(o[-1]), "longest": int(length.max()),
                      "empty": int((length == 0).sum()), "mean": float(o[-1]) / n, "time": 0.0}


# ---------------------------------------------------------------------------------------------------------------- 2. n_irr = 1
@pytest.mark.parametrize("n", A.SIZES)
@pytest.mark.parametrize("case", ["zero", "cycle", "all"])
def test_nirr_1_is_plain_hermite(gpu, n, case):
    """n_irr = 1, 5 steps: q, v, a0, j0 bit for bit murbhip_steps' under "integrator" 2, whatever the radius."""
    s, h = system(n), radius_cases(n)[case]
    with make_sim(gpu, s) as sim, make_sim(gpu, s) as ref:
        sim.ac_begin(h, 1)
        sim.ac_steps(DT, 5)
        ref.steps(DT, 5)
        x, y = sim.state(), ref.state()
        assert all(same(x[k], y[k]) for k in STATE)
        assert same(np.stack(sim.acc()), np.stack(ref.acc())) and same(np.stack(sim.jerk()), np.stack(ref.jerk()))
        st = sim.ac_state()
        assert (st["steps"], st["regular_steps"], st["m"]) == (5, 5, 0) and st["time"] == 5 * float(DT)
        if case == "all":
            assert st["entries"] == n * (n - 1) and st["empty"] == 0
        if case == "zero":
            assert st["entries"] == 0 and st["empty"] == n


# ------------------------------------------------------------------------------------------------------ 3. one step at a time
@pytest.mark.parametrize("n", A.SIZES)
def test_every_step_restated(gpu, n):
    """n_irr = 3, 7 steps, one at a time, the cycling radii.  A second context holds the predicted state (hermite_ref.predict of
    the device's q, v, a0, j0, rounded) and gives the list fields by list_field_at and the new lists by neighbours_of; from them
    the numpy corrector, polynomial and derivative update reproduce q, v, a0, j0, aR, jR, a2R, a3R bit for bit, the device's
    (aI, jI) is list_field_at's, and after a regular step ac_lists() is neighbours_of on the predicted state."""
    s, h = system(n), A.radii(n)
    n_irr = 3
    with make_sim(gpu, s) as sim, make_sim(gpu, s) as other:
        sim.ac_begin(h, n_irr)
        m = 0
        for step in range(7):
            b = snapshot(sim)
            lists = sim.ac_lists()
            sim.ac_steps(DT, 1)
            e = snapshot(sim)
            qp, vp = (np.asarray(x, np.float32) for x in H.predict(b["q"], b["v"], b["a0"], b["j0"], DT))
            other.upload({**{k: qp[i] for i, k in enumerate(A.Q)}, **{k: vp[i] for i, k in enumerate(A.V)}, "m": s["m"]})
            old = other.list_field_at(qp, vp, *lists)
            aIo, jIo = np.stack([old[k] for k in ACC]), np.stack([old[k] for k in JERK])
            regular = m + 1 == n_irr
            if not regular:
                assert same(e["aI"], aIo) and same(e["jI"], jIo), step
                aRt, jRt = A.poly(b["aR"], b["jR"], b["a2R"], b["a3R"], A.elapsed(m + 1, DT))
                a1, j1 = aIo + aRt, jIo + jRt
                for k in ("aR", "jR", "a2R", "a3R"):
                    assert same(e[k], b[k]), (step, k)
                new_lists = sim.ac_lists()
                assert np.array_equal(new_lists[0], lists[0]) and np.array_equal(new_lists[1], lists[1])
                m += 1
            else:
                a1, j1 = e["a0"], e["j0"]   # the full sweep's rows: the device's own
                other.compute_acc_jerk()
                assert same(a1, np.stack(other.acc())) and same(j1, np.stack(other.jerk())), step
                no, nj, _ = other.neighbours_of(None, h)
                got = sim.ac_lists()
                assert np.array_equal(got[0], no) and np.array_equal(got[1], nj), step
                new = other.list_field_at(qp, vp, no, nj)
                aIn, jIn = np.stack([new[k] for k in ACC]), np.stack([new[k] for k in JERK])
                assert same(e["aI"], aIn) and same(e["jI"], jIn), step
                a2R, a3R = A.derivatives(b["aR"], b["jR"], a1 - aIo, j1 - jIo, A.elapsed(n_irr, DT))
                assert same(e["a2R"], a2R) and same(e["a3R"], a3R), step
                assert same(e["aR"], a1 - aIn) and same(e["jR"], j1 - jIn), step
                m = 0
            assert same(e["a0"], a1) and same(e["j0"], j1), step
            q1, v1 = H.correct(b["q"], b["v"], b["a0"], b["j0"], a1, j1, DT, state32=True)
            assert same(e["q"], q1) and same(e["v"], v1), step
            st = sim.ac_state()
            assert (st["m"], st["steps"], st["regular_steps"]) == (m, step + 1, (step + 1) // n_irr)


# ------------------------------------------------------------------------------------------------------------------- 4. h = 0
def test_radius_zero_has_no_irregular_force(gpu):
    """h = 0, n_irr = 4: after every regular step aI == +0 and aR == a0 bit for bit (and between them aI stays +0)."""
    n = 1025
    with make_sim(gpu, system(n)) as sim:
        sim.ac_begin(0.0, 4)
        for step in range(1, 9):
            sim.ac_steps(DT, 1)
            f = sim.ac_forces()
            assert not bits(f["aI"]).any() and not bits(f["jI"]).any(), step
            if step % 4 == 0:
                assert same(f["aR"], np.stack(sim.acc())) and same(f["jR"], np.stack(sim.jerk())), step
        assert sim.ac_state()["entries"] == 0


# ------------------------------------------------------------------------------------------------------------ 5. against ac_ref
@lru_cache(maxsize=None)
def reference(n, steps):
    """(fp64-sum run, float32-sum run) of ac_ref on the cycling radii, n_irr = 4.  Do not modify."""
    s, h = system(n), A.radii(n)
    return A.run(s, h, 4, steps, A.SOFT, DT).state(), A.run(s, h, 4, steps, A.SOFT, DT, sums="f32").state()


@pytest.mark.parametrize("n", A.SIZES)
def test_values_against_the_restatement(gpu, n):
    """n_irr = 4, 16 steps against ac_ref with fp64 sums: positions and velocities within 4 x the distance between ac_ref with
    float32 sums and ac_ref with fp64 sums on the same inputs (the convention of field_ref.py / list_ref.py).
    Measured (largest error / bound): DESIGN.md 4.23."""
    r64, r32 = reference(n, 16)
    bound = [4.0 * d for d in A.distance(r32, r64)]
    with make_sim(gpu, system(n)) as sim:
        sim.ac_begin(A.radii(n), 4)
        sim.ac_steps(DT, 16)
        got = sim.state()
    err = A.distance(got, r64)
    print(f"n = {n}: |dq| {err[0]:.3e} (bound {bound[0]:.3e}), |dv| {err[1]:.3e} (bound {bound[1]:.3e})")
    assert bound[0] > 0 and bound[1] > 0
    assert err[0] <= bound[0] and err[1] <= bound[1]


def test_energy_drift(gpu):
    """n = 1025, n_irr = 4, 64 steps: the relative energy drift on the device is at most 4 x ac_ref's on the same run plus the
    drift plain Hermite shows on the device at that dt (sum order alone moves it, hence the factor).  Measured: DESIGN.md 4.23."""
    n, steps = 1025, 64
    s, h = system(n), A.radii(n)
    e0 = A.energy(s, A.SOFT)
    drift = lambda st: abs((A.energy({**st, "m": s["m"]}, A.SOFT) - e0) / e0)   # noqa: E731
    ref = drift(A.run(s, h, 4, steps, A.SOFT, DT).state())
    with make_sim(gpu, s) as sim, make_sim(gpu, s) as plain:
        sim.ac_begin(h, 4)
        sim.ac_steps(DT, steps)
        plain.steps(DT, steps)
        got, herm = drift(sim.state()), drift(plain.state())
    print(f"relative energy drift after {steps} steps: device {got:.3e}, ac_ref {ref:.3e}, plain Hermite on the device {herm:.3e}")
    assert got <= 4.0 * ref + herm


# ----------------------------------------------------------------------------------------------------------------- 6. observers
def flat(r):
    """The arrays of a read-out's result (a dict, or a tuple that may hold dicts and None), in a fixed order."""
    if isinstance(r, dict):
        return [np.asarray(r[k]) for k in sorted(r)]
    out = []
    for x in r:
        out += flat(x) if isinstance(x, dict) else [] if x is None else [np.asarray(x)]
    return out


def test_read_outs_are_observers(gpu):
    """Read-outs between ac_steps calls under "field_batch" 16 and "list_entries" 16 (n_irr = 3: irregular and regular steps follow
    them): the scheme's bits are those of an undisturbed run, and each read-out returns the bits it returns as the only
    observer, on a fresh context that took the same steps in one call."""
    n = 1025
    s, h = system(n), A.radii(n)
    who = np.arange(0, n, 7, dtype=np.int32)
    reads = (lambda x: x.field_of(who), lambda x: x.neighbours_of(who, 0.1), lambda x: x.irregular_field_of(who, 0.2),
             lambda x: x.knn_of(who, 6), lambda x: x.field_of(who))
    with make_sim(gpu, s, field_batch=16, list_entries=16) as seen, make_sim(gpu, s) as alone:
        seen.ac_begin(h, 3)
        alone.ac_begin(h, 3)
        for k, read in enumerate(reads):
            seen.ac_steps(DT, 2)
            got = flat(read(seen))
            with make_sim(gpu, s) as fresh:
                fresh.ac_begin(h, 3)
                fresh.ac_steps(DT, 2 * (k + 1))
                want = flat(read(fresh))
            assert len(got) == len(want) and len(got) > 0
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        alone.ac_steps(DT, 2 * len(reads))
        assert same_snapshots(snapshot(seen), snapshot(alone))
        lo, la = seen.ac_lists(), alone.ac_lists()
        assert np.array_equal(lo[0], la[0]) and np.array_equal(lo[1], la[1]) and seen.ac_state() == alone.ac_state()


# ------------------------------------------------------------------------------------------------------------------ 7. batching
def test_one_call_is_many_calls(gpu):
    """ac_steps(dt, 6) once equals ac_steps(dt, 1) six times (n_irr = 4: a regular step inside)."""
    n = 1025
    s, h = system(n), A.radii(n)
    with make_sim(gpu, s) as once, make_sim(gpu, s) as many:
        once.ac_begin(h, 4)
        many.ac_begin(h, 4)
        once.ac_steps(DT, 6)
        for _ in range(6):
            many.ac_steps(DT, 1)
        assert same_snapshots(snapshot(once), snapshot(many))
        assert once.ac_state() == many.ac_state()


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def code_of(call):
    with pytest.raises(Exception) as e:
        call()
    return e.value.code


def test_refusals_and_states(gpu):
    """Every refusal and state of the header's Rules."""
    n = 1025
    s, h = system(n), A.radii(n)
    L = gpu.lib()
    with make_sim(gpu, s) as sim:
        hnd = sim._h
        # nothing live yet
        assert code_of(lambda: sim.ac_steps(DT, 1)) == E_STATE and code_of(sim.ac_lists) == E_STATE and code_of(sim.ac_forces) == E_STATE
        assert sim.ac_state() == {**{k: 0 for k in gpu.AC_STATE_KEYS[:7]}, "mean": 0.0, "time": 0.0}
        sim.ac_end()
        # invalid arguments, checked before any launch
        for bad in (0, -1, gpu.AC_NIRR_MAX + 1):
            assert code_of(lambda: sim.ac_begin(h, bad)) == E_INVALID
        assert code_of(lambda: sim.ac_begin(-0.1, 4)) == E_INVALID and code_of(lambda: sim.ac_begin(np.inf, 4)) == E_INVALID
        bad_h = h.copy()
        bad_h[7] = np.nan
        assert code_of(lambda: sim.ac_begin(bad_h, 4)) == E_INVALID
        sim.ac_begin(h, gpu.AC_NIRR_MAX)
        sim.ac_begin(h, 4)   # a live scheme is replaced
        before = snapshot(sim)
        for dt in (0.0, -1.0, np.nan, np.inf):
            assert code_of(lambda: sim.ac_steps(dt, 1)) == E_INVALID
        assert code_of(lambda: sim.ac_steps(DT, -1)) == E_INVALID
        sim.ac_steps(DT, 0)
        assert L.murbac_lists(hnd, None, None, 0) == E_INVALID and L.murbac_state(hnd, None) == E_INVALID
        offsets = np.zeros(n + 1, np.uint64)
        idx = np.full(8, -7, np.int32)
        up, ip = C.POINTER(C.c_ulong), C.POINTER(C.c_int)
        assert L.murbac_lists(hnd, offsets.ctypes.data_as(up), idx.ctypes.data_as(ip), 8) == E_INVALID
        assert np.array_equal(offsets, sim.ac_lists()[0]) and np.all(idx == -7), "complete offsets, an untouched idx"
        assert L.murbac_forces(hnd, None, None, None, None) == 0
        assert same_snapshots(snapshot(sim), before) and sim.ac_state()["steps"] == 0, "a refused call changes nothing"
        # requirements
        sim.set_option("integrator", 0)
        assert code_of(lambda: sim.ac_steps(DT, 1)) == E_STATE and code_of(lambda: sim.ac_begin(h, 4)) == E_STATE
        sim.set_option("integrator", 2)
        sim.ac_steps(DT, 1)
        sim.upload_radii(np.full(n, 1e-4, np.float32))   # "contact" reads them; with "contact" off they change nothing of the scheme
        for option in ("nearest", "contact", "potential"):
            sim.ac_begin(h, 4)
            sim.set_option(option, 1)   # a change of a side option ends the scheme, and the option bars the next
            assert code_of(lambda: sim.ac_steps(DT, 1)) == E_STATE and code_of(lambda: sim.ac_begin(h, 4)) == E_STATE, option
            sim.set_option(option, 0)
        # an open block: the bodies sit at different times
        sim.ac_begin(h, 4)
        out = sim.evolve_block(4 * float(DT), blocks=1, kmax=2, max_steps=1)
        assert not out["synchronised"], "the call ended inside its block"
        assert code_of(lambda: sim.ac_begin(h, 4)) == E_STATE and code_of(lambda: sim.ac_steps(DT, 1)) == E_STATE
        sim.upload(s)
        sim.upload_tracers(np.zeros((3, 2), np.float32) + 0.5)
        assert code_of(lambda: sim.ac_begin(h, 4)) == E_STATE
        sim.clear_tracers()
        # what ends the scheme, silently
        for name, end in (("upload", lambda: sim.upload(s)), ("step", lambda: sim.step(DT)), ("steps", lambda: sim.steps(DT, 2)),
                          ("evolve", lambda: sim.evolve(4 * float(DT), dt_max=float(DT))),
                          ("evolve_block", lambda: sim.evolve_block(4 * float(DT), blocks=1, kmax=2)),
                          ("integrate_host_acc", lambda: sim.integrate_host_acc(np.zeros((3, n), np.float32), DT)),
                          ("set_block_levels", lambda: sim.set_block_levels(np.zeros(n, np.int32), 2)), ("ac_end", sim.ac_end),
                          ("init_bodies", lambda: sim.init_bodies("random"))):
            sim.ac_begin(h, 4)
            sim.ac_steps(DT, 2)
            end()
            assert code_of(lambda: sim.ac_steps(DT, 1)) == E_STATE, name
            assert code_of(sim.ac_lists) == E_STATE and code_of(sim.ac_forces) == E_STATE and sim.ac_state()["n_irr"] == 0, name
        # the bodies go on under plain Hermite steps after an ended scheme, and energy and downloads work while one is live
        sim.upload(s)
        sim.ac_begin(h, 4)
        sim.ac_steps(DT, 3)
        ke, pe = sim.energy()
        assert np.isfinite(ke) and np.isfinite(pe) and ke > 0 > pe
        mid = snapshot(sim)
        sim.ac_steps(DT, 1)
        assert not same(snapshot(sim)["q"], mid["q"])
    with gpu.Simulation(n, soft=A.SOFT) as empty:
        empty.set_option("integrator", 2)
        assert code_of(lambda: empty.ac_begin(0.1, 4)) == E_STATE, "before the first upload"
    with gpu.Simulation(n, soft=A.SOFT, devices=[0, 0]) as two:   # "integrator" 2 is refused there already
        two.upload(s)
        assert code_of(lambda: two.ac_begin(0.1, 4)) == E_STATE, "several shards"


def test_however_a_scheme_ends_the_next_hermite_step_is_the_same(gpu):
    """The scheme stopped on an irregular step (m != 0): its total is extrapolated and is not kept as a Hermite evaluation, whichever
    call ends it.  steps(), ac_end() then steps(), evolve(), evolve_block() and set_block_levels() then steps() all go on bit for bit
    like a fresh context uploaded with the same bodies.  Stopped on a regular step (n_irr = 1) the total is a full sweep's and is
    kept: ac_steps(3) then steps(2) is steps(5).  While the scheme is live compute_acc_jerk() evaluates nothing."""
    n = 1025
    s, h = system(n), A.radii(n)

    def stopped(sim):
        sim.upload(s)
        sim.ac_begin(h, 4)
        sim.ac_steps(DT, 2)
        assert sim.ac_state()["m"] == 2
        return {**sim.state(), "m": s["m"]}

    span = 4 * float(DT)
    ways = {"steps": lambda x: x.steps(DT, 2), "ac_end, steps": lambda x: (x.ac_end(), x.steps(DT, 2)),
            "set_block_levels, steps": lambda x: (x.set_block_levels(np.zeros(n, np.int32), 2), x.steps(DT, 2)),
            "evolve": lambda x: x.evolve(span, dt_max=float(DT)), "evolve_block": lambda x: x.evolve_block(span, blocks=1, kmax=2)}
    fresh_way = {"ac_end, steps": "steps"}
    with make_sim(gpu, s) as sim, make_sim(gpu, s) as fresh:
        for name, go_on in ways.items():
            mid = stopped(sim)
            before = np.stack(sim.acc())
            sim.compute_acc_jerk()
            assert same(np.stack(sim.acc()), before) and sim.ac_state()["m"] == 2, "an observer while the scheme is live"
            go_on(sim)
            fresh.upload(mid)
            ways[fresh_way.get(name, name)](fresh)
            x, y = sim.state(), fresh.state()
            assert all(same(x[k], y[k]) for k in STATE), name
            assert same(np.stack(sim.acc()), np.stack(fresh.acc())) and same(np.stack(sim.jerk()), np.stack(fresh.jerk())), name
        sim.upload(s)
        sim.ac_begin(h, 1)
        sim.ac_steps(DT, 3)
        sim.steps(DT, 2)
        fresh.upload(s)
        fresh.steps(DT, 5)
        x, y = sim.state(), fresh.state()
        assert all(same(x[k], y[k]) for k in STATE)


def test_failed_rebuild(gpu):
    """A rebuild whose total passes 2^31 - 1 entries returns MURBHIP_E_INVALID, leaves the bodies at the end of the last completed
    step and ends the scheme.  n = 46 342 is the smallest n with n (n - 1) > 2^31 - 1; the limit is checked after the count pass and
    before anything is allocated.  Bodies of negligible mass in the unit cube fall towards the origin at q / (2 dt) x 0.95: with
    h = 0.1 the lists of ac_begin hold a few entries per thousand bodies, the irregular step succeeds, and the regular step's
    predicted positions lie within 0.05 sqrt(3) < h of each other, every body then being every body's neighbour.  A radius that
    takes in every body fails in ac_begin in the same way."""
    n, dt = 46342, np.float32(2.0 ** -6)
    assert n * (n - 1) > 2 ** 31 - 1 >= (n - 1) * (n - 2)
    rng = np.random.default_rng(7)
    q = rng.uniform(0.0, 1.0, (3, n)).astype(np.float32)
    v = (-q.astype(np.float64) * 0.95 / (2.0 * float(dt))).astype(np.float32)
    s = {**{k: q[i] for i, k in enumerate(A.Q)}, **{k: v[i] for i, k in enumerate(A.V)}, "m": np.ones(n, np.float32)}
    with make_sim(gpu, s) as sim:
        sim.ac_begin(0.1, 2)
        st = sim.ac_state()
        assert 0 < st["entries"] < 2 ** 27
        sim.ac_steps(dt, 1)
        mid = sim.state()
        assert np.abs(np.stack([mid[k] for k in A.Q]) - q.astype(np.float64) * 0.525).max() < 1e-4, "half way, in a straight line"
        assert code_of(lambda: sim.ac_steps(dt, 1)) == E_INVALID
        after = sim.state()
        assert all(same(after[k], mid[k]) for k in STATE), "the bodies stand at the end of the last completed step"
        assert sim.ac_state()["n_irr"] == 0 and code_of(lambda: sim.ac_steps(dt, 1)) == E_STATE and code_of(sim.ac_lists) == E_STATE
        sim.steps(dt, 1)   # and plain Hermite goes on from there
        end = sim.state()
        assert np.abs(np.stack([end[k] for k in A.Q])).max() < 0.06
        sim.upload(s)
        assert code_of(lambda: sim.ac_begin(2.0, 2)) == E_INVALID and code_of(lambda: sim.ac_steps(dt, 1)) == E_STATE
        got = sim.state()
        assert all(same(got[k], s[k]) for k in STATE)


# ------------------------------------------------------------------------------------------------------------------ 9. ac_radii
@pytest.mark.parametrize("k", [1, 12, 40])
def test_radii_give_k_entries(gpu, k):
    """ac_radii(k): every body's list has at least k entries, and (k within knn_of's columns) some list has exactly k."""
    n = 1025
    with make_sim(gpu, system(n)) as sim:
        h = sim.ac_radii(k)
        assert h.dtype == np.float32 and h.shape == (n,) and np.all(h > 0)
        sim.ac_begin(h, 2)
        length = np.diff(sim.ac_lists()[0].astype(np.int64))
        st = sim.ac_state()
        assert length.min() >= k and st["empty"] == 0 and st["longest"] == length.max()
        if k <= gpu.KNN_KMAX:
            assert length.min() == k


# ------------------------------------------------------------------------------------------------------------------ 10. plugin
def test_plugin_ac_steps(gpu):
    """SimulationNBodyHIP::acBegin / acSteps (HostSim.ac_begin / ac_steps on the Hermite plugin) and the `hip+hermite+ac` plugin
    (HostSim(integrator=5, rnb=, nirr=): one step of dt per iteration, begun at the first) both leave the bodies where the
    binding's ac_begin / ac_steps leave the same bodies, bit for bit; the neighbour radius gives lists."""
    n, soft, dt, n_irr = 2049, 2e8, 3600.0, 3
    with gpu.HostSim(n, "galaxy", soft, dt, integrator=2) as host:
        st = host.state()
    h = 0.02 * float(np.ptp(st["qx"]))
    with gpu.Simulation(n, soft=soft) as sim:
        sim.set_option("integrator", 2)
        sim.upload(st)
        sim.ac_begin(h, n_irr)
        assert sim.ac_state()["longest"] > 2 and sim.ac_state()["empty"] > 0, "some bodies have neighbours and some have none"
        sim.ac_steps(dt, 7)
        want = sim.state()
    with gpu.HostSim(n, "galaxy", soft, dt, integrator=2) as host:
        host.ac_begin(h, n_irr)
        host.ac_steps(dt, 7)
        got = host.state()
        assert all(same(got[k], want[k]) for k in STATE)
        with pytest.raises(gpu.MurbHipError) as e:
            host.ac_begin(h, 0)
        assert e.value.code == E_INVALID
    with gpu.HostSim(n, "galaxy", soft, dt, integrator=5, rnb=h, nirr=n_irr) as plug:
        plug.step(7)
        got = plug.state()
        assert all(same(got[k], want[k]) for k in STATE)
        assert plug.history()["energy"].shape == (7,)
    with gpu.HostSim(n, "galaxy", soft, dt) as plain:   # "integrator" 0: the scheme is refused, the plugin goes on
        with pytest.raises(gpu.MurbHipError) as e:
            plain.ac_begin(h, n_irr)
        assert e.value.code == E_STATE
    with pytest.raises(ValueError):
        gpu.HostSim(n, "galaxy", soft, dt, integrator=5, rnb=h, nirr=0)


def test_murb_hip_cli_ac(gpu, tmp_path):
    """`murb-hip --im hip+hermite+ac --rnb R --nirr K`: hip+hermite's banner and final line; with --nirr 1 the tracked energies
    are hip+hermite's to the last digit (the scheme is then plain Hermite bit for bit); a bad --nirr or --rnb ends the program."""
    import re
    import subprocess
    exe = os.path.join(ROOT, "nbody-eurohpc_amd", "bin", "murb-hip")
    rows = {}
    for tag, extra in (("hip+hermite", []), ("hip+hermite+ac", ["--rnb", "2e9", "--nirr", "1"]), ("hip+hermite+ac", ["--rnb", "2e9", "--nirr", "3"])):
        csv = tmp_path / f"m{len(rows)}.csv"
        r = subprocess.run([exe, "-n", "2048", "-i", "6", "--nv", "--im", tag, "--gf", "--csv", str(csv)] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert "  -> implementation    (--im  ): " + tag in r.stdout
        assert re.search(r"Entire simulation took ([0-9.e+]+) ms \(([0-9.e+]+) FPS, +([0-9.]+) Gflop/s\)", r.stdout), r.stdout
        rows[(tag, tuple(extra))] = csv.read_text().splitlines()
    plain, one, three = rows.values()
    assert len(plain) == len(one) == len(three) == 7 and one == plain
    e = [float(x.split(",")[1]) for x in three[1:]]
    assert abs(e[-1] - e[0]) < 1e-3 * abs(e[0])
    for bad in (["--nirr", "0"], ["--nirr", "4097"], ["--rnb", "-1"]):
        r = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", "hip+hermite+ac"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "exiting" in r.stdout, bad
    for other in (["--nirr", "3"], ["--rnb", "1e9"]):   # like --renc: an option of another implementation is refused, not ignored
        r = subprocess.run([exe, "-n", "64", "-i", "1", "--nv", "--im", "hip+hermite"] + other, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "need hip+hermite+ac" in r.stdout, other
    h = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert "hip+hermite+ac" in h.stdout + h.stderr and "--nirr" in h.stdout + h.stderr

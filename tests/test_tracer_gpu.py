"""GPU: massless tracers (include/murbtracer.h) through the C ABI, the Python interface and the plugin.

The normative tie is to a yardstick the parent commit has: a tracer's (a, j) are murbfield_at's bits for the same point, velocity
and no skipped body at the same chunk count.  Everything else is built on that and on the fp64 restatement of predictor and
corrector (tests/helpers/hermite_ref.py, bit-exact with fp32 stores): one step of the tracers is reproduced bit for bit from a
second context that holds the restatement's PREDICTED bodies.  Reproducibility, the bodies being left alone and the state rules
are differential, bit for bit."""
import ctypes as C
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import field_ref as F         # noqa: E402
import hermite_ref as H       # noqa: E402
import tracer_ref as T        # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -2000, -2001
SIZES = (2, 513, 1500)            # one tile, two tiles, a ragged three-tile layout
COUNTS = (1, 15, 16, 17, 33, 100)
BATCHES = (16, 32, 0)             # 0: the default; 33 and 100 tracers then need several launches per step
FKEYS = F.KEYS[:6]
SKEYS = T.Q + T.V
_fp = C.POINTER(C.c_float)


def make_sim(gpu, s, tracers=None, soft=T.SOFT, **opts):
    sim = gpu.Simulation(len(s["m"]), soft=soft)
    sim.set_option("integrator", 2)
    for k, v in opts.items():
        if k in gpu.TRACER_OPTIONS:
            sim.set_tracer_option(k, v)
        elif k in gpu.FIELD_OPTIONS:
            sim.set_field_option(k, v)
        else:
            sim.set_option(k, v)
    sim.upload(s)
    if tracers is not None:
        sim.upload_tracers(*tracers)
    return sim


def code_of(gpu, call):
    with pytest.raises(gpu.MurbHipError) as e:
        call()
    return e.value.code


def set_chunks(sim, chunks):
    """"tracer_chunks" and "field_chunks" resolved to the same count."""
    sim.set_tracer_option("tracer_chunks", chunks)
    sim.set_field_option("field_chunks", chunks)
    assert sim.tracer_option("tracer_chunks") == sim.field_option("field_chunks")
    return sim.tracer_option("tracer_chunks")


def tracer_record(sim, forces=True):
    """Everything a context says about its tracers, as one dict of arrays."""
    out = dict(sim.tracers())
    if forces:
        out.update(sim.tracer_forces())
    return out


def body_record(sim, option=None):
    out = dict(sim.state())
    out.update(zip(("ax", "ay", "az"), sim.acc()))
    out.update(zip(("jx", "jy", "jz"), sim.jerk()))
    if option == "nearest":
        out["nn"], out["nn_r2"] = sim.nearest()
    if option == "potential":
        out["phi"] = sim.potential()
    return out


def st(d, keys):
    return np.stack([d[k] for k in keys])


@lru_cache(maxsize=None)
def case(n):
    """(bodies, tq, tv, fp64 reference of the field at the 100 tracers, C of field_ref's bound): CPU only, made once."""
    s = F.system(n)
    tq, tv = T.tracers(s, max(COUNTS))
    ref, c = F.bound_of(tq, tv, None, s, T.SOFT)
    return s, tq, tv, ref, c


# ------------------------------------------------------------------------------------------ 1. evaluation equals the read-out
@pytest.mark.parametrize("n", SIZES)
def test_evaluation_equals_the_readout(gpu, n):
    """compute_tracers() then tracer_forces(): the bits of field_at(q, v, skip=None) (ax ... jz) for every count, chunk count
    and batch, and both within tests/test_field_gpu.py's bound of the fp64 sum (field_ref.bound_of / check, as it states it)."""
    s, tq, tv, ref, c = case(n)
    tiles = -(-n // 512)
    with make_sim(gpu, s) as sim:
        for chunks in sorted({1, min(2, tiles), min(3, tiles)}):
            assert set_chunks(sim, chunks) == chunks
            whole = sim.field_at(tq, tv)
            for batch in BATCHES:
                sim.set_tracer_option("tracer_batch", batch)
                for m in COUNTS:
                    sim.upload_tracers(tq[:, :m], tv[:, :m])
                    assert sim.tracer_count() == m
                    assert code_of(gpu, sim.tracer_forces) == E_STATE, "no evaluation is current after an upload"
                    sim.compute_tracers()
                    got = sim.tracer_forces()
                    fld = sim.field_at(tq[:, :m], tv[:, :m])
                    for k in FKEYS:
                        assert np.array_equal(F.bits(got[k]), F.bits(fld[k])), f"n={n} chunks={chunks} batch={batch} M={m}: {k}"
                        assert np.array_equal(F.bits(got[k]), F.bits(whole[k][:m])), "the count changed a tracer's bits"
                    back = sim.tracers()
                    assert all(np.array_equal(F.bits(back[k]), F.bits(x[:m])) for k, x in zip(SKEYS, list(tq) + list(tv)))
                    if batch == 0:
                        both = (st(got, FKEYS[:3]), st(got, FKEYS[3:]), fld["phi"])
                        F.check(both, ref, c, f"n={n} chunks={chunks} M={m}", rows=np.arange(m))
        sim.upload_tracers(tq[:, :5])          # at rest
        sim.compute_tracers()
        rest = sim.tracer_forces()
        fld = sim.field_at(tq[:, :5], None)
        assert all(np.array_equal(F.bits(rest[k]), F.bits(fld[k])) for k in FKEYS) and not st(sim.tracers(), T.V).any()


# ---------------------------------------------------------------------------------------------------- 2. one step, bit for bit
def expected_step(gpu, s, bodies, a0, j0, tr, dt, chunks):
    """The tracers after one step of size dt, from the restatement: the bodies' predicted state (bit-exact) goes to a second
    context, murbfield_at there at the restatement's predicted tracers is (a1, j1), then the fp64 corrector with fp32 stores."""
    pred = T.predicted_state({**bodies, "m": s["m"]}, a0, j0, dt)
    tq, tv, ta0, tj0 = st(tr, T.Q), st(tr, T.V), st(tr, FKEYS[:3]), st(tr, FKEYS[3:])
    tp, tw = (np.asarray(x, np.float32) for x in H.predict(tq, tv, ta0, tj0, dt))
    with gpu.Simulation(len(s["m"]), soft=T.SOFT) as second:
        second.set_field_option("field_chunks", chunks)
        second.upload(pred)
        f = second.field_at(tp, tw)
    a1, j1 = st(f, FKEYS[:3]), st(f, FKEYS[3:])
    q1, v1 = H.correct(tq, tv, ta0, tj0, a1, j1, dt, state32=True)
    out = {k: np.asarray(x, np.float32) for k, x in zip(SKEYS, list(q1) + list(v1))}
    out.update({k: x for k, x in zip(FKEYS, list(a1) + list(j1))})
    return out


@pytest.mark.parametrize("n", SIZES)
def test_one_step_bit_for_bit(gpu, n):
    """Three consecutive murbhip_step(dt) and one murbhip_evolve with max_steps 1 (dt from out5): the device's tracer q, v and
    remembered (a0, j0) equal the restatement's in every bit.  The field is taken at the bodies' PREDICTED state: a sweep that
    read the current records instead differs in (a1, j1) from the first step on."""
    s, tq, tv, _, _ = case(n)
    m = 33
    tiles = -(-n // 512)
    with make_sim(gpu, s, (tq[:, :m], tv[:, :m]), tracer_batch=16) as sim:
        chunks = set_chunks(sim, min(2, tiles))
        sim.compute_acc_jerk()
        sim.compute_tracers()
        for step in range(4):
            bodies = sim.state()
            a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
            tr = tracer_record(sim)
            if step < 3:
                dt = T.DT
                sim.step(dt)
            else:
                out = sim.evolve(10 * float(T.DT), max_steps=1)
                assert out["steps"] == 1 and out["dt_min"] == out["dt_max"]
                dt = np.float32(out["dt_min"])
            want = expected_step(gpu, s, bodies, a0, j0, tr, dt, chunks)
            got = tracer_record(sim)
            moved = any(not np.array_equal(F.bits(got[k]), F.bits(tr[k])) for k in T.Q)
            assert moved, "the step did not move the tracers"
            for k in SKEYS + FKEYS:
                bad = np.flatnonzero(F.bits(got[k]) != F.bits(want[k]))
                assert bad.size == 0, f"n={n} step {step} (dt={dt}): {k} of tracers {bad[:8]} differs from the restatement"


# ------------------------------------------------------------------------------------------------------ 3. bodies untouched
def clock_tracer():
    """One tracer that starts at x = 0 with velocity (1, 0, 0), 1e6 box lengths above the bodies: a clock.  The bodies' pull on
    it is at most G M / z^2 = 7e-10 (G M <= 1.34 x 513) and its x part 1e-15, which is 1e-8 of vx's last place over the runs
    below: vx stays 1 in every bit, and the corrector's x + dt (v0 + v1) / 2 + dt^2 (a0 - a1) / 12 is x + dt exactly in fp64 (the
    last term is below 1e-22, under half a last place of the fp64 sum), rounded once to fp32.  So the clock's x after a run is
    x <- fp32(x + dt) over the steps the bodies took, in every bit: one step less or more moves it by several last places (the
    steps are 2e-8 and more, a last place below x = 0.125 is 7.5e-9 at the most)."""
    return np.array([[0.0], [0.0], [1e6]], np.float32), np.array([[1.0], [0.0], [0.0]], np.float32)


def clock_after(x, dts):
    for dt in np.asarray(dts, np.float32):
        x = np.float32(np.float64(x) + np.float64(dt))
    return x


@pytest.mark.parametrize("option", [None, "nearest", "potential"])
def test_bodies_untouched(gpu, option):
    """"tracer_dt" 0: steps(20), evolve over a fixed duration (several batches of enqueued steps) and evolve ended by an encounter
    stop, with and without tracers: the bodies' q, v, a, j, out5, the nearest / potential read-outs and the encounter list are
    identical in every bit, and the tracers sit at the bodies' model time after each of the three: the clock tracer's x has
    the bits of x <- fp32(x + dt) over the step ring's dts, whose sum is the model time out5 reports, so a tracer that missed a
    step, took one too many, or was carried past the step that hit fails."""
    s, tq, tv, _, _ = case(513)
    cq, cv = clock_tracer()
    tracers = (np.concatenate([tq[:, :32], cq], 1), np.concatenate([tv[:, :32], cv], 1))
    opts = {option: 1} if option else {}
    records = []
    for with_tracers in (False, True):
        with make_sim(gpu, s, tracers if with_tracers else None, tracer_batch=16, **opts) as sim:
            rec = {}
            clock = {"x": np.float32(0.0)}

            def at_model_time(what, dts, time):
                """`dts`: the steps of the run just made; `time`: the model time it reports."""
                dts = np.asarray(dts, np.float32)
                total = float(np.sum(dts, dtype=np.float64))
                # the device's clock adds the fp32 steps in fp64; the last step of a run to its end is the remaining time rounded to fp32
                assert abs(total - time) <= float(np.spacing(dts.max())), f"{what}: the steps add up to {total}, the model time is {time}"
                clock["x"] = clock_after(clock["x"], dts)
                if not with_tracers:
                    return
                tr = sim.tracers()
                x, vx = tr["qx"][-1], tr["vx"][-1]
                print(f"{option} {what}: clock tracer at {float(x)!r}, restated {float(clock['x'])!r}, {len(dts)} steps of "
                      f"{float(dts.min()):.3e} to {float(dts.max()):.3e} adding up to {total!r}")
                assert float(dts.min()) > 2 * float(np.spacing(clock["x"])), "the clock does not resolve the smallest step"
                assert vx == np.float32(1.0) and F.bits(x) == F.bits(clock["x"]), \
                    f"after {what} the clock tracer sits at {float(x)!r}, the bodies' steps put it at {float(clock['x'])!r}"
                assert np.isfinite(st(tr, SKEYS)).all()

            sim.steps(T.DT, 20)
            rec["steps"] = body_record(sim, option)
            at_model_time("steps(20)", [T.DT] * 20, 20 * float(T.DT))
            out = sim.evolve(0.01)
            assert out["steps"] > 4, "the run is meant to span several batches (the first of a fresh call is 4 steps)"
            rec["evolve"] = body_record(sim, option)
            rec["out5"] = out
            rec["dts"] = sim.evolve_dts()
            assert len(rec["dts"]) == out["steps"], "the step ring holds the whole run"
            at_model_time("evolve", rec["dts"], out["time"])
            if option == "nearest":
                _, r2 = sim.nearest()
                sim.set_encounter(float(np.sqrt(max(r2.min() - float(T.SOFT) ** 2, 0.0))) * 1.5)
                out = sim.evolve(0.05)
                enc = sim.encounters()
                assert enc["count"] > 0 and out["time"] < 0.05, "the encounter stop did not end the run"
                rec["stop"] = body_record(sim, option)
                rec["stop_out5"] = out
                rec["enc"] = enc
                rec["stop_dts"] = sim.evolve_dts()
                assert len(rec["stop_dts"]) == out["steps"], "the step ring holds the whole run"
                at_model_time("the encounter stop", rec["stop_dts"], out["time"])
            records.append(rec)
    without, with_ = records
    for key in without:
        assert T.same(without[key], with_[key]), f"{option}: the tracers changed the bodies' {key}"


# ------------------------------------------------------------------------------------------------------------- 4. company
def test_company(gpu):
    """One tracer's bits after 5 steps: alone; as the first, 16th, 17th and last of a set of 33; in the reversed set; under
    each batch value: all equal.  The padded copies in the last group of 16 leave no trace: tracer M - 1 of a set of 17
    equals the same tracer alone (a build that drops or mis-stores the ragged last group differs here)."""
    s, tq, tv, _, _ = case(513)
    x = 7                                           # the tracer followed

    def run(order, batch):
        order = np.asarray(order)
        with make_sim(gpu, s, (tq[:, order], tv[:, order]), tracer_batch=batch) as sim:
            sim.steps(T.DT, 5)
            rec = tracer_record(sim)
        at = int(np.flatnonzero(order == x)[0])
        assert len(rec["qx"]) == len(order)
        return {k: v[at:at + 1] for k, v in rec.items()}, rec

    alone, _ = run([x], 0)
    others = [k for k in range(40) if k != x][:32]
    for place in (0, 15, 16, 32):
        order = others[:place] + [x] + others[place:]
        for batch in BATCHES:
            got, _ = run(order, batch)
            assert T.same(got, alone), f"place {place} of 33, batch {batch}"
    order = others[:16] + [x] + others[16:]
    fwd, whole = run(order, 16)
    back, whole_r = run(order[::-1], 16)
    assert T.same(back, alone) and all(np.array_equal(F.bits(whole[k]), F.bits(whole_r[k][::-1])) for k in whole), "reversed order"
    for batch in BATCHES:
        last17, rec17 = run(others[:16] + [x], batch)
        assert T.same(last17, alone), f"last of 17, batch {batch}: the ragged last group"
        assert np.isfinite(st(rec17, SKEYS + FKEYS)).all()


# ------------------------------------------------------------------------------------------------------------ 5. "tracer_dt" 1
def tight_system():
    """A heavy body (G m = 1) at rest, a light body (G m = 1e-6) 100 away on a slow orbit, soft 1e-4; one tracer on a circular
    orbit of radius 0.01 about the heavy body (period 6.3e-3), or far away from everything."""
    g = float(H.G)
    s = {k: np.zeros(2, np.float32) for k in SKEYS}
    s["qx"][1] = 100.0
    s["vy"][1] = 0.1
    s["m"] = np.array([1.0 / g, 1e-6 / g], np.float32)
    near = (np.array([[0.01], [0.0], [0.0]], np.float32), np.array([[0.0], [10.0], [0.0]], np.float32))
    far = (np.array([[0.0], [0.0], [1e4]], np.float32), np.zeros((3, 1), np.float32))
    return s, np.float32(1e-4), near, far


def test_tracer_dt(gpu):
    """With "tracer_dt" 1 a tracer on a tight orbit makes evolve take more steps than with 0, and every step's dt is at most the
    restatement's Aarseth step of that tracer (the first: eta_start |a0| / |j0|); with the tracer far away from everything
    the option changes no bit."""
    s, soft, near, far = tight_system()
    eta, eta_start, duration = 0.02, 0.01, 0.01
    steps = {}
    for mode in (0, 1):
        with make_sim(gpu, s, near, soft=soft, tracer_dt=mode) as sim:
            out = sim.evolve(duration, eta=eta, eta_start=eta_start, dt_max=duration / 4)
            steps[mode] = out["steps"]
            assert abs(out["time"] - duration) <= 1e-12
    print("steps with tracer_dt 0 / 1:", steps)
    assert steps[0] <= 5 and steps[1] > 10 * steps[0]      # 0: the bodies alone ask for dt_max, a quarter of the duration
    with make_sim(gpu, s, near, soft=soft, tracer_dt=1) as sim:
        sim.compute_tracers()
        f0 = sim.tracer_forces()
        bound = np.float32(T.first_step(st(f0, FKEYS[:3]), st(f0, FKEYS[3:]), eta_start)[0])
        for k in range(24):
            out = sim.evolve(duration, eta=eta, eta_start=eta_start, dt_max=duration / 4, max_steps=1)
            dt = np.float32(out["dt_min"])
            assert out["steps"] == 1 and dt <= bound, f"step {k}: dt {dt} above the tracer's own step {bound}"
            f1 = sim.tracer_forces()
            bound = np.float32(T.aarseth_step(st(f0, FKEYS[:3]), st(f0, FKEYS[3:]), st(f1, FKEYS[:3]), st(f1, FKEYS[3:]), dt, eta)[0])
            assert np.float32(out["dt_next"]) <= bound
            f0 = f1
    recs = []
    for mode in (0, 1):
        with make_sim(gpu, s, far, soft=soft, tracer_dt=mode) as sim:
            out = sim.evolve(duration, eta=eta, eta_start=eta_start, dt_max=duration / 4)
            recs.append((out, sim.evolve_dts(), body_record(sim), tracer_record(sim)))
    assert recs[0][0] == recs[1][0] and all(T.same(a, b) for a, b in zip(recs[0][1:], recs[1][1:])), "a far tracer changed a bit"


# ------------------------------------------------------------------------------------------------------------ 6. state rules
def test_refusals(gpu):
    """Every refusal the header lists returns its code."""
    s, tq, tv, _, _ = case(513)
    n, L = 513, gpu.lib()
    q, v = tq[:, :17].copy(), tv[:, :17].copy()
    with gpu.Simulation(n, soft=T.SOFT) as sim:                  # "integrator" 0
        sim.upload(s)
        for integrator in (0, 1):
            sim.set_option("integrator", integrator)
            assert code_of(gpu, lambda: sim.upload_tracers(q, v)) == E_STATE
        assert sim.tracer_count() == 0
    with gpu.Simulation(n, soft=T.SOFT, devices=[0, 0]) as two:  # several shards
        two.upload(s)
        assert code_of(gpu, lambda: two.upload_tracers(q, v)) == E_STATE
    with make_sim(gpu, s) as sim:
        out = sim.evolve_block(0.5, blocks=1, kmax=3, max_steps=1)                  # every body wants less than 1/16: a block of 8 steps
        assert not out["synchronised"], "the block is meant to stay open"
        assert code_of(gpu, lambda: sim.upload_tracers(q, v)) == E_STATE and sim.tracer_count() == 0
        assert code_of(gpu, sim.clear_tracers) == E_STATE
        sim.upload(s)                                                               # closes it
        sim.upload_tracers(q, v)
        p = [np.ascontiguousarray(x) for x in list(q) + list(v)]
        ptr = [x.ctypes.data_as(_fp) for x in p]
        for k in range(3):
            a = list(ptr)
            a[k] = None
            assert L.murbtracer_upload(sim._h, 17, *a) == E_INVALID
        assert L.murbtracer_upload(sim._h, 17, *ptr[:4], None, None) == E_INVALID
        bad = [x.copy() for x in p]
        bad[4][16] = np.inf
        assert L.murbtracer_upload(sim._h, 17, *[x.ctypes.data_as(_fp) for x in bad]) == E_INVALID
        out = [np.zeros(17, np.float32) for _ in range(6)]
        assert L.murbtracer_download_forces(sim._h, out[0].ctypes.data_as(_fp), None, None, None, None, None) == E_INVALID
        assert L.murbtracer_set_option(sim._h, b"tracer_batch", 24) == E_INVALID
        assert L.murbtracer_set_option(sim._h, b"tracer_dt", 2) == E_INVALID
        assert L.murbtracer_set_option(sim._h, b"tracer_chunks", -1) == E_INVALID
        assert L.murbtracer_set_option(sim._h, b"field_chunks", 1) == E_INVALID
        assert sim.tracer_count() == 17 and T.same(sim.tracers(), dict(zip(SKEYS, p)))
        for integrator in (0, 1):
            assert code_of(gpu, lambda: sim.set_option("integrator", integrator)) == E_STATE
        assert code_of(gpu, lambda: sim.evolve_block(float(T.DT) * 8, blocks=1, kmax=3)) == E_STATE
        assert code_of(gpu, lambda: sim.set_block_levels(np.zeros(n, np.int32), 3)) == E_STATE
        assert code_of(gpu, sim.tracer_forces) == E_STATE
        sim.clear_tracers()
        assert sim.tracer_count() == 0
        sim.set_option("integrator", 0)                                             # free again
        sim.set_option("integrator", 2)
        sim.upload_tracers(q[:, :0], None)                                          # count 0 clears
        assert sim.tracer_count() == 0


def refused_calls(gpu, sim, q, v):
    """The refused calls of a context with resident tracers; each must return its code."""
    L = gpu.lib()
    n = sim.n
    p = [np.ascontiguousarray(x) for x in list(q) + list(v)]
    bad = [x.copy() for x in p]
    bad[0][0] = np.nan
    assert L.murbtracer_upload(sim._h, len(bad[0]), *[x.ctypes.data_as(_fp) for x in bad]) == E_INVALID
    assert L.murbtracer_upload(sim._h, 3, None, None, None, None, None, None) == E_INVALID
    assert code_of(gpu, lambda: sim.set_option("integrator", 0)) == E_STATE
    assert code_of(gpu, lambda: sim.evolve_block(float(T.DT) * 8, blocks=1, kmax=3)) == E_STATE
    assert code_of(gpu, lambda: sim.set_block_levels(np.zeros(n, np.int32), 3)) == E_STATE
    assert L.murbtracer_set_option(sim._h, b"tracer_dt", 7) == E_INVALID
    assert L.murbtracer_set_option(sim._h, b"tracer_batch", 17) == E_INVALID


@pytest.mark.parametrize("option", [None, "nearest", "contact", "potential"])
def test_refused_calls_and_readouts_change_nothing(gpu, option):
    """A short sequence (steps, evolve, an upload of the bodies, steps) run three times: plain; with every refused call between
    its parts; with murbfield_at / murbtidal_at between its parts.  Every later bit of bodies and tracers is the same, the
    read-outs return what they return on a context without tracers at the same body state, and "nearest", "contact" or
    "potential" may be on.  murbhip_upload of the bodies keeps the tracers' q and v and makes tracer_forces refuse until the next
    evaluation."""
    s, tq, tv, _, _ = case(513)
    q, v = tq[:, :33], tv[:, :33]
    opts = {option: 1} if option else {}
    radii = np.full(513, 1e-3, np.float32)

    def sequence(between, tracers=True):
        log = []
        with make_sim(gpu, s, (q, v) if tracers else None, tracer_batch=16, **opts) as sim:
            if option == "contact":
                sim.upload_radii(radii)
            between(sim)
            sim.steps(T.DT, 3)
            log.append(between(sim))
            if tracers:
                log.append(tracer_record(sim))
            out = sim.evolve(0.004)
            log.append(out["steps"])
            log.append(between(sim))
            if tracers:
                before = sim.tracers()
            sim.upload(s)
            if option == "contact":
                sim.upload_radii(radii)
            if tracers:
                assert T.same(sim.tracers(), before), "an upload of the bodies moved the tracers"
                assert code_of(gpu, sim.tracer_forces) == E_STATE
                if between is nothing:
                    sim.compute_tracers()
                    again = sim.tracer_forces()
                    fld = sim.field_at(st(before, T.Q), st(before, T.V))
                    assert all(np.array_equal(F.bits(again[k]), F.bits(fld[k])) for k in FKEYS)
            between(sim)
            sim.steps(T.DT, 2)
            log.append(body_record(sim, option if option != "contact" else None))
            if tracers:
                log.append(tracer_record(sim))
        return log

    def nothing(sim):
        return None

    def refused(sim):
        if sim.tracer_count():
            refused_calls(gpu, sim, q, v)
        return None

    probe = (tq[:, 40:57], tv[:, 40:57])

    def readouts(sim):
        sim.set_field_option("field_chunks", 1)
        return sim.field_at(*probe), sim.tidal_at(probe[0])

    plain = sequence(nothing)
    with_refused = sequence(refused)
    with_readouts = sequence(readouts)
    no_tracers = sequence(readouts, tracers=False)

    def strip(log):
        return [x for x in log if not isinstance(x, tuple) and x is not None]

    for a, b in zip(strip(plain), strip(with_refused)):
        assert T.same(a, b) if isinstance(a, dict) else a == b, "a refused call changed a later bit"
    for a, b in zip(strip(plain), strip(with_readouts)):
        assert T.same(a, b) if isinstance(a, dict) else a == b, "a read-out between the steps changed a later bit"
    mine = [x for x in with_readouts if isinstance(x, tuple)]
    theirs = [x for x in no_tracers if isinstance(x, tuple)]
    assert len(mine) == len(theirs) == 2
    for (f1, t1), (f2, t2) in zip(mine, theirs):
        assert T.same(f1, f2) and T.same(t1, t2), "the tracers changed a read-out's bits"


def test_new_bodies_and_radii_keep_the_tracers(gpu):
    """murbhip_upload_radii and murbhip_init_bodies with tracers resident and their evaluation current (straight after steps):
    each keeps the tracers' q and v in every bit and drops only the evaluation, so tracer_forces refuses until the next one.
    What the device kept is what it steps from: the next step gives the bits of a fresh context that gets the same bodies and
    the downloaded tracers."""
    n, soft, dt = 513, np.float32(2e8), np.float32(3600.0)
    s = gpu.init_bodies(n, "galaxy")
    rng = np.random.default_rng(11)
    q = (float(np.abs(s["qx"]).max()) * rng.uniform(-1, 1, (3, 17))).astype(np.float32)
    v = (1e3 * rng.standard_normal((3, 17))).astype(np.float32)
    radii = np.full(n, 1e6, np.float32)

    def dropped(sim, before, what):
        assert T.same(sim.tracers(), before), f"{what} moved the tracers"
        assert sim.tracer_count() == 17 and code_of(gpu, sim.tracer_forces) == E_STATE, f"{what} kept the tracers' evaluation"
        sim.compute_tracers()
        got, fld = sim.tracer_forces(), sim.field_at(st(before, T.Q), st(before, T.V))
        assert all(np.array_equal(F.bits(got[k]), F.bits(fld[k])) for k in FKEYS), f"the evaluation after {what}"

    with make_sim(gpu, s, (q, v), soft=soft) as sim:
        set_chunks(sim, 1)
        sim.steps(dt, 2)
        sim.tracer_forces()                         # current: the steps left it
        before = sim.tracers()
        sim.upload_radii(radii)
        dropped(sim, before, "murbhip_upload_radii")
        sim.steps(dt, 2)
        sim.tracer_forces()
        before = sim.tracers()
        sim.init_bodies("galaxy", 5)
        assert code_of(gpu, sim.tracer_forces) == E_STATE, "murbhip_init_bodies kept the tracers' evaluation"
        assert T.same(sim.tracers(), before), "murbhip_init_bodies moved the tracers"
        sim.steps(dt, 2)                            # evaluates the tracers against the new bodies first
        got, bodies = tracer_record(sim), sim.state()
    with gpu.Simulation(n, soft=soft) as fresh:
        fresh.set_option("integrator", 2)
        fresh.set_tracer_option("tracer_chunks", 1)
        fresh.init_bodies("galaxy", 5)
        fresh.upload_tracers(st(before, T.Q), st(before, T.V))
        fresh.steps(dt, 2)
        assert T.same(tracer_record(fresh), got), "the tracers kept through murbhip_init_bodies are not the ones downloaded"
        assert T.same(fresh.state(), bodies)
    assert any(not np.array_equal(F.bits(got[k]), F.bits(before[k])) for k in T.Q), "the tracers did not move"


# ------------------------------------------------------------------------------------------------------- 7. accuracy over a run
# The existing path's figures for the run below, measured on an MI355X with the massless BODY alone (no tracers resident; DESIGN.md
# §4.15 has the table): its distance to the fp64 restatement after 200 steps, and how far re-ordering the fp32 sums alone moves it
# (the spread across the "jsplit" cuts of the bodies' sweep, 1 and 2 at two layout tiles).
BODY_DISTANCE = 2.407750343e-06   # massless body 100 of 513, 200 steps of 1e-4, default cut (one chunk): |q - q_fp64|
BODY_SPREAD = 4.256623047e-07     # |q("jsplit" 1) - q("jsplit" 2)| of the same body ("jsplit" 2: 2.017982615e-06 from fp64)


MASSLESS = 100            # in the first layout tile: the second then holds one massive body, so that the "jsplit" cuts differ
ACC_DT = np.float32(1e-4) # 200 steps are 0.4 crossing times: rounding errors are not yet amplified by the system's chaos


@lru_cache(maxsize=None)
def accuracy_case():
    s = {k: x.copy() for k, x in F.system(513).items()}
    s["m"][MASSLESS] = 0.0                         # the massless body, and the tracer that starts from its state
    tq = np.stack([s[k][MASSLESS:MASSLESS + 1] for k in T.Q])
    tv = np.stack([s[k][MASSLESS:MASSLESS + 1] for k in T.V])
    ref, rq, _ = T.run(s, tq, tv, 200, T.SOFT, ACC_DT)
    return s, tq, tv, np.array([ref[k][MASSLESS] for k in T.Q]), rq[:, 0]


def test_accuracy_over_a_run(gpu):
    """A tracer and a massless body from the same state in the same system (N = 513), 200 fixed steps: both distances to the
    fp64 restatement run from the same start.  The tracer's may exceed the massless body's recorded distance by the body's own
    recorded spread across "jsplit" cuts, which is what re-ordering fp32 sums alone does."""
    s, tq, tv, ref_body, ref_tracer = accuracy_case()
    assert np.abs(ref_body - ref_tracer).max() <= 1e-12, "the two restatements are one"
    with make_sim(gpu, s, (tq, tv)) as sim:
        sim.steps(ACC_DT, 200)
        body = sim.state()
        tr = sim.tracers()
    d_body = float(np.linalg.norm(np.array([body[k][MASSLESS] for k in T.Q], np.float64) - ref_body))
    d_tracer = float(np.linalg.norm(st(tr, T.Q)[:, 0].astype(np.float64) - ref_tracer))
    print(f"distance to the fp64 restatement after 200 steps: massless body {d_body:.3e}, tracer {d_tracer:.3e}; "
          f"recorded {BODY_DISTANCE} + margin {BODY_SPREAD}")
    assert d_tracer <= BODY_DISTANCE + BODY_SPREAD
    assert d_body <= BODY_DISTANCE + BODY_SPREAD, "the massless body itself left the figures recorded for it"


# ------------------------------------------------------------------------------------------------------------------ the plugin
@pytest.mark.parametrize("integrator", [2, 3])
def test_hostsim_carries_tracers(gpu, integrator):
    """HostSim(tracers=) (SimulationNBodyHIP::setTracers / getTracers) and a Simulation driven by hand give equal tracer bits."""
    n, soft, dt = 1024, np.float32(2e8), np.float32(3600.0)
    s = gpu.init_bodies(n, "galaxy")
    rng = np.random.default_rng(9)
    scale = float(np.abs(s["qx"]).max())
    q = (scale * rng.uniform(-1, 1, (3, 21))).astype(np.float32)
    v = np.zeros((3, 21), np.float32)
    with gpu.HostSim(n, "galaxy", soft=soft, dt=dt, integrator=integrator, tracers=(q, v)) as host:
        host.step(2)
        got = host.tracers()
        bodies = host.state()
    with gpu.Simulation(n, soft=soft) as sim:
        sim.set_option("integrator", 2)
        sim.upload(s)
        sim.upload_tracers(q, v)
        for _ in range(2):
            if integrator == 2:
                sim.step(dt)
            else:
                sim.evolve(float(dt), 0.02, 0.01, 0.0, float(dt), 1000000)
        want = sim.tracers()
        mine = sim.state()
    assert T.same(got, want), "the plugin's tracers differ from a Simulation's driven by hand"
    assert all(np.array_equal(F.bits(bodies[k]), F.bits(mine[k])) for k in SKEYS)
    assert any(not np.array_equal(F.bits(got[k]), F.bits(x)) for k, x in zip(T.Q, q)), "the tracers did not move"

"""GPU: read-outs and refused calls never change a later result (include/murbhip.h, "Call orders").

Everything is differential, bit for bit, between two contexts of the same build: `mixed` runs a sequence with its observers and
refused calls, `clean` runs its twin (the body-changing calls alone, read once at the end) and, per observer, the twin plus that
observer alone.  C1: equal end read-outs.  C2: every observer's value equals its solo value.  C3: every refused call returns
its code.  C4 (family K): after a value-changing set of a plan key the results are those of a context that had the key before
its upload.  tests/helpers/call_orders.py has the table, the interpreter and the generators; tests/test_call_orders_host.py
pins them.  The only bound here is test_energy_from_the_force_evaluation's 1e-7 on the fused potential against fp64."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import call_orders as C   # noqa: E402

pytestmark = pytest.mark.gpu

SOFT, DT = np.float32(2e8), np.float32(3600.0)
NEUTRAL = {"profile": 0, "energy_sweep": 0, "evolve_batch": 0}
RAN = {"F": {}, "K": {}, "H": {}}      # sequences run per family and configuration: printed, and compared with the pinned counts


def make(gpu, n, devices):
    return gpu.Simulation(n, soft=SOFT, **({"devices": list(devices)} if devices else {}))


class Pair:
    """The context under test and the one its twins and solo sequences run on.  Every sequence starts from its own upload, so
    the pair serves a whole configuration; what `clean` returns is kept per sequence."""

    def __init__(self, gpu, n, devices, options, ctx):
        self.gpu, self.ctx, self.options = gpu, ctx, dict(options)
        self.mixed, self.clean = make(gpu, n, devices), make(gpu, n, devices)
        self.kept = {}
        self.problems = []

    def close(self):
        self.mixed.close()
        self.clean.close()

    def prepare(self, sim):
        sim.upload(self.ctx["s"])      # closes an open block: every option below may then be set
        sim.set_encounter(0.0)
        for k, v in {"integrator": self.ctx["integrator"], **self.options, **NEUTRAL}.items():
            sim.set_option(k, v)

    def run_clean(self, seq):
        key = tuple(seq)
        if key not in self.kept:
            self.prepare(self.clean)
            self.kept[key] = C.run(self.clean, seq, self.ctx, self.gpu.MurbHipError)
        return self.kept[key]

    def check(self, seq):
        """C1, C2 and C3 of one sequence; problems are collected, the first with the diagnostic."""
        self.prepare(self.mixed)
        rec = C.run(self.mixed, seq, self.ctx, self.gpu.MurbHipError)
        found = []
        tw = self.run_clean(C.twin(seq))
        d = C.differing(rec, tw)
        if d:
            found.append(f"C1: {d} differ from the twin's")
        for pos, alone in C.solo(seq).items():
            at = next(i for i, op in enumerate(alone) if op.kind == "O")
            if rec["values"][pos] != self.run_clean(alone)["values"][at]:
                found.append(f"C2: {pos}:{C.describe(seq[pos])} is not its solo value")
        for pos, (name, want, got) in rec["refused"].items():
            if got != want:
                found.append(f"C3: {pos}:{C.describe(seq[pos])} returned {got}")
        if found:
            if not self.problems and any(f.startswith("C1") for f in found):
                found += C.diagnose(seq, tw, self.run_clean)
            self.problems.append(C.show(seq) + "\n    " + "\n    ".join(found))
        return rec

    def verdict(self, ran, total):
        for problem in self.problems:
            print(problem)
        assert not self.problems, f"{len(self.problems)} of {ran} sequences fail; the first 5:\n" + "\n".join(self.problems[:5])
        assert ran == total, (ran, total)


def assert_info(sim, want):
    for k, v in want.items():
        got = sim.info(k)
        assert (got >= v) if k == "sym_passes" else (got == v), (k, got, v)


def report(family, name, ran):
    RAN[family][name] = RAN[family].get(name, 0) + ran
    print(f"call orders: family {family}, {name}: {ran} sequences ran (so far {RAN[family][name]} of {C.counts()[family][name]})")


# ---------------------------------------------------------------------------------------------------------------- family F
@pytest.mark.parametrize("integrator", C.F_INTEGRATORS)
@pytest.mark.parametrize("name,n,devices,options,info", C.F_CONFIGS, ids=[c[0] for c in C.F_CONFIGS])
def test_force_plan_observers(gpu, name, n, devices, options, info, integrator):
    """Family F: prefix, o1, o2, step, step for every ordered pair of the force plans' observers, under "integrator" 0 and 1."""
    ctx = {"s": gpu.init_bodies(n, "galaxy"), "dt": DT, "integrator": integrator}
    pair = Pair(gpu, n, devices, options, ctx)
    try:
        pair.prepare(pair.mixed)
        pair.mixed.compute_acc()
        pair.mixed.sync()
        assert_info(pair.mixed, info)
        seqs = C.family_f()
        for seq in seqs:
            pair.check(seq)
        report("F", name, len(seqs))
        pair.verdict(len(seqs), C.counts()["F"][name] // len(C.F_INTEGRATORS))
    finally:
        pair.close()


# ---------------------------------------------------------------------------------------------------------------- family K
@pytest.mark.parametrize("name,n,devices,options,info,entries", C.K_CONFIGS, ids=[c[0] for c in C.K_CONFIGS])
def test_plan_key_change_drops_the_remembered_forces(gpu, O, name, n, devices, options, info, entries):
    """Family K (C4): a value-changing set of a plan key between an evaluation and its use.  K-a: upload, compute_acc, set key,
    step, step ends like a context that had the key before its upload; K-b, K-c: the energies after the set equal that
    context's, `==` on the doubles, fused and swept; K-d: the A/B cross-check without a key change; wherever the plan after the set is
    pair-symmetric, the last fused value of K-c also against fp64 within 1e-7 (a potential of the diagonal blocks alone misses it
    by orders).  The plan is asserted before every case and after every set, and that it moved wherever get_info shows it."""
    s = gpu.init_bodies(n, "galaxy")
    ctx = {"s": s, "dt": DT, "integrator": 0}
    pe64 = O.energy_f64(s, SOFT)[1]
    ran = against_fp64 = 0
    moved = {}      # key -> whether any of its listed values changed what get_info shows of the plan
    problems = []
    pair = Pair(gpu, n, devices, {}, ctx)
    for key, value, beside in entries:
        base = {**C.K_DEFAULTS, **options, **beside}
        pair.options = base      # every plan key is in it: what an earlier entry had in force goes back
        fresh = make(gpu, n, devices)
        try:
            for k, v in {"integrator": 0, **base, key: value}.items():
                fresh.set_option(k, v)

            def run_fresh(seq):
                for k, v in NEUTRAL.items():
                    fresh.set_option(k, v)
                return C.run(fresh, seq, ctx, gpu.MurbHipError)

            after = C.k_variant_after(info["variant"], key, value)
            for case, (seq, positions, fresh_seqs) in C.family_k(key, value).items():
                pair.prepare(pair.mixed)      # the key goes back first
                pair.mixed.compute_acc()
                pair.mixed.sync()
                assert_info(pair.mixed, info)
                shown = C.K_VISIBLE.get(key)
                before = pair.mixed.info(shown) if shown else None
                rec = C.run(pair.mixed, seq, ctx, gpu.MurbHipError)
                ran += 1
                assert pair.mixed.info("variant") == after, (key, value, pair.mixed.info("variant"), after)
                if shown and (devices is None or key != "sym_pass_mb"):
                    moved[key] = moved.get(key, False) or pair.mixed.info(shown) != before
                found = []
                if case == "a":
                    d = C.differing(rec, run_fresh(C.K_FRESH_A))
                    if d:
                        found.append(f"{d} differ from the fresh context's")
                for pos, fseq in zip(positions, fresh_seqs):
                    want = run_fresh(fseq)["values"][len(fseq) - 1]
                    if rec["values"][pos] != want:
                        got_pe, want_pe = np.frombuffer(rec["values"][pos][1], "<f8")[0], np.frombuffer(want[1], "<f8")[0]
                        found.append(f"energy at {pos}: potential {got_pe!r}, the fresh context's {want_pe!r} ({(got_pe - want_pe) / want_pe:.3e})")
                if case == "c" and after == 8:      # the plan asserted above, not a condition read from the device
                    got_pe = np.frombuffer(rec["values"][7][1], "<f8")[0]
                    against_fp64 += 1
                    if not abs(got_pe - pe64) <= 1e-7 * abs(pe64):
                        found.append(f"fused potential after the cross-check off fp64 by {(got_pe - pe64) / pe64:.3e}")
                if found:
                    problems.append(f"K-{case} {key}={value}: " + "; ".join(found))
        except BaseException:
            pair.close()
            raise
        finally:
            fresh.close()
    try:
        pair.options = {**C.K_DEFAULTS, **options}
        pair.prepare(pair.mixed)
        rec = C.run(pair.mixed, C.K_D, ctx, gpu.MurbHipError)
        ran += 1
        if rec["values"][2] != rec["values"][6]:
            problems.append("K-d: the fused energy after the sweep is not the one before it")
        report("K", name, ran)
        pair.problems = problems
        pair.verdict(ran, C.counts()["K"][name])
    finally:
        pair.close()
    assert all(moved.values()), f"no listed value of these keys moved the plan: {[k for k, m in moved.items() if not m]}"
    want_fp64 = sum(C.k_variant_after(info["variant"], key, value) == 8 for key, value, _ in entries)
    assert against_fp64 == want_fp64 >= 1, (against_fp64, want_fp64)


# ---------------------------------------------------------------------------------------------------------------- family H
def hermite_ctx(gpu, n, option):
    s = gpu.init_bodies(n, "random")
    rng = np.random.default_rng(7)
    span = float(np.ptp(s["qx"]))
    ctx = {"s": s, "dt": DT, "integrator": 2, "option": option, "T": 8.0 * float(DT), "dt_max": 2.0 ** 17,
           "levels": (np.arange(n) % 4).astype(np.int32), "enc_r": np.float32(1e-3 * span),
           "host_acc": tuple(rng.standard_normal(n).astype(np.float32) * np.float32(1e-6) for _ in range(3)),
           "radii2": rng.uniform(0.0, 2e-3 * span, n).astype(np.float32)}
    if option == "contact":
        ctx["radii"] = rng.uniform(0.0, 1e-3 * span, n).astype(np.float32)
    return ctx


@pytest.mark.parametrize("name,n,option,options", C.H_CONFIGS, ids=[c[0] for c in C.H_CONFIGS])
def test_hermite_observers_and_refusals(gpu, name, n, option, options):
    """Family H: upload, m1, every observer and refused call legal there (in table order, and reversed), m2, for every ordered
    pair of body-changing calls of the Hermite path that may follow each other, the open block's included."""
    ctx = hermite_ctx(gpu, n, option)
    pair = Pair(gpu, n, None, {"nearest": 0, "contact": 0, "potential": 0, **options}, ctx)
    try:
        pair.prepare(pair.mixed)
        assert_info(pair.mixed, C.H_INFO[name])
        seqs = C.family_h(option)
        for seq in seqs:
            rec = pair.check(seq)
            for call, out in rec["raw_outs"]:
                if call in C.BLOCK_OPS:      # individual steps: some block step had fewer than n active bodies
                    assert out["body_steps"] < out["steps"] * n, (C.show(seq), out)
        report("H", name, len(seqs))
        pair.verdict(len(seqs), C.counts()["H"][name])
    finally:
        pair.close()

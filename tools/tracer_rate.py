#!/usr/bin/env python3
"""Cost of carrying massless tracers (include/murbtracer.h): the tracer sweep's kernel span beside the field sweep's span for the
same points, N and chunk count, and the Hermite step with and without tracers.  One process after murbhip_warmup, the legs
alternating, three rounds, in the manner of tools/field_rate.py.

    python tools/tracer_rate.py [--sizes 30000,200000] [--counts 4096,0] [--reps 5] [--rounds 3] [--out profiles/tracer_sweep.txt]

Per leg: the sweep launches' HIP-event spans summed per step or per call ("profile" 2: span_tracer_* of murbhip_steps, where the
sweep runs back to back with the bodies' own, and of murbtracer_compute after a fresh upload, which has the duty cycle of a
read-out; span_field_* of murbfield_at at the tracers' places and velocities), and the wall time of a fixed Hermite step (enqueue `reps`
steps, wait, divide) with the tracers resident and after murbtracer_clear.  pairs/s = count x N / time.  count 0 means N."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

DT = 3600.0


def span_tracer(sim, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples
    sim.steps(DT, reps)
    sim.sync()
    return sim.info("span_tracer_ms_avg") * sim.info("span_tracer_count") / reps


def span_tracer_alone(sim, q, v, reps):
    """murbtracer_compute after a fresh upload: the sweep with the duty cycle of a murbfield_at call (upload, launches, wait)."""
    sim.set_option("profile", 2)
    for _ in range(reps):
        sim.upload_tracers(q, v)
        sim.compute_tracers()
        sim.sync()
    return sim.info("span_tracer_ms_avg") * sim.info("span_tracer_count") / reps


def span_field(sim, q, v, reps):
    sim.set_option("profile", 2)
    for _ in range(reps):
        sim.field_at(q, v)
    return sim.info("span_field_ms_avg") * sim.info("span_field_count") / reps


def step_wall(sim, reps):
    sim.set_option("profile", 0)
    sim.sync()
    t0 = time.perf_counter()
    sim.steps(DT, reps)
    sim.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--counts", default="4096,0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; sweep = HIP-event spans of the sweep launches, "
        "step = wall time of an enqueued fixed Hermite step")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n) as sim:
            sim.set_option("integrator", 2)
            sim.upload(s)
            sim.warmup(100.0)
            cus = int(sim.info("cu_count"))
            sim.set_field_option("field_chunks", 0)
            sim.set_tracer_option("tracer_chunks", 0)
            chunks = sim.tracer_option("tracer_chunks")
            assert chunks == sim.field_option("field_chunks")
            say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks, batch {sim.tracer_option('tracer_batch')})")
            for m in (int(c) or n for c in args.counts.split(",")):
                pick = rng.choice(n, m, replace=m > n)
                q = np.stack([s[k][pick] * np.float32(1.001) for k in ("qx", "qy", "qz")])     # beside the bodies, not on them
                v = np.stack([s[k][pick] for k in ("vx", "vy", "vz")])
                got = {"tracer": [], "alone": [], "field": [], "with": [], "without": []}
                for _ in range(args.rounds):
                    sim.upload_tracers(q, v)
                    got["tracer"].append(span_tracer(sim, args.reps))
                    got["with"].append(step_wall(sim, args.reps))
                    sim.clear_tracers()
                    got["without"].append(step_wall(sim, args.reps))
                    got["field"].append(span_field(sim, q, v, args.reps))
                    got["alone"].append(span_tracer_alone(sim, q, v, args.reps))
                    sim.clear_tracers()
                sim.set_option("profile", 0)
                pairs = float(m) * float(n)
                for name, what in (("tracer", "tracer sweep, per step        "), ("alone", "tracer sweep, murbtracer_compute"),
                                   ("field", "field sweep, same points      ")):
                    a = sum(got[name]) / len(got[name])
                    say(f"  M = {m:7d}  {what}: {a:9.4f} ms  {pairs / a * 1e3:.3e} pairs/s   rounds: " + ", ".join(f"{t:.4f}" for t in got[name]))
                for name, what in (("with", "Hermite step with the tracers "), ("without", "Hermite step without          ")):
                    a = sum(got[name]) / len(got[name])
                    say(f"  M = {m:7d}  {what}: {a:9.4f} ms                          rounds: " + ", ".join(f"{t:.4f}" for t in got[name]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

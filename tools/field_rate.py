#!/usr/bin/env python3
"""Cost of the field read-out: murbfield_of at `count` of the N bodies, beside the Hermite sweep with the per-body potential
(murb_force_jerk_pot_kernel: the same arithmetic, the same occupancy) as the yardstick for count = N.  One process after
murbhip_warmup, the legs alternating, three rounds.

    python tools/field_rate.py [--sizes 30000,200000] [--counts 16,4096,0] [--chunks 0,16,64,256] [--reps 5] [--rounds 3]
                               [--out profiles/field_sweep.txt]

Two times per leg: the sweep kernel's HIP-event span ("profile" 2, span_field_ms_avg x span_field_count: the call's launches summed) and
the wall time of the whole synchronous call (upload of the list, pack, sweep, row sum, download).  pairs/s = count x N / time.
count 0 means N.  --chunks: values of "field_chunks" to try (0 = the default rule)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402


def timed_field(sim, bodies, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the field sweep's own span kind
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.field_of(bodies)
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info("span_field_ms_avg") * sim.info("span_field_count") / reps, wall


def timed_sweep(sim, reps):
    sim.set_option("profile", 1)
    sim.steps(3600.0, reps)
    sim.sync()
    return sim.info("force_ms_avg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--counts", default="16,4096,0")
    ap.add_argument("--chunks", default="0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event span of the sweep, call = wall time of the synchronous call")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n) as sim:
            sim.upload(s)
            sim.set_option("integrator", 2)
            sim.set_option("potential", 1)
            sim.warmup(100.0)
            legs = [(int(c) or n, int(k)) for k in args.chunks.split(",") for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c, _ in legs}
            got = {leg: [] for leg in legs}
            sweep = []
            for _ in range(args.rounds):
                sweep.append(timed_sweep(sim, args.reps))
                for c, k in legs:
                    sim.set_field_option("field_chunks", k)
                    got[(c, k)].append(timed_field(sim, lists[c], args.reps))
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
            chunks_of = {}
            for _, k in legs:
                sim.set_field_option("field_chunks", k)
                chunks_of[k] = sim.field_option("field_chunks")
        a = sum(sweep) / len(sweep)
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles)")
        say(f"  sweep with the potential, all bodies       : {a:9.4f} ms  {float(n) * n / a * 1e3:.3e} pairs/s   rounds: "
            + ", ".join(f"{t:.4f}" for t in sweep))
        for (c, k), r in got.items():
            kern, wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
            pairs = float(c) * float(n)
            say(f"  field_of count {c:7d}, {chunks_of[k]:4d} chunks (option {k:3d}): kernel {kern:9.4f} ms  {pairs / kern * 1e3:.3e} pairs/s"
                f"   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

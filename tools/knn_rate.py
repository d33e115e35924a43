#!/usr/bin/env python3
"""Cost of the neighbour read-out: murbknn_of at `count` of the N bodies with k = 6 and k = 32 beside murbfield_of at the same
bodies, in the same process and build.  One process after murbhip_warmup, the legs alternating, three rounds of five calls.

    python tools/knn_rate.py [--sizes 30000,200000] [--counts 4096,0] [--ks 6,32] [--reps 5] [--rounds 3] [--out profiles/knn_sweep.txt]

Two times per leg: the sweep kernel's HIP-event span ("profile" 2, span_knn_ms_avg x span_knn_count, span_field_* for the field
leg: the call's launches summed) and the wall time of the whole synchronous call (upload of the list, pack, sweep, merge,
download).  pairs/s = count x N / time.  count 0 means N.  All legs run under the same "field_chunks" and "field_batch" (the
defaults).  At the largest size also the wall time of murbdensity_centre (k = 6) beside one tracked iteration (murbhip_energy
and a step)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402


def timed(sim, call, kind, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info(f"span_{kind}_ms_avg") * sim.info(f"span_{kind}_count") / reps, wall


def wall_ms(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--counts", default="4096,0")
    ap.add_argument("--ks", default="6,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    ks = [int(x) for x in args.ks.split(",")]
    sizes = [int(x) for x in args.sizes.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event span of the sweep, call = wall time of the synchronous call")
    for n in sizes:
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            legs = ["field"] + [f"knn{k}" for k in ks]
            got = {(c, leg): [] for c in counts for leg in legs}
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "field")].append(timed(sim, lambda: sim.field_of(lists[c]), "field", args.reps))
                    for k in ks:
                        got[(c, f"knn{k}")].append(timed(sim, lambda: sim.knn_of(lists[c], k=k), "knn", args.reps))
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
            chunks = sim.field_option("field_chunks")
            extra = None
            if n == max(sizes):
                def tracked():
                    sim.energy()
                    sim.step(3600.0)
                    sim.sync()
                extra = [(wall_ms(lambda: sim.density_centre(6), args.reps), wall_ms(tracked, args.reps)) for _ in range(args.rounds)]
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks)")
        for c in counts:
            kern = {}
            for leg in legs:
                r = got[(c, leg)]
                kern[leg], wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
                pairs = float(c) * float(n)
                say(f"  {leg + '_of':8s} count {c:7d}: kernel {kern[leg]:9.4f} ms  {pairs / kern[leg] * 1e3:.3e} pairs/s"
                    f"   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
            for k in ks:
                say(f"  knn (k = {k}) / field kernel time at count {c}: {kern[f'knn{k}'] / kern['field']:.3f}")
        if extra:
            say("  density_centre(6) wall ms, rounds: " + ", ".join(f"{a:.3f}" for a, _ in extra)
                + "   one tracked iteration (energy + step) wall ms: " + ", ".join(f"{b:.3f}" for _, b in extra))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

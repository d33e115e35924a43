#!/usr/bin/env python3
"""Cost of the tidal read-out: murbtidal_of at `count` of the N bodies beside murbfield_of at the same bodies, in the same
process and build.  One process after murbhip_warmup, the two legs alternating, three rounds of five calls.

    python tools/tidal_rate.py [--sizes 30000,200000] [--counts 16,4096,0] [--reps 5] [--rounds 3] [--out profiles/tidal_sweep.txt]

Two times per leg: the sweep kernel's HIP-event span ("profile" 2, span_tidal_ms_avg x span_tidal_count, span_field_* for the
field leg: the call's launches summed) and the wall time of the whole synchronous call (upload of the list, pack, sweep, row
sum, download).  pairs/s = count x N / time.  count 0 means N.  Both legs run under the same "field_chunks" and "field_batch"
(the defaults)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402


def timed(sim, call, kind, bodies, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        call(bodies)
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info(f"span_{kind}_ms_avg") * sim.info(f"span_{kind}_count") / reps, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--counts", default="16,4096,0")
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
            sim.warmup(100.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            got = {(c, kind): [] for c in counts for kind in ("field", "tidal")}
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "field")].append(timed(sim, sim.field_of, "field", lists[c], args.reps))
                    got[(c, "tidal")].append(timed(sim, sim.tidal_of, "tidal", lists[c], args.reps))
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
            chunks = sim.field_option("field_chunks")
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks)")
        for c in counts:
            kern = {}
            for kind in ("field", "tidal"):
                r = got[(c, kind)]
                kern[kind], wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
                pairs = float(c) * float(n)
                say(f"  {kind}_of count {c:7d}: kernel {kern[kind]:9.4f} ms  {pairs / kern[kind] * 1e3:.3e} pairs/s"
                    f"   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
            say(f"  tidal / field kernel time at count {c}: {kern['tidal'] / kern['field']:.3f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

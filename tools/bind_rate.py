#!/usr/bin/env python3
"""Cost of the bound-pair read-out: murbbind_of at `count` of the N bodies beside murbfield_of and murbknn_of (k = 6) at the same
bodies, and murbbind_pairs (the sweep over all bodies twice, the elements, the census, the compaction), in the same process
and build.  One process after murbhip_warmup, the legs alternating, three rounds of five calls.

    python tools/bind_rate.py [--sizes 30000,200000] [--counts 4096,0] [--reps 5] [--rounds 3] [--out profiles/bind_sweep.txt]

Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kind bind, field, knn) and the wall time of the whole synchronous call.  pairs/s = count x N / time.  count 0 means N.
All legs run under the same "field_chunks" and "field_batch" (the defaults).  The `binaries` leg is Simulation.binaries(): the
count-only call, then the sized one where there are pairs, each a sweep over all N bodies."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

SOFT = 2e8


def timed(sim, call, kind, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info(f"span_{kind}_ms_avg") * sim.info(f"span_{kind}_count") / reps, wall


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

    sizes = [int(x) for x in args.sizes.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    for n in sizes:
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            legs = ["field", "knn6", "bind"]
            got = {(c, leg): [] for c in counts for leg in legs}
            pairs_leg = []
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "field")].append(timed(sim, lambda: sim.field_of(lists[c]), "field", args.reps))
                    got[(c, "knn6")].append(timed(sim, lambda: sim.knn_of(lists[c], k=6), "knn", args.reps))
                    got[(c, "bind")].append(timed(sim, lambda: sim.bound_partner_of(lists[c]), "bind", args.reps))
                pairs_leg.append(timed(sim, sim.binaries, "bind", args.reps))
            census = sim.binaries()["census"]
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
            chunks = sim.field_option("field_chunks")
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks)")
        for c in counts:
            kern = {}
            for leg in legs:
                r = got[(c, leg)]
                kern[leg], wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
                pairs = float(c) * float(n)
                say(f"  {leg:8s} count {c:7d}: kernel {kern[leg]:9.4f} ms  {pairs / kern[leg] * 1e3:.3e} pairs/s"
                    f"   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
            say(f"  bind / field kernel time at count {c}: {kern['bind'] / kern['field']:.3f};  bind / knn (k = 6): {kern['bind'] / kern['knn6']:.3f}")
        k, w = sum(x for x, _ in pairs_leg) / len(pairs_leg), sum(y for _, y in pairs_leg) / len(pairs_leg)
        say(f"  binaries(): kernel {k:9.4f} ms   call {w:9.4f} ms   census: {census['pairs']} bound pairs, {census['mutual_pairs']} mutual, "
            f"{census['bound_bodies']} bodies whose partner has h < 0")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the neighbours-within-a-radius read-out: murbnbr_of at `count` of the N bodies, count-only and with lists, beside
murbfield_of and murbknn_of (k = 6) at the same bodies, in the same process and build.  One process after murbhip_warmup, the
legs alternating, three rounds of five calls.

    python tools/nbr_rate.py [--sizes 30000,200000] [--counts 4096,0] [--means 6,64] [--reps 5] [--rounds 3] [--out profiles/nbr_sweep.txt]

The radius is set from the bodies: for a mean count of about 6 the median distance of the 6th neighbour (murbknn_of on 4 096
bodies), for about 64 the median distance of the 32nd times 2^(1/3), each then scaled four times by the cube root of wanted
over counted on those 4 096 bodies; the mean count a leg really had is printed with it.
Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kind nbr, field, knn) and the wall time of the whole synchronous call.  The `count` leg is the count-only call (one count
sweep per launch).  The `lists` leg is Simulation.neighbours_of with lists: the count-only call, then the sized call, which
counts again and fills: two count sweeps and the fill sweeps; `fill` = lists - 2 x count is the fill sweep alone.  pairs/s =
count x N / time.  count 0 means N.  All legs run under the same "field_chunks" and "field_batch" (the defaults)."""
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
    ap.add_argument("--means", default="6,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    means = [int(x) for x in args.means.split(",")]
    sizes = [int(x) for x in args.sizes.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    for n in sizes:
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            soft2 = float(np.float32(SOFT) * np.float32(SOFT))
            sample = np.sort(rng.choice(n, min(n, 4096), replace=False)).astype(np.int32)
            _, r2 = sim.knn_of(sample, k=32)
            d = np.sqrt(np.maximum(np.median(r2.astype(np.float64), axis=0) - soft2, 0.0))
            radius = {m: float(d[m - 1]) if m <= 32 else float(d[31] * (m / 32.0) ** (1.0 / 3.0)) for m in means}
            for m in means:      # the bodies are clustered, so the median distance overshoots the MEAN count: scale h to it
                for _ in range(4):
                    have = float(sim.neighbours_of(sample, h=radius[m], lists=False)[0][-1]) / len(sample)
                    radius[m] *= (m / max(have, 1e-3)) ** (1.0 / 3.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            legs = ["field", "knn6"] + [f"{what}{m}" for m in means for what in ("count", "lists")]
            got = {(c, leg): [] for c in counts for leg in legs}
            mean = {}
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "field")].append(timed(sim, lambda: sim.field_of(lists[c]), "field", args.reps))
                    got[(c, "knn6")].append(timed(sim, lambda: sim.knn_of(lists[c], k=6), "knn", args.reps))
                    for m in means:
                        got[(c, f"count{m}")].append(timed(sim, lambda: sim.neighbours_of(lists[c], h=radius[m], lists=False), "nbr", args.reps))
                        got[(c, f"lists{m}")].append(timed(sim, lambda: sim.neighbours_of(lists[c], h=radius[m]), "nbr", args.reps))
                        mean[(c, m)] = float(sim.neighbours_of(lists[c], h=radius[m], lists=False)[0][-1]) / c
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
            chunks = sim.field_option("field_chunks")
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks)   radii: " + ", ".join(f"about {m}: h = {radius[m]:.4e}" for m in means))
        for c in counts:
            kern = {}
            for leg in legs:
                r = got[(c, leg)]
                kern[leg], wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
                pairs = float(c) * float(n)
                say(f"  {leg:8s} count {c:7d}: kernel {kern[leg]:9.4f} ms  {pairs / kern[leg] * 1e3:.3e} pairs/s"
                    f"   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
            say(f"  knn (k = 6) / field kernel time at count {c}: {kern['knn6'] / kern['field']:.3f}")
            for m in means:
                fill = kern[f"lists{m}"] - 2.0 * kern[f"count{m}"]
                say(f"  mean count {mean[(c, m)]:8.2f} at count {c}: count sweep / field {kern[f'count{m}'] / kern['field']:.3f};"
                    f" fill sweep {fill:.4f} ms, / field {fill / kern['field']:.3f}, / count sweep {fill / kern[f'count{m}']:.3f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

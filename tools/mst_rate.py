#!/usr/bin/env python3
"""Cost of the spanning-tree read-out: murbforeign_of (label[i] = i) at `count` of the N bodies beside murbknn_of (k = 1) and a
count-only murbnbr_of at the same bodies, then one murbmst_of call on the galaxy and on a Plummer sphere, and the mass
segregation ratio of 50 bodies against 50 random sets, in the same process and build.  One process after murbhip_warmup, the legs
alternating, three rounds of five calls.

    python tools/mst_rate.py [--sizes 200000] [--counts 4096,0] [--reps 5] [--rounds 3] [--out profiles/mst_sweep.txt]

Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kind mst, knn, nbr) and the wall time of the whole synchronous call.  pairs/s = count x N / time.  count 0 means N.
All legs run under the same "field_chunks" and "field_batch" (the defaults)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import murbhip      # noqa: E402
import knn_ref      # noqa: E402

SOFT = 2e8


def timed(sim, call, kind, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        out = call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info(f"span_{kind}_ms_avg") * sim.info(f"span_{kind}_count") / reps, wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000")
    ap.add_argument("--counts", default="4096,0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def tree_legs(sim, what, n):
        sim.warmup(100.0)
        sim.spanning_tree()
        kernel, wall, t = timed(sim, sim.spanning_tree, "mst", 1)
        say(f"  spanning_tree(), {what}: {t['rounds']} rounds, {t['edges']} edges, {t['components']} component(s), mean length "
            f"{t['mean_length']:.4e}: sweeps {kernel:9.4f} ms ({kernel / wall:.2f} of the call)   call {wall:9.4f} ms")
        sim.mass_segregation_ratio(50, sets=50)
        kernel, wall, r = timed(sim, lambda: sim.mass_segregation_ratio(50, sets=50), "mst", 1)
        launches = sim.info("span_mst_count")
        say(f"  mass_segregation_ratio(50, sets=50), {what}: ratio {r['ratio']:.3f} +- {r['sigma']:.3f}: sweeps {kernel:9.4f} ms in "
            f"{launches:.0f} launches ({kernel / wall:.3f} of the call)   call {wall:9.4f} ms")
        sim.set_option("profile", 0)

    sizes = [int(x) for x in args.sizes.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    for n in sizes:
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        own = np.arange(n, dtype=np.int32)
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            d = np.sqrt(sim.knn_of(lists[counts[0]], k=1)[1].astype(np.float64))
            h = float(np.median(d))   # the count sweep's radius: the median nearest-neighbour distance
            legs = ["knn", "nbr", "mst"]
            got = {(c, leg): [] for c in counts for leg in legs}
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "knn")].append(timed(sim, lambda: sim.knn_of(lists[c], k=1), "knn", args.reps)[:2])
                    got[(c, "nbr")].append(timed(sim, lambda: sim.neighbours_of(lists[c], h=h, lists=False), "nbr", args.reps)[:2])
                    got[(c, "mst")].append(timed(sim, lambda: sim.foreign_nearest(own, lists[c]), "mst", args.reps)[:2])
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
                say(f"  mst / knn kernel time at count {c}: {kern['mst'] / kern['knn']:.3f};  mst / nbr (count only): {kern['mst'] / kern['nbr']:.3f}")
            tree_legs(sim, "galaxy", n)
        p, soft = knn_ref.plummer(n)
        with murbhip.Simulation(n, soft=float(soft), g=1.0) as sim:
            sim.upload(p)
            tree_legs(sim, "Plummer sphere", n)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the pair-separation read-out: murbsep_of of all N bodies, sum-only, with a histogram at sub = 4 (and at sub = 0 and
sub = 6 over about the same range), and with the worst histogram for the LDS integer adds (sub = 0, one bin, every pair in one
counter), beside the count-only murbnbr_of of the same bodies as the yardstick, in the same process and build.  One process
after murbhip_warmup, the legs alternating, three rounds.

    python tools/sep_rate.py [--sizes 4096,200000] [--reps 3] [--rounds 3] [--out profiles/sep_sweep.txt]

Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kind sep, nbr) and the wall time of the whole synchronous call.  pairs/s = N x N / time.  All legs run under the same
"field_chunks" and "field_batch" (the defaults)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip      # noqa: E402

SOFT = 2e8
SPREAD = (30, 4, 512)     # the galaxy's d2 lies around 2^55: 32 octaves of 16 bins hold it
COARSE = (30, 0, 32)      # the same range, one bin per octave
FINE = (45, 6, 1022)      # 64 bins per octave from 2^45 to just below 2^61
WORST = (0, 0, 1)         # every pair lies above 2 = 2^1: one counter takes them all


def timed(sim, call, kind, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    return sim.info(f"span_{kind}_ms_avg") * sim.info(f"span_{kind}_count") / reps, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,200000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    say(f"# histogram legs, (lo_exp, sub, bins): sub = 4 is {SPREAD}, sub = 0 {COARSE}, sub = 6 {FINE}; worst is {WORST}, every pair in one counter")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            legs = {"nbr count": (lambda: sim.neighbours_of(h=0.1 * SOFT, lists=False), "nbr"),
                    "sep sum": (lambda: sim.separation_of(), "sep"),
                    "sep sub=4": (lambda: sim.separation_of(bins=SPREAD), "sep"),
                    "sep sub=0": (lambda: sim.separation_of(bins=COARSE), "sep"),
                    "sep sub=6": (lambda: sim.separation_of(bins=FINE), "sep"),
                    "sep worst": (lambda: sim.separation_of(bins=WORST), "sep")}
            got = {leg: [] for leg in legs}
            for _ in range(args.rounds):
                for leg, (call, kind) in legs.items():
                    got[leg].append(timed(sim, call, kind, args.reps))
            sim.set_option("profile", 0)
            _, hist, out4 = sim.separation_of(bins=SPREAD)
            _, _, worst4 = sim.separation_of(bins=WORST)
            fullest = {name: int(sim.separation_of(bins=b)[1].max()) for name, b in (("sub=0", COARSE), ("sub=6", FINE))}
            mean = sim.mean_separation()
            cus, chunks = int(sim.info("cu_count")), sim.field_option("field_chunks")
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks); mean separation {mean:.6e}")
        say(f"  sub = 4: {out4}, bins in use {int((hist > 0).sum())}, fullest bin {int(hist.max())};  fullest bin at {fullest};  worst: {worst4}")
        kern = {}
        pairs = float(n) * float(n)
        for leg in legs:
            r = got[leg]
            kern[leg], wall = sum(x for x, _ in r) / len(r), sum(y for _, y in r) / len(r)
            say(f"  {leg:10s}: kernel {kern[leg]:9.4f} ms  {pairs / kern[leg] * 1e3:.3e} pairs/s   call {wall:9.4f} ms  {pairs / wall * 1e3:.3e} pairs/s"
                "   kernel rounds: " + ", ".join(f"{x:.4f}" for x, _ in r))
        say(f"  kernel time over the count-only neighbour sweep: sum {kern['sep sum'] / kern['nbr count']:.3f}, "
            f"sub=4 {kern['sep sub=4'] / kern['nbr count']:.3f}, sub=0 {kern['sep sub=0'] / kern['nbr count']:.3f}, "
            f"sub=6 {kern['sep sub=6'] / kern['nbr count']:.3f}, worst {kern['sep worst'] / kern['nbr count']:.3f};  "
            f"worst over sub=4 {kern['sep worst'] / kern['sep sub=4']:.3f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

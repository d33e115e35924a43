#!/usr/bin/env python3
"""Cost of the listed-source read-out: murbsplit_of of all N bodies (the neighbour lists produced and consumed on the device) at
radii that give a mean list length of about 32 and about 128, beside murbfield_of of all bodies (the full sweep) and murbnbr_of
with lists at the same radii, in the same process and build.  One process after murbhip_warmup, the legs alternating, three
rounds.

    python tools/list_rate.py [--sizes 4096,200000] [--means 32,128] [--reps 3] [--rounds 3] [--out profiles/list_sweep.txt]

Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kinds field, nbr, list) and the wall time of the whole synchronous call.  The list sweep gathers per entry one 4-byte
index and two 16-byte records of one 32-byte line: entries/s x 36 B is the gather rate it implies."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

SOFT = 2e8
ENTRY_BYTES = 36   # a 4-byte index and a 32-byte line of records


def timed(sim, call, kinds, reps):
    sim.set_option("profile", 2)     # drains the device and clears the samples; level 2 records the read-outs' own span kinds
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    return {k: sim.info(f"span_{k}_ms_avg") * sim.info(f"span_{k}_count") / reps for k in kinds}, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,200000")
    ap.add_argument("--means", default="32,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    means = [int(x) for x in args.means.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            soft2 = float(np.float32(SOFT) * np.float32(SOFT))
            sample = np.sort(rng.choice(n, min(n, 4096), replace=False)).astype(np.int32)
            _, r2 = sim.knn_of(sample, k=32)
            d = np.sqrt(np.maximum(np.median(r2.astype(np.float64), axis=0) - soft2, 0.0))
            radius = {m: float(d[31] * (m / 32.0) ** (1.0 / 3.0)) for m in means}
            for m in means:      # the bodies are clustered, so the median distance overshoots the MEAN count: scale h to it
                for _ in range(5):
                    have = float(sim.neighbours_of(sample, h=radius[m], lists=False)[0][-1]) / len(sample)
                    radius[m] *= (m / max(have, 1e-3)) ** (1.0 / 3.0)
            legs = {"field": (lambda: sim.field_of(np.arange(n, dtype=np.int32)), ("field",))}
            for m in means:
                legs[f"lists{m}"] = (lambda m=m: sim.neighbours_of(h=radius[m]), ("nbr",))
                legs[f"split{m}"] = (lambda m=m: sim.irregular_field_of(h=radius[m]), ("nbr", "list"))
            got = {leg: [] for leg in legs}
            for _ in range(args.rounds):
                for leg, (call, kinds) in legs.items():
                    got[leg].append(timed(sim, call, kinds, args.reps))
            sim.set_option("profile", 0)
            length = {m: sim.irregular_field_of(h=radius[m])[0].astype(np.int64) for m in means}
            cus, chunks = int(sim.info("cu_count")), sim.field_option("field_chunks")
        say(f"N = {n}  ({cus} CUs, {(n + 511) // 512} tiles, {chunks} chunks)   radii: " + ", ".join(f"about {m}: h = {radius[m]:.4e}" for m in means))
        kern, wall = {}, {}
        for leg, (_, kinds) in legs.items():
            r = got[leg]
            for k in kinds:
                kern[leg, k] = sum(x[k] for x, _ in r) / len(r)
            wall[leg] = sum(y for _, y in r) / len(r)
            say(f"  {leg:9s}: " + "  ".join(f"{k} kernel {kern[leg, k]:9.4f} ms (rounds " + ", ".join(f"{x[k]:.4f}" for x, _ in r) + ")" for k in kinds)
                + f"   call {wall[leg]:9.4f} ms")
        for m in means:
            entries = int(length[m].sum())
            sweep, nbr = kern[f"split{m}", "list"], kern[f"split{m}", "nbr"]
            rate = entries / sweep * 1e3
            say(f"  mean list length {entries / n:8.2f} (longest {int(length[m].max())}, empty {int((length[m] == 0).sum())}): list sweep {sweep:.4f} ms, "
                f"{rate:.3e} entries/s, x {ENTRY_BYTES} B = {rate * ENTRY_BYTES / 1e12:.3f} TB/s gathered")
            say(f"      list sweep / murbsplit_of kernels {sweep / (sweep + nbr):.3f}; murbsplit_of kernels {sweep + nbr:.4f} ms = {(sweep + nbr) / kern['field', 'field']:.3f} of the full sweep, "
                f"the list sweep alone {sweep / kern['field', 'field']:.4f} of it; calls: split {wall[f'split{m}']:.3f} ms, lists to the host {wall[f'lists{m}']:.3f} ms, "
                f"field {wall['field']:.3f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of option "potential": the Hermite integrator's acceleration + jerk sweep with and without the per-body potential,
timed with HIP events ("profile" 1, force_ms_avg) in one process after murbhip_warmup, the two alternating A B A B.

    python tools/potential_rate.py [--sizes 30000,200000] [--reps 10] [--rounds 3] [--out profiles/potential_sweep.txt]

Prints, per size: ms per sweep and pairs per second (N^2 / time) of both forms, every round's figures, and the ratio
potential 1 / potential 0.  --out: the same lines into a file as well."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402


def timed(sim, reps, dt):
    sim.set_option("profile", 1)     # drains the device and clears the samples
    sim.steps(dt, reps)
    sim.sync()
    return sim.info("force_ms_avg"), int(sim.info("force_launches"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; times are HIP-event spans of single launches")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        with murbhip.Simulation(n) as sim:
            sim.upload(s)
            sim.set_option("integrator", 2)
            sim.warmup(100.0)
            plain, pot = [], []
            for _ in range(args.rounds):
                sim.set_option("potential", 0)
                plain.append(timed(sim, args.reps, 3600.0))
                sim.set_option("potential", 1)
                pot.append(timed(sim, args.reps, 3600.0))
            sim.set_option("profile", 0)
            cus, parts = int(sim.info("cu_count")), int(sim.info("hermite_parts"))
        a = sum(t for t, _ in plain) / len(plain)
        b = sum(t for t, _ in pot) / len(pot)
        pairs = float(n) * float(n)
        say(f"N = {n}  ({cus} CUs, {parts} j chunks)")
        say(f"  acceleration + jerk sweep         : {a:9.4f} ms per sweep  {pairs / a * 1e3:.3e} pairs/s   rounds: "
            + ", ".join(f"{t:.4f} ms x {k}" for t, k in plain))
        say(f"  sweep with the potential          : {b:9.4f} ms per sweep  {pairs / b * 1e3:.3e} pairs/s   rounds: "
            + ", ".join(f"{t:.4f} ms x {k}" for t, k in pot))
        say(f"  ratio potential 1 / potential 0   : {b / a:.3f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of the Hermite integrator's acceleration + jerk sweep against the one-sided force kernel ("variant" 1), timed
with HIP events ("profile" 1, force_ms_avg) in the same process after murbhip_warmup, alternating A B A B.

    python tools/hermite_rate.py [--sizes 30000,200000] [--reps 10] [--rounds 2] [--nearest] [--contact]

Prints, per size: ms per sweep, pairs per second (N^2 / time) and the ratio of the two kernels.  --nearest: a third leg in
every round, the sweep with option "nearest" 1 (the nearest-neighbour kernel), and its ratio to the plain sweep.  --contact:
likewise a leg with option "contact" 1 (the contact kernel) and the scheme's own radii."""
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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nearest", action="store_true", help='also time the sweep with option "nearest" 1')
    ap.add_argument("--contact", action="store_true", help='also time the sweep with option "contact" 1')
    args = ap.parse_args()
    print(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; times are HIP-event spans of single launches")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        with murbhip.Simulation(n) as sim:
            sim.upload(s)
            sim.set_option("fuse_integrate", 0)   # the yardstick's span is the force launch alone, as the sweep's is
            sim.warmup(100.0)
            if args.contact:
                sim.upload_radii(s["r"])
            one, herm, near, cont = [], [], [], []
            for _ in range(args.rounds):
                sim.set_option("integrator", 0)
                sim.set_option("variant", 1)
                one.append(timed(sim, args.reps, 3600.0))
                sim.set_option("variant", 0)
                sim.set_option("integrator", 2)
                herm.append(timed(sim, args.reps, 3600.0))
                if args.nearest:
                    sim.set_option("nearest", 1)
                    near.append(timed(sim, args.reps, 3600.0))
                    sim.set_option("nearest", 0)
                if args.contact:
                    sim.set_option("contact", 1)
                    cont.append(timed(sim, args.reps, 3600.0))
                    sim.set_option("contact", 0)
            sim.set_option("profile", 0)
            cus = int(sim.info("cu_count"))
        a = sum(t for t, _ in one) / len(one)
        b = sum(t for t, _ in herm) / len(herm)
        pairs = float(n) * float(n)
        print(f"N = {n}  ({cus} CUs)")
        print(f"  one-sided force kernel (variant 1): {a:9.4f} ms per sweep  {pairs / a * 1e3:.3e} pairs/s   rounds: "
              + ", ".join(f"{t:.4f} ms x {k}" for t, k in one))
        print(f"  acceleration + jerk sweep         : {b:9.4f} ms per sweep  {pairs / b * 1e3:.3e} pairs/s   rounds: "
              + ", ".join(f"{t:.4f} ms x {k}" for t, k in herm))
        print(f"  ratio sweep / force kernel        : {b / a:.2f}")
        if near:
            c = sum(t for t, _ in near) / len(near)
            print(f"  sweep with nearest neighbours     : {c:9.4f} ms per sweep  {pairs / c * 1e3:.3e} pairs/s   rounds: "
                  + ", ".join(f"{t:.4f} ms x {k}" for t, k in near))
            print(f"  ratio nearest 1 / nearest 0       : {c / b:.3f}")
        if cont:
            c = sum(t for t, _ in cont) / len(cont)
            print(f"  sweep with contacts by radii      : {c:9.4f} ms per sweep  {pairs / c * 1e3:.3e} pairs/s   rounds: "
                  + ", ".join(f"{t:.4f} ms x {k}" for t, k in cont))
            print(f"  ratio contact 1 / contact 0       : {c / b:.3f}")


if __name__ == "__main__":
    main()

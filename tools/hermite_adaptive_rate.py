#!/usr/bin/env python3
"""What the device-side step control of murbhip_evolve costs: K Hermite steps of a fixed size through
(a) murbhip_steps(dt, K) ("integrator" 2: three launches a step, dt a launch argument) and
(b) murbhip_evolve pinned to the same dt (dt_min = dt_max = dt, duration = K dt: four launches a step, dt and the done flag
    read from the control block, the criterion evaluated in the corrector, one read-back per batch of 64 steps),
host clock around work that ends in a device sync, same process, same state, alternating a b a b after murbhip_warmup.
Also the time of a batch's no-op tail: one step with "evolve_batch" 64 (63 steps find the done flag set) against
"evolve_batch" 1.

    python tools/hermite_adaptive_rate.py [--sizes 1024,30000,200000] [--rounds 5] [--seconds 0.4]

Prints per size the per-step times of every round, their medians and the ratio b / a."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

DT = 3600.0


def fixed(sim, k):
    t0 = time.perf_counter()
    sim.steps(DT, k)
    sim.sync()
    return (time.perf_counter() - t0) / k


def pinned(sim, k):
    t0 = time.perf_counter()
    out = sim.evolve(k * DT, dt_min=DT, dt_max=DT)     # returns synchronised
    t = time.perf_counter() - t0
    assert out["steps"] == k, out
    return t / k


def one_step(sim, batch):
    sim.set_option("evolve_batch", batch)
    t0 = time.perf_counter()
    out = sim.evolve(DT, dt_min=DT, dt_max=DT)
    t = time.perf_counter() - t0
    sim.set_option("evolve_batch", 0)
    assert out["steps"] == 1, out
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,30000,200000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.4, help="length of one timed window (sets K per size)")
    args = ap.parse_args()
    assert murbhip.device_count() > 0, "needs an MI355X: there is nothing to time without one"
    print(f"# {murbhip.device_count()} device(s); {args.rounds} rounds a b a b, windows of ~{args.seconds} s; host clock around synced calls")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        with murbhip.Simulation(n) as sim:
            sim.set_option("integrator", 2)
            sim.upload(s)
            sim.warmup(100.0)
            k = max(64, min(20000, int(args.seconds / fixed(sim, 8))))
            pinned(sim, 8)     # first launches of the adaptive kernels
            a, b = [], []
            for _ in range(args.rounds):
                a.append(fixed(sim, k))
                b.append(pinned(sim, k))
            tail = [one_step(sim, 64) - one_step(sim, 1) for _ in range(args.rounds)] if n >= 100000 else None
        ma, mb = statistics.median(a), statistics.median(b)
        us = lambda xs: ", ".join(f"{x * 1e6:.1f}" for x in xs)
        print(f"N = {n}  K = {k} steps per window")
        print(f"  (a) murbhip_steps        : median {ma * 1e6:10.1f} us per step   rounds: {us(a)}")
        print(f"  (b) murbhip_evolve pinned: median {mb * 1e6:10.1f} us per step   rounds: {us(b)}")
        print(f"  b / a = {mb / ma:.4f}   spread of (a): {(max(a) - min(a)) / ma * 100:.2f} %, of (b): {(max(b) - min(b)) / mb * 100:.2f} %")
        if tail:
            mt = statistics.median(tail)
            print(f"  no-op tail: 63 steps (252 launches) with the done flag set: median {mt * 1e6:.1f} us"
                  f" = {mt / 252 * 1e6:.2f} us a launch, {mt / 252 * 64 * 1e6:.1f} us per 64 launches   rounds: {us(tail)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a block step of murbhip_evolve_block costs against the size of its active set, beside a fixed Hermite step of all
bodies (murbhip_steps, "integrator" 2), per value of "block_units".

An active set of a chosen size is held for a whole timed window through the test hooks: the chosen bodies get level kmax
(steps of one tick), the others level 0, and eta is so small that the criterion never lets a level go up again — so the
K <= 2^kmax - 1 block steps of a window all advance exactly those bodies (every step counts as clamped, which costs nothing).
Host clock around calls that end in a device sync, K block steps a call in batches of 64 ("evolve_batch" 64, K a multiple of
64: no no-op tail), same process, alternating rounds over (units, active set) after murbhip_warmup.  Also the no-op tail of a
batch: one block step with "evolve_batch" 64 (63 x 6 launches find the done flag set) against "evolve_batch" 1.

    python tools/hermite_block_rate.py [--sizes 30000,200000] [--active 1,16,256,4096,0] [--units 0,256,640,2560,5120]
                                       [--rounds 3] [--seconds 0.1] [--nearest | --contact]

(active 0 = all bodies, units 0 = the default.  --nearest: every cell is timed twice in every round, with option "nearest" 0 and
1, and a second table has the ratio 1 / 0; --contact: the same with option "contact" and the scheme's own radii.)  Prints per size a table of median microseconds per block step."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

DT, KMAX, TINY_ETA = 3600.0, 12, 1e-12


def fixed(sim, s, k):
    sim.upload(s)
    sim.compute_acc_jerk()
    sim.sync()
    t0 = time.perf_counter()
    sim.steps(DT, k)
    sim.sync()
    return (time.perf_counter() - t0) / k


def block(sim, s, levels, k, batch=64):
    """Seconds per block step over k steps that all advance the bodies at level KMAX."""
    sim.upload(s)
    sim.compute_acc_jerk()
    sim.set_block_levels(levels, KMAX)     # syncs
    sim.set_option("evolve_batch", batch)
    t0 = time.perf_counter()
    out = sim.evolve_block(DT * 2 ** KMAX, eta=TINY_ETA, kmax=KMAX, max_steps=k)     # a step of the active bodies is DT
    t = time.perf_counter() - t0
    sim.set_option("evolve_batch", 0)
    want = int((levels == KMAX).sum())
    assert out["steps"] == k and out["body_steps"] == k * want and out["max_active"] == want, out
    return t / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30000,200000")
    ap.add_argument("--active", default="1,16,256,4096,0")
    ap.add_argument("--units", default="0,256,640,2560,5120")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.1, help="length of one timed window (sets K per case)")
    ap.add_argument("--nearest", action="store_true", help='also time every cell with option "nearest" 1')
    ap.add_argument("--contact", action="store_true", help='also time every cell with option "contact" 1 (not beside --nearest)')
    args = ap.parse_args()
    assert not (args.nearest and args.contact), "--nearest and --contact exclude each other, like the options"
    extra = "contact" if args.contact else "nearest" if args.nearest else None
    assert murbhip.device_count() > 0, "needs an MI355X: there is nothing to time without one"
    units = [int(x) for x in args.units.split(",")]
    print(f"# {args.rounds} alternating rounds, windows of ~{args.seconds} s, host clock around synced calls; microseconds per step")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        active = [n if int(x) == 0 else min(int(x), n) for x in args.active.split(",")]
        with murbhip.Simulation(n) as sim:
            sim.set_option("integrator", 2)
            sim.upload(s)
            if args.contact:
                sim.upload_radii(s["r"])
            sim.warmup(100.0)
            print(f"N = {n}: {int(sim.info('cu_count'))} CUs, sweep grid {int(sim.info('block_grid'))} workgroups, default "
                  f"block_units {int(sim.info('block_units'))}, {int(sim.info('slots')) // 512} layout tiles")
            levels = {}
            for m in active:     # spread over the bodies; the last real body always among them
                lv = np.zeros(n, np.int32)
                lv[np.unique(np.linspace(0, n - 1, m).astype(np.int64))] = KMAX
                lv[n - 1] = KMAX
                if m == n:
                    lv[:] = KMAX
                levels[m] = lv
            k_of = {}
            for m in active:     # window lengths from a first, untimed look
                t = block(sim, s, levels[m], 64)
                k_of[m] = max(64, min(2 ** KMAX - 64, int(args.seconds / t) // 64 * 64))
            k_fixed = max(8, int(args.seconds / fixed(sim, s, 8)))
            times = {(u, m): [] for u in units for m in active}
            near = {(u, m): [] for u in units for m in active}
            fix, fix_near = [], []
            for _ in range(args.rounds):
                fix.append(fixed(sim, s, k_fixed))
                if extra:
                    sim.set_option(extra, 1)
                    fix_near.append(fixed(sim, s, k_fixed))
                    sim.set_option(extra, 0)
                for u in units:
                    sim.set_option("block_units", u)
                    for m in active:
                        times[(u, m)].append(block(sim, s, levels[m], k_of[m]))
                        if extra:
                            sim.set_option(extra, 1)
                            near[(u, m)].append(block(sim, s, levels[m], k_of[m]))
                            sim.set_option(extra, 0)
            sim.set_option("block_units", 0)
            tail = [block(sim, s, levels[active[0]], 1, 64) - block(sim, s, levels[active[0]], 1, 1) for _ in range(max(args.rounds, 5))]
        mf = statistics.median(fix)
        print(f"  murbhip_steps (fixed step of all bodies): median {mf * 1e6:.1f}   rounds: " + ", ".join(f"{x * 1e6:.1f}" for x in fix))
        print("  block step, median per (block_units, active set); K = " + ", ".join(f"{m}: {k_of[m]}" for m in active))
        print("    units \\ active " + "".join(f"{m:>12d}" for m in active))
        for u in units:
            print(f"    {u:>14d} " + "".join(f"{statistics.median(times[(u, m)]) * 1e6:12.1f}" for m in active))
        if extra:
            mn = statistics.median(fix_near)
            print(f"  murbhip_steps with \"{extra}\" 1: median {mn * 1e6:.1f} ({mn / mf:.3f} of the plain step)   rounds: "
                  + ", ".join(f"{x * 1e6:.1f}" for x in fix_near))
            print(f"  block step with \"{extra}\" 1, median, and its ratio to \"{extra}\" 0")
            for u in units:
                print(f"    {u:>14d} " + "".join(f"{statistics.median(near[(u, m)]) * 1e6:12.1f}" for m in active))
                print(f"    {'ratio':>14s} " + "".join(f"{statistics.median(near[(u, m)]) / statistics.median(times[(u, m)]):12.3f}" for m in active))
        full = statistics.median(times[(units[0], active[-1])])
        if active[-1] == n:
            print(f"  block step of all bodies / fixed step = {full / mf:.3f}")
        spread = max((max(v) - min(v)) / statistics.median(v) for v in times.values())
        print(f"  largest spread of a cell over its rounds: {spread * 100:.1f} %")
        mt = statistics.median(tail)
        print(f"  no-op tail: 63 block steps (378 launches) with the done flag set: median {mt * 1e6:.1f} us = {mt / 378 * 1e6:.2f} us a launch"
              "   rounds: " + ", ".join(f"{x * 1e6:.1f}" for x in tail))


if __name__ == "__main__":
    main()

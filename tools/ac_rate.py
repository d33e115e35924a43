#!/usr/bin/env python3
"""Cost of the Ahmad-Cohen scheme (include/murbac.h): an irregular step by launch, a regular step with the rebuild separated out, and
the whole cycle of n_irr steps against n_irr plain Hermite steps of the same process, the two legs alternating, three rounds, one
process after murbhip_warmup.

    python tools/ac_rate.py [--sizes 4096,200000] [--ks 32,128] [--nirr 1,4,8,16] [--rounds 3] [--out profiles/ac_steps.txt]

Wall times are of enqueue + sync over whole cycles; the kernel times are HIP-event spans ("profile" 2): `list` the list sweeps,
`nbr` the rebuild's count and fill sweeps, `force` the full acceleration + jerk sweep, `ac_predict` and `ac_correct` the two small
launches of an irregular step.  The spans come from one more, profiled, run of each leg; the wall times from unprofiled ones."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-eurohpc_amd"))
import murbhip   # noqa: E402

SOFT, DT = 2e8, 3600.0


def spans(sim):
    out = {k: sim.info(f"span_{k}_ms_avg") * sim.info(f"span_{k}_count") for k in ("list", "nbr", "ac_predict", "ac_correct")}
    out["force"] = sim.info("force_ms_total")
    out["lists"] = sim.info("span_list_count")
    return out


def timed(sim, call, steps, profile=0):
    """Wall milliseconds per step of `call` (enqueue, then sync); with profile=2 also the spans' totals per step.  The wall times
    that are reported come from unprofiled runs: two event records a launch cost a small step as much as the launch."""
    sim.sync()
    sim.set_option("profile", profile)   # drains the device and clears the samples
    t0 = time.perf_counter()
    call()
    sim.sync()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return wall, ({k: v / steps for k, v in spans(sim).items()} if profile else {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,200000")
    ap.add_argument("--ks", default="32,128")
    ap.add_argument("--nirr", default="1,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {murbhip.device_count()} device(s); rounds {args.rounds}, legs alternating; dt {DT}; ms per step unless a cycle is named")
    for n in (int(x) for x in args.sizes.split(",")):
        s = murbhip.init_bodies(n, "galaxy")
        cycles = 2 if n > 50000 else 16
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.set_option("integrator", 2)
            sim.upload(s)
            sim.warmup(100.0)
            say(f"N = {n}  ({int(sim.info('cu_count'))} CUs)")
            for k in (int(x) for x in args.ks.split(",")):
                sim.upload(s)
                h = sim.ac_radii(k)
                # all steps irregular: the largest n_irr
                sim.ac_begin(h, murbhip.AC_NIRR_MAX)
                st = sim.ac_state()
                sim.ac_steps(DT, 4)
                irr = [timed(sim, lambda: sim.ac_steps(DT, 64), 64) for _ in range(args.rounds)]
                profiled, x = timed(sim, lambda: sim.ac_steps(DT, 64), 64, profile=2)
                wall, sweep, pred, corr = np.mean([w for w, _ in irr]), x["list"], x["ac_predict"], x["ac_correct"]
                say(f"  ac_radii({k}): mean list {st['mean']:.1f}, longest {st['longest']}, entries {st['entries']}")
                say(f"    irregular step {wall:.4f} ms (rounds " + ", ".join(f"{w:.4f}" for w, _ in irr) + f"): predictor {pred:.4f} ms, list sweep {sweep:.4f} ms, "
                    f"corrector {corr:.4f} ms (spans of a profiled round of {profiled:.4f} ms a step); the wall time's remainder {wall - pred - sweep - corr:.4f} ms")
                for n_irr in (int(x) for x in args.nirr.split(",")):
                    steps = n_irr * cycles
                    ac, herm = [], []
                    for _ in range(args.rounds):
                        sim.upload(s)
                        sim.steps(DT, 1)
                        herm.append(timed(sim, lambda: sim.steps(DT, steps), steps))
                        sim.upload(s)
                        sim.ac_begin(h, n_irr)
                        sim.ac_steps(DT, n_irr)
                        ac.append(timed(sim, lambda: sim.ac_steps(DT, steps), steps))
                        end = sim.ac_state()
                    sim.upload(s)
                    sim.ac_begin(h, n_irr)
                    sim.ac_steps(DT, n_irr)
                    x = timed(sim, lambda: sim.ac_steps(DT, steps), steps, profile=2)[1]
                    sim.set_option("profile", 0)
                    aw, hw = np.mean([w for w, _ in ac]), np.mean([w for w, _ in herm])
                    per_cycle = {key: x[key] * n_irr for key in ("list", "nbr", "force", "lists")}   # of the profiled cycles
                    say(f"    n_irr {n_irr:2d}: cycle {aw * n_irr:9.4f} ms (rounds " + ", ".join(f"{w * n_irr:.4f}" for w, _ in ac) + f") against {n_irr} Hermite steps "
                        f"{hw * n_irr:9.4f} ms (rounds " + ", ".join(f"{w * n_irr:.4f}" for w, _ in herm) + f"): x {hw / aw:.2f}")
                    say(f"               per cycle: full sweep {per_cycle['force']:.4f} ms, rebuild sweeps (count + fill) {per_cycle['nbr']:.4f} ms, "
                        f"{per_cycle['lists']:.0f} list sweeps {per_cycle['list']:.4f} ms, the rest (small launches, the round trip, gaps) "
                        f"{aw * n_irr - per_cycle['force'] - per_cycle['nbr'] - per_cycle['list']:.4f} ms; lists at the end: mean {end['mean']:.1f}, longest {end['longest']}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

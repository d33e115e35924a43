#!/usr/bin/env python3
"""Cost of the potential read-out: murbpot_of at `count` of the N bodies beside murbfield_of and murbbind_of at the same bodies,
with and without a mask, and one murbbound_members call on a Plummer sphere with escapers (tests/helpers/bound_ref.py's
fixture B at size N), in the same process and build.  One process after murbhip_warmup, the legs alternating, three rounds of
five calls.

    python tools/pot_rate.py [--sizes 200000] [--counts 4096,0] [--reps 5] [--rounds 3] [--out profiles/pot_sweep.txt]

Two times per leg: the sweep kernels' HIP-event spans ("profile" 2, span_<kind>_ms_avg x span_<kind>_count: the call's launches
summed; kind pot, field, bind) and the wall time of the whole synchronous call.  pairs/s = count x N / time.  count 0 means N.
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
import bound_ref    # noqa: E402

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

    sizes = [int(x) for x in args.sizes.split(",")]
    say(f"# {murbhip.device_count()} device(s); reps {args.reps}, rounds {args.rounds}; kernel = HIP-event spans of the sweeps, call = wall time of the synchronous call")
    for n in sizes:
        s = murbhip.init_bodies(n, "galaxy")
        rng = np.random.default_rng(1)
        mask = rng.uniform(size=n) < 0.5
        with murbhip.Simulation(n, soft=SOFT) as sim:
            sim.upload(s)
            sim.warmup(100.0)
            counts = [int(c) or n for c in args.counts.split(",")]
            lists = {c: np.sort(rng.choice(n, c, replace=False)).astype(np.int32) for c in counts}
            legs = ["field", "bind", "pot", "pot+mask"]
            got = {(c, leg): [] for c in counts for leg in legs}
            for _ in range(args.rounds):
                for c in counts:
                    got[(c, "field")].append(timed(sim, lambda: sim.field_of(lists[c]), "field", args.reps))
                    got[(c, "bind")].append(timed(sim, lambda: sim.bound_partner_of(lists[c]), "bind", args.reps))
                    got[(c, "pot")].append(timed(sim, lambda: sim.potential_of(lists[c]), "pot", args.reps))
                    got[(c, "pot+mask")].append(timed(sim, lambda: sim.potential_of(lists[c], member=mask), "pot", args.reps))
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
            say(f"  pot / field kernel time at count {c}: {kern['pot'] / kern['field']:.3f};  pot / bind: {kern['pot'] / kern['bind']:.3f}")
        q, v, m = bound_ref.plummer(n, np.random.default_rng(12))
        b = bound_ref._state(q, v * 1.3, m)
        with murbhip.Simulation(n, soft=float(bound_ref.SOFT), g=bound_ref.G) as sim:
            sim.upload(b)
            sim.warmup(100.0)
            sim.bound_members()
            kernel, wall = timed(sim, sim.bound_members, "pot", 1)
            r = sim.bound_members()
            sim.set_option("profile", 0)
        say(f"  bound_members(), Plummer sphere with velocities x 1.3: {r['rounds']} rounds, converged {r['converged']}, {r['members']} members of {n}, "
            f"bound mass {r['mass']:.4f}, K/|W| {r['virial_ratio']:.3f}: sweeps {kernel:9.4f} ms   call {wall:9.4f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""GPU: murbhip_block_set_levels clears every body's ticks before it returns, in the order of the compute stream.

The call used to clear them with a fill on the null stream, which returns before the fill has run and which the compute stream
(non-blocking) does not wait for.  The next murbhip_evolve_block then could read the last block's ticks in its first launch
(the minimum over t_i + step_i) and the cleared ones in its second (who is due at that time): a step that stepped nobody,
body_steps == 0.  Whether the two streams really overlap depends on the hardware queues they fall on.  It showed in
tests/test_block_wrap_gpu.py, deterministically, once tests/test_bind_gpu.py had run before it in the same process (a block
left open and finished on one context, then a context of two shards), and went away with the ordered fill.

This file states the contract in that file's shape: after the same two contexts, block steps of a large active set and then of
single bodies, each from an open block whose ticks are not zero, with the read-outs that file makes in between; every step
steps exactly the bodies whose level was set, and their ticks alone move.  It is NOT a reproducer: a build with the former fill
passed it on the one MI355X it was tried on, where the two files in the order above still failed.  That order stays the check
that caught it."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import knn_ref as K           # noqa: E402

pytestmark = pytest.mark.gpu

SOFT, DT_MAX, KMAX = np.float32(2e8), np.float32(4.0 * 3600.0), 2


def contexts_before(gpu, small):
    """What ran before in the process that showed it: a block left open and finished on one context, a context of two shards."""
    s, soft = K.plummer(3000)
    with gpu.Simulation(3000, soft=soft, g=1.0) as sim:
        sim.set_option("integrator", 2)
        sim.upload(s)
        assert not sim.evolve_block(2.0 ** -6, blocks=1, kmax=5, max_steps=1)["synchronised"]
        assert sim.evolve_block(2.0 ** -6, blocks=1, kmax=5)["synchronised"]
    with gpu.Simulation(2049, soft=SOFT, devices=[0, 0]) as two:
        two.upload(small)


@pytest.mark.parametrize("n", (5120, 4609))
def test_levels_and_cleared_ticks_reach_the_next_block(gpu, O, n):
    s = O.init_bodies(n, "random")
    stale = {k: (np.float32(2.0) * v if k in ("qx", "qy", "qz") else v.copy()) for k, v in s.items()}
    contexts_before(gpu, {k: v[:2049] for k, v in s.items()})
    sets = [np.arange(0, n, 2)] + [np.array([b]) for b in (0, 511, 512, n - 1)]
    for option in (None, "potential", "nearest"):
        with gpu.Simulation(n, soft=SOFT) as sim:
            sim.set_option("integrator", 2)
            if option:
                sim.set_option(option, 1)
            for act in sets:
                sim.set_option("block_units", -(-len(act) // 16))
                levels = np.zeros(n, np.int32)
                levels[act] = KMAX
                for state in (stale, s):
                    sim.upload(state)
                    sim.compute_acc_jerk()
                    sim.acc(), sim.jerk()
                    if option:
                        sim.potential() if option == "potential" else sim.nearest()
                    sim.set_block_levels(levels, KMAX)      # nothing between this and the block: a read-out here would wait for the fill
                    out = sim.evolve_block(float(DT_MAX), kmax=KMAX, max_steps=1)      # leaves the block open: the active bodies at tick 1
                    assert out["steps"] == 1 and out["body_steps"] == len(act) == out["max_active"], (option, len(act), out)
                    ticks, _ = sim.block_state()
                    assert (ticks[act] == 1).all() and ticks.sum() == len(act), (option, len(act))

"""The pair-symmetric kernels on the work lists of a ragged last block, residue by residue.  All tests here need an MI355X.

With "pad_aware" 1 the work list depends on `rem`, the number of real bodies in a slice's last block of 1024 slots: which
block of a pair is walked, which sub-blocks are dropped, where the piece that straddles the last real body is cut (the next
multiple of 16 x waves: 64 or 128 bodies), and the steps of a triangular diagonal piece.  tests/test_abi_and_host.py checks
those tables cell by cell on the CPU; here the kernels run on them, for every residue of helpers/ragged.py (both sides of
every such length), with the probes of tests/test_pair_coverage.py as they stand: every body's acceleration against the
fp64 sum over the probe's sources, relative to the sum of the term magnitudes (TOL_F64_MAX), the potential energy against
the fp64 pair sum (TOL_PE_FUSED; TOL_PE_SWEEP at a single block), each probe asserting its own power.  No tolerance is
defined here.

Besides the sources oracle.probe_sources places (the last three bodies, each shard's first and last body, eight offsets a
block), every ragged block carries mass on its first body, on both sides of every multiple of 64 below `rem` and on the
body before its last one (helpers/ragged.py: ragged_sources): both sides of every possible cut."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_pair_coverage import BLOCK, SOFT, TOL_PE_FUSED, TOL_PE_SWEEP, Problem, probe_forces, probe_potential, probe_step, set_options

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from ragged import REMS, ragged_sources   # noqa: E402

pytestmark = pytest.mark.gpu


class RaggedProblem(Problem):
    """A Problem whose every probe also holds the ragged blocks' sources."""

    def __init__(self, gpu, O, n, world=1, probes=4, k_max=128, per_block=8):
        super().__init__(gpu, O, n, world=world, probes=probes, k_max=k_max, per_block=per_block)
        extra = ragged_sources(self.firsts, self.counts, self.slice)
        for f, c in zip(self.firsts, self.counts):          # what the sweep is about, restated: the slice's last block
            rem = c % BLOCK
            if rem:
                first = f + c - rem
                want = {first, first + max(rem - 2, 0)} | {first + 64 * k - d for k in range(1, (rem - 1) // 64 + 1) for d in (0, 1)}
                assert want <= set(extra.tolist()), (n, world, rem)
        self.sources = [np.union1d(src, extra) for src in self.sources]


def forced(sim, what, **opts):
    """Force the pair-symmetric kernel with `opts` and check what the context reports of the plan: the variant, sym_waves,
    jsplit and taper.  It has no read-out for diag_tri, sym_red, xcd_order or pad_aware (as in test_forced_options): a
    wrong result under them fails the probes, an ignored option would not show."""
    set_options(sim, variant=8, **opts)
    got = {k: int(sim.info(k)) for k in ("variant", "sym_waves", "jsplit", "taper") if k == "variant" or k in opts}
    assert got == {k: (8 if k == "variant" else opts[k]) for k in got}, (what, got)


# ---------------------------------------------------------------------------------------------------- one GPU
# (sym_waves, jsplit, taper, diag_tri, sym_red), then one list in XCD order and one that walks the padding
SETTINGS = [dict(sym_waves=w, jsplit=j, taper=t, diag_tri=d, sym_red=r) for (w, j, t, d, r) in
            [(4, 1, 0, 0, 0), (4, 4, 30, 1, 1), (4, 16, 100, 1, 1), (8, 1, 0, 1, 1), (8, 8, 100, 0, 0), (8, 4, 30, 1, 1)]]
SETTINGS += [dict(SETTINGS[1], xcd_order=1), dict(SETTINGS[3], pad_aware=0)]
WITH_ENERGY = (1, 4)    # a triangular and a plain diagonal block: the fused pair potential + the diagonal-block potential kernel


@pytest.mark.parametrize("rem", REMS)
def test_ragged_last_block_one_gpu(gpu, O, rem):
    """n = rem, 1024 + rem and 3072 + rem, one context each: the default plan (the one-launch one-sided kernel), then the
    pair-symmetric kernel forced under every setting: compute_acc and the step route (the row sum + update in the launch
    behind it) for each, energy() for two.  Above one block the potential comes out of the fused pair potential plus the
    diagonal-block potential kernel and is held to TOL_PE_FUSED.  At n = rem there is no off-diagonal item: the
    diagonal-block kernel on the single ragged block is the whole answer, a few fp32 pair terms with nothing to average
    over, held to TOL_PE_SWEEP like the other small potentials of test_pair_coverage.py."""
    for n in ([rem] if rem >= 2 else []) + [BLOCK + rem, 3 * BLOCK + rem]:
        P = RaggedProblem(gpu, O, n)
        Q = RaggedProblem(gpu, O, n, probes=2, k_max=64)
        with gpu.Simulation(n, soft=SOFT) as sim:
            if n <= 2 * BLOCK:
                assert int(sim.info("variant")) == 1
            what = f"n={n} default plan (variant {int(sim.info('variant'))})"
            probe_forces(P, sim, what)
            probe_step(P, sim, what)
            for k, opts in enumerate(SETTINGS):
                what = f"n={n} rem={rem} {opts}"
                forced(sim, what, **opts)
                probe_forces(P, sim, what)
                probe_step(P, sim, what)
                if k in WITH_ENERGY:
                    probe_potential(Q, sim, what, TOL_PE_FUSED if n > BLOCK else TOL_PE_SWEEP)


# ---------------------------------------------------------------------------------------------------- passes
@pytest.mark.parametrize("rem", [1, 65, 129, 513])
def test_ragged_last_block_in_passes(gpu, O, rem):
    """Ten blocks under a partial-row budget of 1 MiB (seven passes): the ragged block's items fall into several passes."""
    n = 9 * BLOCK + rem
    P = RaggedProblem(gpu, O, n)
    Q = RaggedProblem(gpu, O, n, probes=2, k_max=64)
    with gpu.Simulation(n, soft=SOFT) as sim:
        set_options(sim, sym_pass_mb=1)
        probe_forces(P, sim, f"n={n} sym_pass_mb=1")
        assert int(sim.info("variant")) == 8 and sim.info("sym_passes") >= 2, sim.info("sym_passes")
        probe_step(P, sim, f"n={n} sym_pass_mb=1")
        probe_potential(Q, sim, f"n={n} sym_pass_mb=1", TOL_PE_FUSED)
        assert sim.info("sym_passes") >= 2


# ---------------------------------------------------------------------------------------------------- shards on one device
SHARD_OPTIONS = [dict(), dict(overlap=0), dict(overlap=2, tri_div=2, tri_first_pct=0), dict(tri_div=8, tri_first_pct=100)]


@pytest.mark.parametrize("rem", [1, 2, 64, 65, 128, 129, 513, 1023])
@pytest.mark.parametrize("shards", [2, 3, 4])
def test_ragged_last_blocks_of_shards(gpu, O, shards, rem):
    """Two blocks a slice on 2, 3 and 4 shards of one device: every slice ends in rem bodies (k = 0), or one of them in
    rem - 1 (k = 1: cut lengths 128 and 64 in one block pair at rem = 65; a wholly empty block at rem = 1)."""
    for k in (0, 1):
        n = shards * (BLOCK + rem) - k
        P = RaggedProblem(gpu, O, n, world=shards)
        Q = RaggedProblem(gpu, O, n, world=shards, probes=2, k_max=64)
        assert sorted({c - BLOCK for c in P.counts}) == ([rem] if k == 0 else [rem - 1, rem])
        with gpu.Simulation(n, soft=SOFT, devices=[0] * shards) as sim:
            for opts in SHARD_OPTIONS:
                what = f"n={n} shards={shards} rem={rem} {opts}"
                forced(sim, what, **opts)
                probe_forces(P, sim, what)
            probe_potential(Q, sim, what, TOL_PE_FUSED)


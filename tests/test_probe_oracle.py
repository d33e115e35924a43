"""CPU: the checker of the sparse-mass probes (tests/test_pair_coverage.py).  The sources oracle agrees with the full fp64
direct sum, an honest fp32 sum passes the probe metric, and every kind of pair-coverage bug fails it: the GPU tests'
tolerance is neither too tight nor blind."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from ragged import ragged_offsets, ragged_sources   # noqa: E402

SOFT = np.float32(2e8)
TOL_F64_MAX = 2e-6     # tests/test_gpu_parity.py
TOL_PE_FUSED = 1e-7    # ... the potential out of the pair-symmetric force evaluation


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


def geometry(mh, n, world):
    fc = [mh.partition(n, world, r) for r in range(world)]
    return [f for f, _ in fc], [c for _, c in fc], mh.slice_slots(n, world)


def term(s, i, j, soft=SOFT, q_from=None):
    """fp64 c_ij: the pull of body j (mass m_j, at the position of body q_from, default j) on body i."""
    q_from = j if q_from is None else q_from
    d = np.array([np.float64(s[k][q_from]) - np.float64(s[k][i]) for k in ("qx", "qy", "qz")])
    g = np.float64(np.float32(6.67384e-11))
    return g * np.float64(s["m"][j]) * d / (d @ d + np.float64(soft) ** 2) ** 1.5


@pytest.fixture(scope="module", params=["galaxy", "random"])
def probe(request, mh, O):
    n = 3001
    s = O.init_bodies(n, request.param)
    src = O.probe_sources(n, *geometry(mh, n, 1), probes=1)[0]
    ps = O.probe_state(s, src, seed=5)
    return ps, src, O.accel_f64_sources(ps, src)


def test_sources_oracle_equals_the_full_direct_sum(O, probe):
    ps, src, (a, abs_sum, min_term) = probe
    full = O.accel_f64(ps, SOFT)
    assert O.rel_err(a, full).max() <= 1e-12
    assert O.probe_err(a, full, abs_sum).max() <= 1e-12
    assert (abs_sum > 0).all() and np.isfinite(min_term).all()
    _, pe = O.energy_f64(ps, SOFT)
    pe_src, min_pair = O.potential_f64_sources(ps, src)
    assert abs(pe_src - pe) <= 1e-12 * abs(pe) and 0 < min_pair < abs(pe)


def test_probe_has_the_power_to_see_one_term(O, probe):
    ps, src, (a, abs_sum, min_term) = probe
    assert (O.probe_power(abs_sum, min_term) >= 10 * TOL_F64_MAX).mean() >= 0.99


def test_honest_fp32_sum_passes(O, probe):
    ps, src, (a, abs_sum, _) = probe
    f32 = O.accel_slice_f32(ps, 0, len(ps["qx"]), SOFT)
    assert O.probe_err(f32, a, abs_sum).max() <= TOL_F64_MAX


def test_every_mutation_fails(O, probe):
    """One (i, s) term missing, one doubled, a source's mass at its neighbour's position, a reaction of the wrong sign:
    each fails the metric, on a body where the probe claims the power to see it."""
    ps, src, (a, abs_sum, min_term) = probe
    n = len(ps["qx"])
    truth = np.stack(a)
    power = O.probe_power(abs_sum, min_term)
    rng = np.random.default_rng(3)
    seen = np.flatnonzero(power >= 10 * TOL_F64_MAX)
    for i in rng.choice(seen, 8, replace=False):
        s = rng.choice(src[src != i])
        c = term(ps, i, s)
        for mutated in (truth[:, i] - c, truth[:, i] + c):        # pair skipped / counted twice
            m = truth.copy()
            m[:, i] = mutated
            assert O.probe_err(tuple(m), a, abs_sum)[i] > 10 * TOL_F64_MAX
    # a source's mass pulling from the next slot's position (a misrouted j index), felt by every body
    s = int(src[len(src) // 2])
    nb = s + 1 if s + 1 < n else s - 1
    m = truth.copy()
    for i in range(n):
        if i != s:
            m[:, i] += term(ps, i, s, q_from=nb) - term(ps, i, s)
    assert (O.probe_err(tuple(m), a, abs_sum) > TOL_F64_MAX).mean() > 0.5
    # the reaction of a pair-symmetric item with its sign flipped: the j side block of one item gets -c instead of +c
    blk = s // 1024
    other = (blk + 1) % (-(-n // 1024))
    rows = [i for i in range(other * 1024, min(n, other * 1024 + 1024)) if i != s]
    m = truth.copy()
    for i in rows:
        m[:, i] -= 2 * term(ps, i, s)
    e = O.probe_err(tuple(m), a, abs_sum)[rows]
    assert (e > 10 * TOL_F64_MAX).mean() > 0.99


def test_potential_probe_sees_one_pair(O, mh):
    """At most 64 sources: one pair of the potential is >= 10x the fused path's tolerance; a missing one fails it."""
    n = 30000
    s = O.init_bodies(n, "galaxy")
    for src in O.probe_sources(n, *geometry(mh, n, 1), probes=2, k_max=64, per_block=2):
        ps = O.probe_state(s, src)
        pe, min_pair = O.potential_f64_sources(ps, src)
        assert min_pair >= 10 * TOL_PE_FUSED * abs(pe)
        assert abs((pe + min_pair) - pe) > TOL_PE_FUSED * abs(pe)


@pytest.mark.parametrize("n,world", [(1024, 1), (29659, 1), (1000000, 1), (6151, 3), (30000, 8), (200000, 8)])
def test_probe_sources_cover_every_block(O, mh, n, world):
    """Every block holds a source in some probe, the shards' first and last bodies and the problem's last three are
    sources, consecutive probes share no slot, and no probe has more than its limit."""
    firsts, counts, slice_slots = geometry(mh, n, world)
    probes = O.probe_sources(n, firsts, counts, slice_slots, probes=2)
    assert len(probes) >= 2 and all(0 < len(p) <= 256 for p in probes)
    blocks = set()
    for p in probes:
        assert len(np.unique(p)) == len(p) and p.min() >= 0 and p.max() < n
        blocks.update(mh.slot_of_body(n, world, int(i)) // 1024 for i in p)
    assert blocks == set(range(world * slice_slots // 1024))
    every = set(np.concatenate(probes).tolist())
    assert every >= set(firsts) | {f + c - 1 for f, c in zip(firsts, counts)} | {n - 3, n - 2, n - 1}
    for p, q in zip(probes, probes[1:]):
        assert not set(p.tolist()) & set(q.tolist())


def test_ragged_offsets_straddle_every_cut():
    """helpers/ragged.py: a ragged block's first body, both sides of every multiple of 64 below its `rem` bodies, rem - 2."""
    assert ragged_offsets(130) == [0, 63, 64, 127, 128] and ragged_offsets(129) == [0, 63, 64, 127, 128]
    assert ragged_offsets(128) == [0, 63, 64, 126] and ragged_offsets(65) == [0, 63, 64] and ragged_offsets(64) == [0, 62]
    assert ragged_offsets(1) == [0] and ragged_offsets(2) == [0] and len(ragged_offsets(1023)) == 32
    firsts, counts, slice_slots = [0, 1089, 2178], [1089, 1089, 1088], 2048      # n = 3 (1024 + 65) - 1
    assert ragged_sources(firsts, counts, slice_slots).tolist() == [f + 1024 + o for f, c in zip(firsts, counts)
                                                                    for o in ([0, 63, 64] if c == 1089 else [0, 62])]


@pytest.mark.parametrize("rem", [2, 65, 513, 1023])
def test_ragged_probes_keep_their_power(O, mh, rem):
    """The probes of tests/test_ragged_block_gpu.py carry up to 33 more sources per ragged block: at its sizes with the most
    of them the force probes still see one term on 99 % of the bodies and the potential probes one pair, 10x the tolerances."""
    for n, world in [(rem, 1), (1024 + rem, 1), (3072 + rem, 1), (9 * 1024 + rem, 1)] + [(W * (1024 + rem) - k, W) for W in (2, 4) for k in (0, 1)]:
        s = O.init_bodies(n, "galaxy")
        firsts, counts, slice_slots = geometry(mh, n, world)
        extra = ragged_sources(firsts, counts, slice_slots)
        for src in O.probe_sources(n, firsts, counts, slice_slots, probes=4, k_max=128, per_block=8):
            src = np.union1d(src, extra)
            ps = O.probe_state(s, src)
            _, abs_sum, min_term = O.accel_f64_sources(ps, src, SOFT)
            assert (O.probe_power(abs_sum, min_term) >= 10 * TOL_F64_MAX).mean() >= 0.99, (n, world)
        for src in O.probe_sources(n, firsts, counts, slice_slots, probes=2, k_max=64, per_block=8):
            src = np.union1d(src, extra)
            pe, min_pair = O.potential_f64_sources(O.probe_state(s, src), src, SOFT)
            assert min_pair >= 10 * TOL_PE_FUSED * abs(pe), (n, world, min_pair / abs(pe))

"""CPU: the yardsticks and the shapes of tests/test_full_wrap_gpu.py (the FULL Hermite sweeps' nearest, contact and potential
forms at 10 to 60 layout tiles).  The row-blocked restatements equal the unblocked ones bit for bit; the dense tie lattice keeps
its properties at the new sizes; the case table of tests/helpers/full_wrap.py holds every shape the GPU file is there for, so
that a later change of sizes or cuts cannot make it go blind; and honest float32 in the device's summation order meets half
the phi bound on every potential case."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import contact_ref as CR      # noqa: E402
import full_wrap as W         # noqa: E402
import hermite_ref as H       # noqa: E402
import nearest_ref as N       # noqa: E402
import potential_ref as PR    # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@lru_cache(maxsize=None)
def lattice(n):
    s, soft, q = N.dense_lattice(n)
    assert soft == np.float32(0.5)
    q2, k = N.shifted(q)
    return s, q, q2, k, CR.dense_radii(n)


# ------------------------------------------------------------------------------------------------ 1. the blocked restatements
@pytest.mark.parametrize("n", [2049, 2561])
def test_blocked_equals_unblocked(n):
    s, q, q2, k, radii = lattice(n)
    for pos in (q, q2):
        want = N.nearest(pos, 0.25, exact=True)
        got = N.nearest_blocked(pos, 0.25)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        want = CR.contact(pos, radii, 0.25)
        got = CR.contact_blocked(pos, radii, 0.25)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        assert not np.signbit(got[1][got[1] == 0]).any()
    m = N.r2_matrix(q, 0.25)
    assert np.array_equal(bits(N.r2_rows(q, 0.25, 512, 1100)), bits(m[512:1100]))
    g = CR.gap2_matrix(q, radii, 0.25)
    assert np.array_equal(bits(CR.gap2_rows(q, radii, 0.25, 2000, n)), bits(g[2000:n]))
    # the blocked statistics are the matrix ones
    st = N.tie_stats_blocked(q, 0.25, lambda lo, hi: N.r2_rows(q, 0.25, lo, hi))
    cnt, span, own = N.tie_stats(m)
    assert np.array_equal(st["cnt"], cnt) and np.array_equal(st["span"], span) and np.array_equal(st["own"], own)
    assert np.array_equal(st["high"], N.highest_index_wins(m)) and np.array_equal(st["later"], N.later_tile_wins(m))
    assert np.array_equal(st["idx"], m.argmin(1)) and np.array_equal(st["idx"], N.nearest_blocked(q, 0.25)[0])
    assert np.array_equal(bits(st["val"]), bits(m.min(1)))
    ct = N.tie_stats_blocked(q, 0.25, lambda lo, hi: CR.gap2_rows(q, radii, 0.25, lo, hi))
    assert np.array_equal(ct["idx"], g.argmin(1)) and np.array_equal(bits(ct["val"]), bits(g.min(1)))
    assert np.array_equal(ct["high"], N.highest_index_wins(g)) and np.array_equal(ct["later"], N.later_tile_wins(g))


def test_blocked_equals_chunked_past_six_tiles():
    """n = 5 120, 10 tiles: the fold over the chunks of every cut the GPU file uses is the blocked brute force."""
    n = W.FULL
    s, q, q2, k, radii = lattice(n)
    tiles = W.tiles_of(n)
    assert tiles == 10
    cuts = sorted({W.parts(j, n) for j in W.CUTS[n]})
    assert cuts == [1, 3, 7, 10]
    for pos, some in ((q, cuts), (q2, [7])):      # the moved lattice at the cut with chunks of one and of two tiles
        nn, ct = N.nearest_blocked(pos, 0.25), CR.contact_blocked(pos, radii, 0.25)
        for chunks in some:
            got = N.chunked(pos, 0.25, n, tiles, chunks)
            assert np.array_equal(got[0], nn[0]) and np.array_equal(bits(got[1]), bits(nn[1])), chunks
            got = CR.chunked(pos, radii, 0.25, n, tiles, chunks)
            assert np.array_equal(got[0], ct[0]) and np.array_equal(bits(got[1]), bits(ct[1])), chunks
    assert N.nearest_blocked(np.zeros((3, 1), np.int64), 0.25)[0][0] == -1
    assert np.isinf(CR.contact_blocked(np.zeros((3, 1), np.int64), np.zeros(1, np.float32), 0.25)[1][0])


# ------------------------------------------------------------------------------------------- 2. the lattice at the new sizes
def own_floor(n):
    """The floor under the share of rows whose tie crosses the border of the body's own tile.  A tie mate lies in the body's own
    tile with probability 511 / (n - 1) under the random order, so with the 4 mates a grid body has at the least the share is
    1 - (1 - 511 / (n - 1))^4: it falls with the tile count, whatever the lattice.  tests/test_nearest_host.py asserts 0.50 at
    2 049 and 2 561 and 0.30 at 4 609, three quarters of that figure (0.68, 0.59, 0.38); the same three quarters here."""
    return 0.75 * (1.0 - (1.0 - 511.0 / (n - 1)) ** 4)


@pytest.mark.parametrize("n", W.LATTICE_SIZES)
def test_dense_lattice_keeps_its_properties(n):
    """tests/test_nearest_host.py's test_dense_lattice_ties and test_dense_lattice_specials and tests/test_contact_host.py's
    test_dense_lattice_contacts, row-blocked.  Forming the rows runs the asserts that every r2, e, s and gap2 is exact in fp32."""
    s, q, q2, k, radii = lattice(n)
    assert own_floor(2049) >= 0.50 and own_floor(4609) >= 0.27
    st = N.tie_stats_blocked(q, 0.25, lambda lo, hi: N.r2_rows(q, 0.25, lo, hi))
    idx, r2 = st["idx"], st["val"]      # test_blocked_equals_unblocked: the winners of nearest_blocked
    idx2 = N.nearest_blocked(q2, 0.25)[0]
    frac = {f: float(np.mean(x)) for f, x in (("ties", st["cnt"] >= 2), ("span", st["span"] >= 2), ("own", st["own"]),
                                               ("high", st["high"] != idx), ("later", st["later"] != idx), ("shift", idx2 != idx))}
    print(f"n = {n} nearest: " + ", ".join(f"{f} {v:.3f}" for f, v in frac.items()) + f"; own floor {own_floor(n):.3f}")
    assert frac["ties"] >= 0.90 and frac["span"] >= 0.80
    assert frac["own"] >= own_floor(n) and st["own"].sum() >= 1000
    assert frac["high"] >= 0.90 and frac["later"] >= 0.90
    assert frac["shift"] >= 0.90, "a refresh that does nothing would not show"
    assert (idx >= 0).all() and (idx < n).all() and (idx != np.arange(n)).all() and (r2[idx] <= r2).all()
    # the specials
    assert q.min() >= 1 and q2.min() >= 1 and (q[:, 0] == 1).all() and r2[0] > 3.25 and 0 < idx[0] < n
    assert np.flatnonzero(idx == n - 1).tolist() == [N.DENSE_PARTNER] and idx[n - 1] == N.DENSE_PARTNER
    last = N.r2_rows(q, 0.25, n - 1, n)[0]
    assert (last == r2[n - 1]).sum() == 1 and (n - 1) // N.TILE == -(-n // N.TILE) - 1      # in the last tile that holds bodies
    for a, b in N.DENSE_PAIRS + ((13, n - 2),):
        assert idx[a] == b and idx[b] == a and r2[a] == r2[b] == np.float32(0.25)
    t = N.DENSE_TRIPLE
    assert (r2[list(t)] == np.float32(0.25)).all() and idx[t[0]] == t[1] and idx[t[1]] == t[0] and idx[t[2]] == t[0]
    for b in N.DENSE_MASSLESS:
        assert s["m"][b] == 0.0 and (idx == b).any()
    assert np.array_equal(np.sort(q2.T.tolist(), 0), np.sort(q.T.tolist(), 0)) and np.array_equal(q + k, q2)
    v = np.stack([s[f] for f in ("vx", "vy", "vz")]).astype(np.float64)
    assert np.array_equal(v * 2.0 ** -30, k) and np.abs(v).max() <= 2.0 ** 35
    assert np.array_equal(np.stack([s[f] for f in ("qx", "qy", "qz")]).astype(np.int64), q)
    # contact
    ct = N.tie_stats_blocked(q, 0.25, lambda lo, hi: CR.gap2_rows(q, radii, 0.25, lo, hi))
    cp, gap2 = ct["idx"], ct["val"]
    cp2 = CR.contact_blocked(q2, radii, 0.25)[0]
    assert not np.signbit(gap2[gap2 == 0]).any()
    sign = [float(np.mean(c)) for c in (gap2 < 0, gap2 == 0, gap2 > 0)]
    cfrac = {f: float(np.mean(x)) for f, x in (("ties", ct["cnt"] >= 2), ("not nearest", cp != idx), ("high", ct["high"] != cp),
                                                ("later", ct["later"] != cp), ("shift", cp2 != cp))}
    print(f"n = {n} contact: gap2 < 0 / == 0 / > 0: {sign[0]:.3f} / {sign[1]:.3f} / {sign[2]:.3f}; "
          + ", ".join(f"{f} {v:.3f}" for f, v in cfrac.items()))
    assert min(sign) >= 0.05
    assert cfrac["ties"] >= 0.20 and cfrac["not nearest"] >= 0.50 and cfrac["high"] >= 0.20
    assert cfrac["shift"] >= 0.90, "a refresh that does nothing would not show"
    assert (gap2[cp] <= gap2).all()


# ---------------------------------------------------------------------------------------------------- 3. the shape arithmetic
def test_sizes_and_tiles():
    import murbhip
    want = {W.FULL: (10, 0), W.ONE_IN_LAST: (10, 511), W.DEEP: (20, 1023), W.DEEPER: (26, 1023), 30000: (60, 720)}
    for n, (tiles, padding) in want.items():
        assert W.slots_of(n) == murbhip.slice_slots(n, 1) and W.tiles_of(n) == tiles and W.slots_of(n) - n == padding
    assert W.FULL % W.TILE == 0                                                      # a problem with no padding slot at all
    assert (W.ONE_IN_LAST - 1) % W.TILE == 0 and W.tiles_of(W.ONE_IN_LAST) == -(-W.ONE_IN_LAST // W.TILE)      # one body in the last tile
    for n in (W.DEEP, W.DEEPER):                                                     # one body in the last but one, the last padding only
        assert (n - 1) % W.TILE == 0 and (n - 1) // W.TILE == W.tiles_of(n) - 2
        assert all(W.masked(W.tiles_of(n) - 1, own, n) for own in range(W.tiles_of(n)))
        assert not W.masked(W.tiles_of(n) - 1, 0, n, padding=False)
    assert set(W.LATTICE_SIZES) == set(W.CUTS) and set(W.GALAXY_SIZES) == set(W.GALAXY_CUTS)
    assert set(W.WALK) <= set(W.CUTS[W.DEEP]) and W.WALK[0] == W.WALK[-1] == 32 and len(set(W.WALK)) == 4


def test_the_restated_rule_of_hermite_parts():
    """Forced: min(jsplit, tiles, 32).  "jsplit" 0 on 256 CUs: 1 chunk up to 15 tiles, then tiles / 8: the GPU file's default
    cuts of 2, 3 and 7 chunks.  The GPU file asserts the device's info("hermite_parts") against this rule with its own CU count."""
    assert [W.parts(j, W.FULL) for j in W.ALL_CUTS] == [1, 1, 3, 7, 10]
    assert [W.parts(j, W.DEEP) for j in W.ALL_CUTS] == [2, 1, 3, 7, 20]
    assert [W.parts(j, W.DEEPER) for j in W.CUTS[W.DEEPER]] == [3, 1, 26]
    assert [W.parts(j, 30000) for j in W.GALAXY_NEAREST_CUTS] == [7, 1, 32]
    for n, chunks in W.DEFAULT_CHUNKS.items():
        assert W.parts(0, n) == chunks, n
    assert {2, 3, 7} <= set(W.DEFAULT_CHUNKS.values())
    assert W.parts(0, 14 * 512) == 1 and W.parts(0, 14 * 512 + 1) == 2 and W.parts(0, 200000) == 3      # 12 544 groups: ceil(36 864 / 12 544)
    assert W.parts(0, W.DEEP, cus=8) == 2 and W.parts(0, W.DEEP, cus=4) == 1                          # a small chip: fewer workgroups wanted
    assert W.parts(0, 30000, cus=64) == 5
    for tiles, chunks in ((10, 3), (10, 7), (20, 7), (26, 3), (60, 7)):
        c = W.cut(tiles, chunks)
        assert c[0][0] == 0 and c[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(c, c[1:])) and all(hi > lo for lo, hi in c)
    assert W.cut(10, 3) == [(0, 3), (3, 6), (6, 10)] and [hi - lo for lo, hi in W.cut(10, 7)] == [1, 1, 2, 1, 2, 1, 2]
    assert [hi - lo for lo, hi in W.cut(60, 7)] == [8, 9, 8, 9, 8, 9, 9] and [hi - lo for lo, hi in W.cut(26, 3)] == [8, 9, 9]


def test_the_cases_hold_every_shape():
    """Over all (n, cut, i tile) of the lattice cases: what the GPU file is there for.  A wave exists for every i tile that
    holds bodies, and every row is compared, so every own tile listed here runs."""
    seen = set()
    longest = 0
    inside = set()
    for n in W.LATTICE_SIZES:
        body_tiles = -(-n // W.TILE)
        for jsplit in W.CUTS[n]:
            chunks = W.parts(jsplit, n)
            for own in range(body_tiles):
                for (t0, t1), st in zip(W.cut(W.tiles_of(n), chunks), W.stages(n, chunks, own)):
                    assert sum(len(x) for x in st) == t1 - t0 and all(len(x) == W.STAGE for x in st[:-1])
                    seen |= set(st[:-1]) | {("last " if len(st[-1]) == 1 else "") + st[-1]}
                    longest = max(longest, W.longest_unmasked_run(st))
                    if t1 - t0 >= 8 and t0 <= own < t1:
                        inside.add("first" if own == t0 else "last" if own == t1 - 1 else "inside")
                    if jsplit == 0 and chunks >= 2 and t0 <= own < t1:
                        seen.add(f"default {chunks}")
    print(sorted(seen), longest, sorted(inside))
    assert longest >= 5, "no chunk with 5 consecutive fully unmasked stages"
    assert {"UU", "UM", "MU", "MM", "last U", "last M"} <= seen
    assert inside == {"first", "last", "inside"}
    assert {"default 2", "default 3"} <= seen and W.parts(0, 30000) == 7
    # the same for the potential form, whose only masked tile is the own one: it sits first, last and inside a long chunk too
    pot = {st_ for n in W.LATTICE_SIZES for j in W.CUTS[n] for own in range(-(-n // W.TILE))
           for st in W.stages(n, W.parts(j, n), own, padding=False) for st_ in st}
    assert {"UU", "UM", "MU", "U", "M"} <= pot and "MM" not in pot
    # n = 9 217, one chunk, a wave of tile 7: 3 full stages, (U, M), 5 full stages, then the lone body's tile and the padding
    assert W.stages(W.DEEP, 1, 7) == [["UU", "UU", "UU", "UM", "UU", "UU", "UU", "UU", "UU", "MM"]]
    assert W.stages(W.DEEP, 2, 17) == [["UU"] * 5, ["UU", "UU", "UU", "UM", "MM"]]
    assert W.stages(W.FULL, 3, 2) == [["UU", "M"], ["UU", "U"], ["UU", "UU"]]
    assert W.stages(W.ONE_IN_LAST, 1, 0)[0] == ["MU", "UU", "UU", "UU", "UM"]
    # the galaxy of 30 000: 60 tiles, the last partly padding; the default cut has chunks of 8 and 9 tiles
    assert W.stages(30000, 7, 59)[-1] == ["UU", "UU", "UU", "UM", "M"] and W.stages(30000, 1, 0)[0][1:-1] == ["UU"] * 28
    cases = W.cases()
    assert max(c for _, _, c in cases) == 32 and {c for n, j, c in cases if j == 0} == {1, 2, 3, 7}


# --------------------------------------------------------------------------------------------------------- 4. the probes' power
def test_own_term_pair_in_tiles_7_and_17():
    """A sum that held the own term once misses the bound by 50 times and more, wherever the pair sits."""
    n = W.DEEP
    s, soft, (a, b) = PR.own_term_pair(n, W.OWN_PAIR_SLOTS)
    assert (a // PR.TILE, b // PR.TILE) == (7, 17) and len(s["m"]) == n and np.flatnonzero(s["m"]).tolist() == [a, b]
    for jsplit in W.OWN_PAIR_CUTS:      # the own tile lies strictly inside a chunk of 10 and of 20 tiles, and alone in one
        for own in (7, 17):
            (t0, t1), = [c for c in W.cut(W.tiles_of(n), W.parts(jsplit, n)) if c[0] <= own < c[1]]
            assert (t1 - t0 == 1) if jsplit == 32 else (t1 - t0 >= 10 and t0 < own < t1 - 1)
    phi = PR.phi_of(s, soft)
    g = float(H.G)
    pair, own = g * PR.OWN_MASS / np.sqrt(PR.OWN_SEP ** 2 + float(soft) ** 2), g * PR.OWN_MASS / float(soft)
    assert np.isclose(phi[a], pair, rtol=1e-6) and np.isclose(phi[b], pair, rtol=1e-6)
    lost = abs(float((np.float32(own) + np.float32(pair)) - np.float32(own)) - pair) / pair      # add, then subtract, in fp32
    print(f"own / pair = {own / pair:.3e}; adding and subtracting the own term in fp32 costs {lost:.2e}")
    assert lost >= 50 * PR.TOL_F64_MAX
    q = H._stack(s, PR.Q)
    rest = np.setdiff1d(np.arange(n), [a, b])
    assert (s["m"][rest] == 0).all() and phi[rest].min() > 0.0 and np.isfinite(np.float32(phi)).all()
    for k in (a, b):
        assert np.sqrt(((q[:, rest] - q[:, [k]]) ** 2).sum(0)).min() >= 1e13
    assert np.array_equal(PR.own_term_pair(514)[0]["qx"], PR.own_term_pair(514, PR.OWN_SLOTS)[0]["qx"])


def test_sparse_sources_over_every_tile():
    n = W.DEEP
    s, soft, src = PR.sparse(n, sources=W.SPARSE_SOURCES)
    assert np.array_equal(np.flatnonzero(s["m"]), src) and 48 <= len(src) <= W.SPARSE_SOURCES
    body_tiles = -(-n // PR.TILE)
    assert body_tiles == 19 and {int(x) // PR.TILE for x in src} == set(range(body_tiles))
    assert all(t * PR.TILE in src for t in range(body_tiles)) and all(t * PR.TILE + 511 in src for t in range(body_tiles - 1))
    assert n - 1 in src and (n - 1) % PR.TILE == 0
    share = PR.power(s, soft)
    need = PR.POWER_FACTOR * PR.TOL_F64_MAX
    print(f"sparse probe, {len(src)} sources: smallest share {share.min():.2e}, 1 % quantile {np.quantile(share, 0.01):.2e}, needs {need:.1e}")
    assert (share >= need).mean() >= 0.99
    phi = PR.phi_of(s, soft)
    assert np.float32(phi.max()) < 1e6 and np.float32(phi.min()) > 1e-3
    old = PR.sparse()      # the default is what it was
    assert len(old[2]) == 16 and old[2].tolist() == list(PR.SPARSE_SOURCES)


# ------------------------------------------------------------------------------------- 5. honest float32 and half the phi bound
def potential_inputs():
    """name -> (state, soft, cuts) of every potential case of the GPU file."""
    import murbhip
    out = {}
    for n in W.LATTICE_SIZES:
        out[f"lattice {n}"] = (lattice(n)[0], np.float32(0.5), W.CUTS[n])
    s, soft, _ = PR.own_term_pair(W.DEEP, W.OWN_PAIR_SLOTS)
    out["own pair"] = (s, soft, W.OWN_PAIR_CUTS)
    s, soft, _ = PR.sparse(W.DEEP, sources=W.SPARSE_SOURCES)
    out["sparse"] = (s, soft, W.CUTS[W.DEEP])
    for n in W.GALAXY_SIZES:
        out[f"galaxy {n}"] = (murbhip.init_bodies(n, "galaxy"), W.GALAXY_SOFT, W.GALAXY_CUTS[n])
    return out


@pytest.mark.parametrize("name", [f"lattice {n}" for n in W.LATTICE_SIZES] + ["own pair", "sparse"] + [f"galaxy {n}" for n in W.GALAXY_SIZES])
def test_float32_in_the_sweeps_order_meets_half_the_bound(name):
    """512 spread rows (the specials of full_wrap.spread_rows among them): numpy float32 in the full sweep's summation order
    (potential_ref.sweep_phi_f32) against potential_ref.phi_f64, for every cut of the case.  At most half of TOL_F64_MAX: the
    bound of the GPU file leaves the device's reciprocal square root and its own fold as much again."""
    s, soft, cuts = potential_inputs()[name]
    n = len(s["m"])
    rows = np.union1d(W.spread_rows(n, 500), W.OWN_PAIR_SLOTS if name == "own pair" else [])
    assert 500 <= len(rows) <= 512 and {0, n - 1, 511, 512} <= set(rows.tolist())
    want = PR.phi_of(s, soft, rows=rows)
    terms = PR.sweep_terms_f32(s, soft, rows, W.tiles_of(n))
    for jsplit in cuts:
        chunks = W.parts(jsplit, n)
        e = PR.rel_err(PR.sweep_phi_f32(terms, rows, chunks), want)
        print(f"{name}, \"jsplit\" {jsplit} ({chunks} chunks): float32 in the sweep's order is off by at most {e.max():.2e}")
        assert e.max() <= 0.5 * PR.TOL_F64_MAX, (name, jsplit)

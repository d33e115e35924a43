"""GPU: the FULL Hermite sweep (murb_force_jerk_sweep: murbhip_compute_acc_jerk, murbhip_step, murbhip_evolve) in its three
side-product forms — murb_nn_sweep_kernel, murb_contact_sweep_kernel, murb_force_jerk_pot_kernel — at 10, 20, 26 and 60 layout
tiles.  No other file runs them on more than 6: there a workgroup's stage loop makes 3 iterations at most, the library's own
cut is one chunk, and the own tile is never strictly inside a long chunk.  tests/helpers/full_wrap.py lists the shapes and
restates info("hermite_parts"); tests/test_full_wrap_host.py pins them (a chunk of 12 consecutive unmasked stages, the masked
tile first, last and inside a chunk, a padding-only tile, the default cuts of 2, 3 and 7 chunks).

Yardsticks, all written from include/murbhip.h and pinned on the CPU: nearest_ref / contact_ref's row-blocked exact searches on
the dense tie lattice (every value exact in fp32: indices equal, values equal as bits, no tolerance), before and after one
predictor step of 2^-30 that moves every body onto another body's cell; potential_ref's fp64 phi within TOL_F64_MAX = 2e-6;
nearest_ref's fp64 candidate sets on the galaxy; and bits against bits: (a, j) with and without the option at the same cut,
(index, value) across the cuts, evolve against step, one context walked through the cuts against fresh ones.

Worst phi error, relative to the fp64 phi (bound 2e-6), and beside it what numpy float32 in the sweep's summation order attains
on 512 spread rows (tests/test_full_wrap_host.py); per case the largest over its cuts:
    case                                        float32 emulation (CPU)     MI355X
    lattice n = 5 120   "jsplit" 0 1 3 7 32            1.96e-07            1.96e-07
    lattice n = 4 609   "jsplit" 0 1 3 7 32            1.71e-07            2.07e-07
    lattice n = 9 217   "jsplit" 0 1 3 7 32            2.37e-07            2.66e-07
    lattice n = 12 289  "jsplit" 0 1 32                2.11e-07            3.32e-07
    own pair in tiles 7 and 17, n = 9 217, 0 1 32      1.54e-07            2.11e-07
    sparse sources, n = 9 217, 0 1 3 7 32              2.10e-07            2.53e-07
    galaxy n = 12 289   "jsplit" 0 1 32                3.83e-07            5.42e-07
    galaxy n = 30 000   "jsplit" 0 1 (1 032 rows)      3.97e-07            3.82e-07
(the MI355X column: every row of the case but for the last line; the own pair's two heavy bodies 1.6e-08).  The galaxy's r2 at
n = 30 000 is within 1.75e-07 of the fp64 minimum on the 1 032 rows (bound 1e-6)."""
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

pytestmark = pytest.mark.gpu

TOL = PR.TOL_F64_MAX
Q, V = PR.Q, PR.V
DT = 2.0 ** -30                 # the step that carries q to q2
SOFT2 = 0.25                    # the lattice's softening, squared
LATTICE_CASES = [(n, j) for n in W.LATTICE_SIZES for j in W.CUTS[n]]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- inputs
@lru_cache(maxsize=None)
def lattice(n):
    """(state, soft, q, q2, radii, the state on q2) of the dense lattice: integer positions before and after the shift."""
    s, soft, q = N.dense_lattice(n)
    q2, _ = N.shifted(q)
    moved = dict(s)
    moved.update({k: q2[i].astype(np.float32) for i, k in enumerate(Q)})
    return s, soft, q, q2, CR.dense_radii(n), moved


@lru_cache(maxsize=None)
def reference(n, mode, moved):
    """(index, value) of the row-blocked restatement on q (moved False) or q2, computed once."""
    s, soft, q, q2, radii, _ = lattice(n)
    pos = q2 if moved else q
    return N.nearest_blocked(pos, SOFT2) if mode == "nearest" else CR.contact_blocked(pos, radii, SOFT2)


@lru_cache(maxsize=None)
def lattice_phi(n):
    s, soft = lattice(n)[:2]
    return PR.phi_of(s, soft)


@lru_cache(maxsize=None)
def own_pair():
    s, soft, slots = PR.own_term_pair(W.DEEP, W.OWN_PAIR_SLOTS)
    return s, soft, slots, PR.phi_of(s, soft)


@lru_cache(maxsize=None)
def sparse():
    s, soft, src = PR.sparse(W.DEEP, sources=W.SPARSE_SOURCES)
    return s, soft, src, PR.phi_of(s, soft)


_galaxy = {}


def galaxy(gpu, n):
    """(state, rows compared with fp64, their fp64 phi): all rows at 12 289, full_wrap.spread_rows at 30 000."""
    if n not in _galaxy:
        s = gpu.init_bodies(n, "galaxy")
        rows = np.arange(n) if n <= 12289 else W.spread_rows(n)
        _galaxy[n] = (s, rows, PR.phi_of(s, W.GALAXY_SOFT, rows=rows))
    return _galaxy[n]


# ------------------------------------------------------------------------------------------------------------------ contexts
OPTION = {"plain": None, "nearest": "nearest", "contact": "contact", "potential": "potential"}


def open_sim(gpu, s, soft, form, jsplit, radii=None):
    """A fresh Hermite context with the form's option set, "jsplit" set and the state uploaded; info("hermite_parts") is
    asserted against the restated rule with the device's own CU count, and the default cut against the table the shapes of
    this file were derived for."""
    n = len(s["m"])
    sim = gpu.Simulation(n, soft=soft)
    try:
        sim.set_option("integrator", 2)
        if OPTION[form]:
            sim.set_option(OPTION[form], 1)
        sim.set_option("jsplit", jsplit)
        check_parts(sim, n, jsplit)
        sim.upload(s)
        if form == "contact":
            sim.upload_radii(radii)
    except BaseException:
        sim.close()
        raise
    return sim


def check_parts(sim, n, jsplit):
    cus, got = int(sim.info("cu_count")), int(sim.info("hermite_parts"))
    assert int(sim.info("slots")) == W.slots_of(n)
    want = W.parts(jsplit, n, cus)
    assert got == want, f"n={n} \"jsplit\" {jsplit}: info(\"hermite_parts\") is {got}, the restated rule gives {want} on {cus} CUs"
    if jsplit == 0:
        assert got == W.DEFAULT_CHUNKS[n], \
            f"n={n}: the default cut is {got} chunks on {cus} CUs, this file's shapes assume {W.DEFAULT_CHUNKS[n]} (256 CUs)"
    return got


def forces(sim):
    return bits(np.stack(list(sim.acc()) + list(sim.jerk())))


def side(sim, form):
    """The form's side product as arrays that compare with array_equal: bits for the floats."""
    if form == "potential":
        return (bits(sim.potential()),)
    if form == "plain":
        return ()
    idx, val = sim.nearest() if form == "nearest" else sim.contact()
    return (idx, bits(val))


def assert_rows(got, want, what):
    """Indices equal and values equal as bits on every row; the message names the first rows that differ and where they lie."""
    bad = np.flatnonzero((got[0] != want[0]) | (bits(got[1]) != bits(want[1])))
    if len(bad):
        lines = [f"body {i} (tile {i // W.TILE}): got ({got[0][i]}, {got[1][i]!r}) in tile {got[0][i] // W.TILE}, want "
                 f"({want[0][i]}, {want[1][i]!r}) in tile {want[0][i] // W.TILE}" for i in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {len(want[0])} rows differ\n  " + "\n  ".join(lines))


def assert_phi(got, want, what, rows=None):
    """phi of `rows` (all by default; `want` holds those rows' fp64 values) within TOL; returns the largest error."""
    rows = np.arange(len(want)) if rows is None else np.asarray(rows)
    assert np.isfinite(got[rows]).all() and not np.signbit(got[rows]).any(), what
    e = PR.rel_err(got[rows], want)
    w = int(np.argmax(e))
    print(f"{what}: phi off by at most {e.max():.2e} of the fp64 value (bound {TOL:.0e}), body {rows[w]}")
    assert e.max() <= TOL, f"{what}: phi of body {rows[w]} (tile {rows[w] // W.TILE}, offset {rows[w] % W.TILE}) off by {e[w]:.3e}; {(e > TOL).sum()} bodies over"
    return float(e.max())


def assert_energy(got, s, want_phi, what):
    want = PR.energy_of(s, want_phi)
    err = abs(got - want) / abs(want)
    print(f"{what}: potential energy {got:.9e}, fp64 {want:.9e}, off by {err:.2e} (bound {TOL:.0e})")
    assert err <= TOL, what


# --------------------------------------------------------------------------------- a. nearest and contact on the lattice, exact
_across_cuts = {}      # (n, mode) -> ("jsplit", index, value bits before, index, value bits after the step) of the first cut that ran


@pytest.mark.parametrize("n,jsplit", LATTICE_CASES)
@pytest.mark.parametrize("mode", ["nearest", "contact"])
def test_lattice_exact(gpu, mode, n, jsplit):
    """Every row of the starting evaluation is the restatement's on q, every row after one step of 2^-30 the restatement's on
    q2; the forces do not change with the option; the bits do not change with the cut; at one cut per size the adaptive
    launch (a non-null control block) gives the step's bits."""
    s, soft, q, q2, radii, _ = lattice(n)
    with open_sim(gpu, s, soft, "plain", jsplit) as off:
        off.compute_acc_jerk()
        plain = forces(off)
    with open_sim(gpu, s, soft, mode, jsplit, radii) as sim:
        parts = int(sim.info("hermite_parts"))
        what = f"n={n} {mode} \"jsplit\" {jsplit} ({parts} chunks of {W.tiles_of(n)} tiles)"
        sim.compute_acc_jerk()
        got = side(sim, mode)
        a0, j0 = np.stack(sim.acc()), np.stack(sim.jerk())
        want = reference(n, mode, False)
        assert_rows((got[0], got[1].view(np.float32)), want, what + ", starting evaluation")
        if mode == "nearest":      # r2(i, j) == r2(j, i) bit for bit: a body's neighbour has a neighbour at most as far
            r2 = got[1].view(np.float32)
            assert (r2[got[0]] <= r2).all(), what
        assert np.array_equal(forces(sim), plain), what + ": the forces changed with the option"
        qp, _ = H.predict(H._stack(s, Q), H._stack(s, V), a0, j0, DT)
        assert np.array_equal(bits(qp.astype(np.float32)), bits(q2.astype(np.float32))), what + ": the predictor does not land on q2"
        sim.step(DT)
        moved = side(sim, mode)
        want2 = reference(n, mode, True)
        assert_rows((moved[0], moved[1].view(np.float32)), want2, what + ", after the step")
        if mode == "nearest":
            r2 = moved[1].view(np.float32)
            assert (r2[moved[0]] <= r2).all(), what
        assert np.mean(moved[0] != got[0]) >= 0.9, what + ": the step changed too few winners"
    first = _across_cuts.setdefault((n, mode), (jsplit,) + got + moved)
    assert all(np.array_equal(x, y) for x, y in zip(got + moved, first[1:])), what + f": the bits differ from those of \"jsplit\" {first[0]}"
    if jsplit == (W.EVOLVE_CUT if W.EVOLVE_CUT in W.CUTS[n] else 0):
        with open_sim(gpu, s, soft, mode, jsplit, radii) as sim:
            out = sim.evolve(DT, dt_min=DT, dt_max=DT, max_steps=1)
            assert out["steps"] == 1 and out["time"] == DT and out["dt_min"] == out["dt_max"] == DT
            again = side(sim, mode)
        assert all(np.array_equal(x, y) for x, y in zip(again, moved)), what + ": evolve differs from step"


# ------------------------------------------------------------------------------------------------------------- b. potential
def potential_case(gpu, s, soft, jsplit, want, what, rows=None, energy=True):
    """One potential case: phi of `rows` against `want` and the energy within TOL, (a, j) those of "potential" 0 at the same
    cut, a step of dt = 0 keeps phi's bits, a second fresh context gives the same bits.  Returns the largest phi error."""
    with open_sim(gpu, s, soft, "plain", jsplit) as off:
        off.compute_acc_jerk()
        plain = forces(off)
    seen = []
    for k in range(2):
        with open_sim(gpu, s, soft, "potential", jsplit) as sim:
            sim.compute_acc_jerk()
            phi = sim.potential()
            seen.append(bits(phi))
            if k:
                continue
            w = sim.potential_energy()
            assert np.array_equal(forces(sim), plain), what + ": the forces changed with the option"
            sim.step(0.0)
            assert np.array_equal(bits(sim.potential()), bits(phi)), what + ": a step of dt = 0 changed phi"
            worst = assert_phi(phi, want, what, rows)
            if energy:
                assert_energy(w, s, want, what)
    assert np.array_equal(seen[0], seen[1]), what + ": two fresh contexts give different bits"
    return worst


@pytest.mark.parametrize("n,jsplit", LATTICE_CASES)
def test_potential_lattice(gpu, n, jsplit):
    s, soft = lattice(n)[:2]
    potential_case(gpu, s, soft, jsplit, lattice_phi(n), f"lattice n={n} \"jsplit\" {jsplit} ({W.parts(jsplit, n)} chunks)")


@pytest.mark.parametrize("jsplit", W.OWN_PAIR_CUTS)
def test_potential_own_term_inside_a_long_chunk(gpu, jsplit):
    """Two bodies of 1e30 kg in tiles 7 and 17 of 20, everything else massless: the own tile lies strictly inside a chunk of 10
    or 20 tiles, or alone in one.  A sum that held the own term once misses the bound 50 times (tests/test_full_wrap_host.py)."""
    s, soft, (a, b), want = own_pair()
    what = f"own pair \"jsplit\" {jsplit}"
    potential_case(gpu, s, soft, jsplit, want, what + ": all")
    with open_sim(gpu, s, soft, "potential", jsplit) as sim:
        sim.compute_acc_jerk()
        assert_phi(sim.potential(), want[[a, b]], what + ": the two", rows=[a, b])


@pytest.mark.parametrize("jsplit", W.CUTS[W.DEEP])
def test_potential_sparse_sources_in_every_tile(gpu, jsplit):
    """Sources in all 19 body-holding tiles of n = 9 217, every tile's first and last slot among them, everything else massless: one
    lost or doubled term is far above the bound on every body (the power is asserted in tests/test_full_wrap_host.py)."""
    s, soft, src, want = sparse()
    potential_case(gpu, s, soft, jsplit, want, f"sparse \"jsplit\" {jsplit}")


@pytest.mark.parametrize("n,jsplit", [(n, j) for n in W.GALAXY_SIZES for j in W.GALAXY_CUTS[n]])
def test_potential_galaxy(gpu, n, jsplit):
    """n = 12 289: all rows and the energy.  n = 30 000 (60 tiles, the default cut 7 chunks): 1 032 spread rows, no energy."""
    s, rows, want = galaxy(gpu, n)
    potential_case(gpu, s, W.GALAXY_SOFT, jsplit, want, f"galaxy n={n} \"jsplit\" {jsplit} ({W.parts(jsplit, n)} chunks)",
                   rows=rows, energy=len(rows) == n)


# ------------------------------------------------------------------------------------------------- c. nearest on the galaxy
def assert_candidates(idx, r2, q, soft2, rows, what):
    """tests/test_nearest_gpu.py's check on `rows`: every index lies in the fp64 candidate set of its body (within a relative
    1e-6 of the minimum) and r2 is within 1e-6 of the fp64 minimum."""
    n = q.shape[1]
    q64 = q.astype(np.float64)
    assert ((idx >= 0) & (idx < n) & (idx != np.arange(n))).all(), what + ": an index is out of range or the body itself"
    worst = 0.0
    for lo in range(0, len(rows), 256):
        r = rows[lo:lo + 256]
        d = q64[:, None, :] - q64[:, r, None]
        d2 = (d * d).sum(0) + float(soft2)
        d2[np.arange(len(r)), r] = np.inf
        best = d2.min(1)
        assert (d2[np.arange(len(r)), idx[r]] <= best * (1.0 + 1e-6)).all(), what + ": an index is not among the nearest bodies"
        worst = max(worst, float((np.abs(r2[r].astype(np.float64) - best) / best).max()))
    print(f"{what}: largest relative r2 error {worst:.3e} on {len(rows)} rows")
    assert worst <= 1e-6, what


def test_nearest_galaxy_30000(gpu):
    """60 layout tiles, the last but one partly padding, the last padding only, in 7 chunks (the default), 1 and 32."""
    n = 30000
    s, rows, _ = galaxy(gpu, n)
    q = np.stack([s[k] for k in Q])
    first = None
    for jsplit in W.GALAXY_NEAREST_CUTS:
        what = f"galaxy n={n} nearest \"jsplit\" {jsplit}"
        with open_sim(gpu, s, W.GALAXY_SOFT, "plain", jsplit) as off:
            off.compute_acc_jerk()
            plain = forces(off)
        with open_sim(gpu, s, W.GALAXY_SOFT, "nearest", jsplit) as sim:
            sim.compute_acc_jerk()
            idx, r2 = sim.nearest()
            assert np.array_equal(forces(sim), plain), what + ": the forces changed with the option"
        assert (r2[idx] <= r2).all(), what
        if first is None:
            first = (idx, bits(r2))
            assert_candidates(idx, r2, q, float(W.GALAXY_SOFT) ** 2, rows, what)
        assert np.array_equal(idx, first[0]) and np.array_equal(bits(r2), first[1]), what + ": the bits differ from those of the first cut"


# ---------------------------------------------------------------------------------- d. one context, many shapes: stale rows
_fresh = {}


def fresh(gpu, form, jsplit):
    """(side product, forces) of a fresh context's starting evaluation of the n = 9 217 lattice at that cut, once."""
    if (form, jsplit) not in _fresh:
        s, soft, q, q2, radii, _ = lattice(W.DEEP)
        with open_sim(gpu, s, soft, form, jsplit, radii) as sim:
            sim.compute_acc_jerk()
            _fresh[form, jsplit] = (side(sim, form), forces(sim))
    return _fresh[form, jsplit]


@pytest.mark.parametrize("form", ["nearest", "contact", "potential"])
def test_one_context_walks_the_cuts(gpu, form):
    """ONE context at n = 9 217 goes through "jsplit" 32, 1, 7, 0, 32: 20, 1, 7, 2, 20 partial rows a body.  The rows are not
    cleared: before every measured evaluation the context evaluates another state (the lattice on q2; doubled positions for the
    potential), so a row of a longer earlier cut that is folded in shows as a wrong minimum or sum.  Every measured result
    carries the bits of a fresh context at that cut."""
    s, soft, q, q2, radii, moved = lattice(W.DEEP)
    stale = W.doubled(s) if form == "potential" else moved
    with open_sim(gpu, s, soft, form, W.WALK[0], radii) as sim:
        for k, jsplit in enumerate(W.WALK):
            sim.set_option("jsplit", jsplit)
            parts = check_parts(sim, W.DEEP, jsplit)
            what = f"{form}, stop {k} of the walk, \"jsplit\" {jsplit} ({parts} chunks)"
            sim.upload(stale)
            sim.compute_acc_jerk()
            dirty = side(sim, form)
            sim.upload(s)
            sim.compute_acc_jerk()
            want_side, want_forces = fresh(gpu, form, jsplit)
            got = side(sim, form)
            assert not all(np.array_equal(x, y) for x, y in zip(dirty, got)), what + ": the other state gives the same result"
            for x, y in zip(got, want_side):
                bad = np.flatnonzero(x != y)
                assert len(bad) == 0, what + f": {len(bad)} rows differ from a fresh context's, first {bad[:6]} (tiles {bad[:6] // W.TILE})"
            assert np.array_equal(forces(sim), want_forces), what + ": (a, j) differ from a fresh context's"


# -------------------------------------------------------------------------------- e. the forms share the rows' fourth floats
def test_the_forms_follow_each_other_in_one_context(gpu):
    """One context at n = 9 217, the default cut: nearest, off, contact (with radii), off, potential, off.  Each evaluation
    carries the bits of a fresh context of that form; the last plain (a, j) those of a context that never had an option."""
    s, soft, q, q2, radii, _ = lattice(W.DEEP)
    with open_sim(gpu, s, soft, "plain", 0) as sim:
        for k, form in enumerate(("nearest", "plain", "contact", "plain", "potential", "plain")):
            for option in ("nearest", "contact", "potential"):
                sim.set_option(option, 0)
            if OPTION[form]:
                sim.set_option(OPTION[form], 1)
            if form == "contact":
                sim.upload_radii(radii)
            check_parts(sim, W.DEEP, 0)
            sim.compute_acc_jerk()
            want_side, want_forces = fresh(gpu, form, 0)
            what = f"stop {k}, {form}"
            for x, y in zip(side(sim, form), want_side):
                bad = np.flatnonzero(x != y)
                assert len(bad) == 0, what + f": {len(bad)} rows differ from a fresh context's, first {bad[:6]} (tiles {bad[:6] // W.TILE})"
            assert np.array_equal(forces(sim), want_forces), what + ": (a, j) differ from a fresh context's"

"""CPU: the yardstick of the per-body potential (tests/helpers/potential_ref.py) on cases with known answers, the power of the
probes the GPU tests use, and the new entry points of the built libraries and the Python interface."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import hermite_ref as H       # noqa: E402
import potential_ref as PR    # noqa: E402

E_INVALID = -2000
G = float(H.G)
M1, M2 = 2.0 ** 34, 2.0 ** 35      # exact in fp32


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# ------------------------------------------------------------------------------------------------------------- known answers
def test_two_bodies():
    s = PR.state([[0.0, 3.0], [0.0, 4.0], [0.0, 0.0]], [M1, M2])
    phi = PR.phi_of(s, 0.0)
    assert np.allclose(phi, [G * M2 / 5.0, G * M1 / 5.0], rtol=1e-12, atol=0.0)
    soft = 12.0      # r^2 + soft^2 = 169
    assert np.allclose(PR.phi_of(s, soft), [G * M2 / 13.0, G * M1 / 13.0], rtol=1e-12, atol=0.0)
    assert np.isclose(PR.energy_of(s, phi), -G * M1 * M2 / 5.0, rtol=1e-12)


def test_two_coincident_bodies_count_for_each_other():
    s = PR.state([[7.0, 7.0], [1.0, 1.0], [2.0, 2.0]], [M1, M2])
    assert np.allclose(PR.phi_of(s, 0.5), [G * M2 / 0.5, G * M1 / 0.5], rtol=1e-12, atol=0.0)


def test_lone_body():
    phi = PR.phi_of(PR.state([[1.0], [2.0], [3.0]], [M1]), 0.5)
    assert phi.shape == (1,) and phi[0] == 0.0 and not np.signbit(phi[0])
    assert PR.rel_err(np.zeros(1, np.float32), phi)[0] == 0.0 and PR.rel_err(np.ones(1, np.float32), phi)[0] == np.inf


def test_massless_body_has_a_phi_and_adds_to_nobodys():
    s = PR.state([[0.0, 3.0, 0.0], [0.0, 4.0, 12.0], [0.0, 0.0, 0.0]], [M1, M2, 0.0])
    phi = PR.phi_of(s, 0.0)
    pair = PR.phi_of(PR.state([[0.0, 3.0], [0.0, 4.0], [0.0, 0.0]], [M1, M2]), 0.0)
    assert np.array_equal(phi[:2], pair)
    assert np.isclose(phi[2], G * M1 / 12.0 + G * M2 / np.sqrt(9.0 + 64.0), rtol=1e-12)
    _, mn = PR.phi_of(s, 0.0, want_min=True)      # the smallest term looks at massive bodies only
    assert np.allclose(mn, [G * M2 / 5.0, G * M1 / 5.0, min(G * M1 / 12.0, G * M2 / np.sqrt(73.0))], rtol=1e-12)
    rows = PR.phi_of(s, 0.0, rows=[2, 0])
    assert np.array_equal(rows, phi[[2, 0]])


# -------------------------------------------------------------------------------------------------------------- the probes
@pytest.mark.parametrize("n", [2, 514])
def test_own_term_probe(n):
    """The own term is 1e4 x the pair term, so a sum that held it once has lost the pair term's low 13 bits: up to 6e-4 (half
    an ulp of the own term over the pair term), 1e-4 for these very numbers."""
    s, soft, (a, b) = PR.own_term_pair(n)
    phi = PR.phi_of(s, soft)
    pair, own = G * PR.OWN_MASS / np.sqrt(PR.OWN_SEP ** 2 + float(soft) ** 2), G * PR.OWN_MASS / float(soft)
    assert np.isclose(phi[a], pair, rtol=1e-6) and np.isclose(phi[b], pair, rtol=1e-6)
    assert own / pair == pytest.approx(1e4, rel=1e-3)
    lost = abs(float((np.float32(own) + np.float32(pair)) - np.float32(own)) - pair) / pair     # add, then subtract, in fp32
    print(f"n={n}: own / pair = {own / pair:.3e}; adding and subtracting the own term in fp32 costs {lost:.2e}")
    assert lost > 10 * PR.TOL_F64_MAX
    if n > 2:
        q = H._stack(s, PR.Q)
        rest = np.setdiff1d(np.arange(n), [a, b])
        assert (s["m"][rest] == 0).all() and phi[rest].min() > 0.0
        for k in (a, b):
            assert np.sqrt(((q[:, rest] - q[:, [k]]) ** 2).sum(0)).min() >= 1e13
        assert a // PR.TILE != b // PR.TILE


@pytest.mark.parametrize("pair", PR.COINCIDENT_PAIRS)
def test_coincident_probe(pair):
    s, soft = PR.coincident(pair)
    a, b = pair
    q, gm = H._stack(s, PR.Q), H._gm(s)
    assert np.array_equal(q[:, a], q[:, b]) and np.array_equal(q, np.round(q))
    phi = PR.phi_of(s, soft)
    apart = PR.phi_of(s, soft) - np.where(np.arange(len(gm)) == a, gm[b], np.where(np.arange(len(gm)) == b, gm[a], 0.0)) / float(soft)
    # each has the other's G m / soft, and that term is far above the bound: leaving it out shows
    assert gm[b] / float(soft) >= 1e3 * PR.TOL_F64_MAX * phi[a] and gm[a] / float(soft) >= 1e3 * PR.TOL_F64_MAX * phi[b]
    assert apart[a] > 0.0 and apart[b] > 0.0


def test_sparse_probe_has_power():
    """For at least 99 % of the bodies the smallest source term is 10 x the bound times phi_i: a lost or doubled term shows."""
    s, soft, src = PR.sparse()
    assert len(src) == 16 and len(s["m"]) == 2049 and (np.flatnonzero(s["m"]) == src).all()
    tiles = set(int(x) // PR.TILE for x in src)
    assert tiles == set(range(5)) and all(t * PR.TILE in src for t in range(5)) and all(t * PR.TILE + 511 in src for t in range(4))
    share = PR.power(s, soft)
    need = PR.POWER_FACTOR * PR.TOL_F64_MAX
    print(f"sparse probe: smallest share {share.min():.2e}, 1 % quantile {np.quantile(share, 0.01):.2e}, needs {need:.1e}")
    assert (share >= need).mean() >= 0.99
    phi = PR.phi_of(s, soft)
    assert np.isfinite(phi).all() and (phi > 0).all()
    assert np.float32(phi.max()) < 1e6 and np.float32(phi.min()) > 1e-3      # G m / r of order 1: far inside fp32's normal range


# ------------------------------------------------------------------------------------------------------------ entry points
def test_potential_entry_points_are_exported(mh):
    header = open(os.path.join(ROOT, "include", "murbhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = set(re.findall(r" T (murbhip_[a-z_0-9]+)", nm.stdout))
    for name in ("murbhip_download_potential", "murbhip_potential_energy"):
        assert name in exported, name + " not exported by libmurbhip.so"
        assert name in mh.EXPORTS, name + " missing from murbhip.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " not declared in include/murbhip.h"
        assert hasattr(mh.lib(), name)
    assert mh.lib().murbhip_version() == 103
    # the argument checks that need no device: no context
    phi, w = np.zeros(4, np.float32), C.c_double()
    assert mh.lib().murbhip_download_potential(None, phi.ctypes.data_as(C.POINTER(C.c_float))) == E_INVALID
    assert mh.lib().murbhip_potential_energy(None, C.byref(w)) == E_INVALID


def test_python_interface_has_the_methods(mh):
    for method in ("potential", "potential_energy"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.potential)
    for name in ("murbhost_sim_set_potential", "murbhost_sim_potential"):
        assert hasattr(mh.host_lib(), name)
    with pytest.raises(ValueError):      # the three Hermite tags only; checked before anything touches a device
        mh.HostSim(64, integrator=1, potential=True)
    with pytest.raises(ValueError):
        mh.HostSim(64, integrator=4, potential=True, contact=True)

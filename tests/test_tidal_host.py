"""CPU: the yardstick of the tidal read-out (tests/helpers/tidal_ref.py) against an independent derivation (central differences
of the field yardstick's acceleration) and against the trace identity, the float32 emulation behind the bound, the new entry
points of the built libraries and the Python interface, and the sweep kernel's code-object metadata."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import code_object as CO      # noqa: E402
import field_ref as F         # noqa: E402
import hermite_ref as H       # noqa: E402
import potential_ref as PR    # noqa: E402
import tidal_ref as T         # noqa: E402

E_INVALID = -2000
G = float(H.G)
SIZES = (2, 63, 513, 2049)


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("n", SIZES)
def test_reference_is_the_gradient_of_the_field(n):
    """Central differences of field_ref.field_f64's acceleration in fp64, step h = 1e-6, at midpoints of body pairs: column b of
    T is (a(p + h e_b) - a(p - h e_b)) / 2h.  All nine differences agree with tidal_f64's six components (so the differences are
    symmetric too) within 1e-7 of the scaling sum.  The truncation error falls as h^2 (measured: 4.6e-9 at most); 1e-7 is 20 x it."""
    s = F.system(n)
    p = F.midpoints(s, 33)[0].astype(np.float64)
    t, ab, _ = T.tidal_f64(p, None, s, F.SOFT)
    want = T.matrix(t)
    h = 1e-6
    worst = 0.0
    for b in range(3):
        e = np.zeros((3, 1))
        e[b] = h
        hi = F.field_f64(p + e, None, None, s, F.SOFT, want_abs=False)[0]
        lo = F.field_f64(p - e, None, None, s, F.SOFT, want_abs=False)[0]
        col = (hi - lo) / (2.0 * h)      # (3, P): d a_a / d p_b for a = 0, 1, 2
        worst = max(worst, float((np.abs(col - want[:, :, b].T) / ab).max()))
    print(f"n={n}: central differences against tidal_f64: {worst:.2e} of the scaling sum")
    assert worst <= 1e-7


@pytest.mark.parametrize("n", SIZES)
def test_trace_identity(n):
    """tr T = -3 soft^2 sum G m inv^5 in fp64, to 1e-12 relative to the scaling sum (at far points the trace itself is 1e-10 of
    it: fp64 resolves no more), with the usual softening and with soft = 2^-20."""
    s = F.system(n)
    for name, p, soft in (("midpoints", F.midpoints(s, 33)[0], F.SOFT), ("far", F.far_points(33)[0], F.SOFT),
                          ("midpoints, soft 2^-20", F.midpoints(s, 33)[0], np.float32(2.0 ** -20))):
        ref = T.tidal_f64(p, None, s, soft)
        e = T.trace_errors(ref[0], ref)
        print(f"n={n} {name}: trace off by {e.max():.2e} of the scaling sum")
        assert e.max() <= 1e-12
        assert (ref[2] < 0).all()


def test_known_answers():
    """One body of G m = 1 at the origin, soft 0, a point at (2, 0, 0): T = diag(2, -1, -1) / 8 (stretch along the line to the
    body, compression across); with the body skipped, nothing; a second body on the first counts; T is the gradient of the
    acceleration with its sign: a = -p / |p|^3 gives d a_x / d x = 2 / |p|^3."""
    m = 1.0 / G      # rounded to float32 in the state: the answers hold to 1e-6
    s = PR.state([[0.0], [0.0], [0.0]], [m])
    p = np.array([[2.0], [0.0], [0.0]])
    t, ab, tr = T.tidal_f64(p, None, s, 0.0)
    assert np.allclose(t[:, 0], [0.25, -0.125, -0.125, 0, 0, 0], rtol=1e-6, atol=1e-12) and tr[0] == 0.0
    assert np.isclose(ab[0], np.sqrt(6.0) / 8.0, rtol=1e-6)
    t, ab, tr = T.tidal_f64(p, [0], s, 0.0)
    assert not t.any() and ab[0] == 0.0
    two = PR.state([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [m, m])
    t, ab, tr = T.tidal_f64(p, [0], two, 0.0)
    assert np.allclose(t[:, 0], [0.25, -0.125, -0.125, 0, 0, 0], rtol=1e-6, atol=1e-12)
    q = np.array([[1.0], [2.0], [2.0]])      # r = 3: off-diagonals 3 d_a d_b / r^5
    t, _, _ = T.tidal_f64(q, None, s, 0.0)
    assert np.allclose(t[:, 0], np.array([3 - 9, 12 - 9, 12 - 9, 6, 6, 12]) / 243.0, rtol=1e-6)
    assert np.allclose(np.linalg.eigvalsh(T.matrix(t)[0]), np.array([-1, -1, 2]) / 27.0, rtol=1e-6)


def test_float32_emulation_and_bound():
    """The float32 emulation attains a few 2^-24 of the scaling sum, so the bounds land between 10 and 40; and a single body's
    term off (nobody skipped where one should be, or the reverse) misses the bound by two orders of magnitude: the bound has
    power."""
    for n in SIZES:
        s = F.system(n)
        for name, (p, _, skip) in (("bodies", F.body_points(s, np.arange(33) % n)), ("midpoints", F.midpoints(s, 33)), ("far", F.far_points(33))):
            ref, c = T.bound_of(p, skip, s, F.SOFT)
            print(f"n={n} {name}: C = {c:.2f}")
            assert 4.0 < c < 100.0, (n, name, c)
            assert T.check(T.tidal_f32(p, skip, s, F.SOFT), ref, c, f"n={n} {name}") <= c / 4 + 1e-9      # a quarter of the bound by construction
            if n >= 63:
                wrong = T.tidal_f64(p, None if skip is not None else np.zeros(33, np.int64), s, F.SOFT)[0]      # one body's term off
                assert T.scaled_errors(wrong, ref).max() > 100 * c * T.U24


# -------------------------------------------------------------------------------------------------------------- entry points
def test_tidal_entry_points_are_exported(mh):
    """include/murbtidal.h, the binding's list and the library's exports name the same two entry points, disjoint from the other
    two interfaces' lists; a NULL context is refused without a device."""
    header = open(os.path.join(ROOT, "include", "murbtidal.h")).read()
    declared = sorted(re.findall(r"^int (murbtidal_\w+)\(", header, re.M))
    assert declared == ["murbtidal_at", "murbtidal_of"] == sorted(mh.TIDAL_EXPORTS)
    assert '#include "murbhip.h"' in header
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbtidal_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    for name in declared:
        assert hasattr(mh.lib(), name)
    assert not set(mh.TIDAL_EXPORTS) & (set(mh.EXPORTS) | set(mh.FIELD_EXPORTS))
    assert mh.lib().murbhip_version() == 103
    assert mh.lib().murbtidal_at(None, 0, *([None] * 10)) == E_INVALID
    assert mh.lib().murbtidal_of(None, 0, *([None] * 7)) == E_INVALID
    # the span kind is documented in the header, and among murbhip_get_info's kinds
    assert "span_tidal_ms_avg" in header and "span_tidal_count" in header
    assert re.search(r"field \| tidal \(compute stream", open(os.path.join(ROOT, "include", "murbhip.h")).read())


def test_python_interface_has_the_methods(mh):
    for method in ("tidal_at", "tidal_of"):
        assert callable(getattr(mh.Simulation, method))
    assert callable(mh.HostSim.tidal_at) and callable(mh.tidal_matrix)
    assert hasattr(mh.host_lib(), "murbhost_sim_tidal_at")
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint tidalAt\(", hpp)
    d = {k: np.arange(2, dtype=np.float32) + i for i, k in enumerate(mh.TIDAL_KEYS)}
    m = mh.tidal_matrix(d)
    assert m.shape == (2, 3, 3) and np.array_equal(m, np.swapaxes(m, 1, 2))
    assert np.array_equal(m[1], np.array([[1, 4, 5], [4, 2, 6], [5, 6, 3]], np.float32))
    assert np.array_equal(m, T.matrix(T.stack(d)))


# --------------------------------------------------------------------------------------------------------------- code object
def test_tidal_kernel_resources():
    """Code-object metadata of a fresh gfx950 build: exactly one murb_tidal_sweep_kernel, 0 bytes of scratch, 0 spilled
    registers, and at most 128 vector registers (the 4 waves per SIMD it is built for); the field sweep is still there once."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_tidal_sweep_kernel")
    assert len(kernels) == 1, "murb_tidal_sweep_kernel missing from the code object, or there twice"
    (name, num), = kernels.items()
    print(name, num)
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128, "no longer fits 4 waves per SIMD"
    assert len(CO.metadata(r"murb_force_field_kernel")) == 1
    rows = CO.metadata(r"murb_tidal_rows_kernel")
    assert len(rows) == 1 and all(v["private_segment_fixed_size"] == 0 for v in rows.values())

"""CPU: the oracle restatement against the REAL reference.  The reference's side of every comparison comes from its
compiled CPU path (oracle/_ref/libmurbref.so) where that was built, and otherwise from the same results recorded from it
(tests/golden/ref_vs_oracle.npz, written by tests/golden/make_golden.py with record() below): bit patterns as SHA-256
digests, the arrays of the comparisons with a tolerance as they are."""
import hashlib
import os

import numpy as np
import pytest

SOFT, DT = np.float32(2e8), np.float32(3600.0)
RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vs_oracle.npz")
SCHEMES = ("galaxy", "random")
INIT_NS = (1, 2, 63, 1000, 2049)
INTEGRATE = (("galaxy", np.float32(3600.0)), ("random", np.float32(0.01)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def digest(a):
    return hashlib.sha256(bits(a).tobytes()).hexdigest()


def integrator_acc(n=1234):
    return (np.linspace(-3, 7, n, dtype=np.float32), np.full(n, 1e-3, np.float32), np.linspace(5, -5, n, dtype=np.float32))


def write_tab(path, n=70000):
    """A synthetic `milkyway_andromeda.tab`: one body per non-empty line, an empty line every 1000 bodies."""
    rng = np.random.default_rng(11)
    rows = rng.normal(size=(n, 7)).astype(np.float32)
    rows[:, 0] = np.abs(rows[:, 0]) * 1e-5
    with open(path, "w") as f:
        for k, r in enumerate(rows):
            f.write(" ".join(f"{x:.9g}" for x in r) + "\n")
            if k % 1000 == 0:
                f.write("\n")                      # empty lines are skipped
    return rows


def record(O, workdir):
    """The reference's side of every test below, computed by the compiled reference (O.have_ref() must hold)."""
    out = {}
    for scheme in SCHEMES:
        for n in INIT_NS:
            r = O.RefSim("cpu+optim", n, scheme)
            out[f"init_{scheme}_{n}_padding"] = np.array([r.padding])
            for k, a in r.state(with_padding=True).items():
                out[f"init_{scheme}_{n}_{k}"] = np.array(digest(a))
            r.close()
        r = O.RefSim("cpu+optim", 1500, scheme, SOFT, DT)
        for step in range(3):
            r.step(1)
            for c, a in zip("xyz", r.acc()):
                out[f"optim_{scheme}_{step}_a{c}"] = np.array(digest(a))
            for k, a in r.state().items():
                out[f"optim_{scheme}_{step}_{k}"] = np.array(digest(a))
        r.close()
    r = O.RefSim("cpu+naive", 700, "random", SOFT, DT)
    r.step(2)
    for k in ("qx", "qy", "qz"):
        out["naive_" + k] = r.state()[k]
    r.close()
    for scheme, dt in INTEGRATE:
        for k, a in O.ref_integrate(1234, scheme, integrator_acc(), dt, 3).items():
            out[f"integrate_{scheme}_{k}"] = np.array(digest(a))
    for tag in ("cpu+optim", "cpu+simd", "cpu+omp"):
        r = O.RefSim(tag, 1024, "galaxy")
        r.step(1)
        for c, a in zip("xyz", r.acc()):
            out[f"acc1024_{tag}_a{c}"] = a
        r.close()
    write_tab(os.path.join(workdir, "milkyway_andromeda.tab"))
    here = os.getcwd()
    os.chdir(workdir)
    try:
        r = O.RefSim("cpu+naive", 5, "collision")    # n is replaced by the number of lines
    finally:
        os.chdir(here)
    out["file_n"], out["file_padding"] = np.array([r.n]), np.array([r.padding])
    for k, a in r.state().items():
        out["file_" + k] = np.array(digest(a))
    r.close()
    return out


@pytest.fixture(scope="module")
def ref(O, tmp_path_factory):
    if O.have_ref():
        O.ref_lib()
        return record(O, str(tmp_path_factory.mktemp("reference")))
    with np.load(RECORDING) as g:
        return {k: g[k] for k in g.files}


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
@pytest.mark.parametrize("n", [1, 2, 63, 1000, 2049])
def test_init_bit_exact(ref, O, scheme, n):
    got = O.init_bodies(n, scheme, with_padding=True)
    assert int(ref[f"init_{scheme}_{n}_padding"][0]) == O.padding(n)
    for k in O.FIELDS:
        assert digest(got[k]) == str(ref[f"init_{scheme}_{n}_{k}"]), k


@pytest.mark.parametrize("scheme", ["galaxy", "random"])
def test_optim_bit_exact_over_steps(ref, O, scheme):
    n = 1500
    s = O.init_bodies(n, scheme)
    for step in range(3):
        acc = O.simulate(s, 1, "cpu+optim", SOFT, DT)
        for c, a in zip("xyz", acc):
            assert digest(a) == str(ref[f"optim_{scheme}_{step}_a{c}"]), (step, c)
        for k in O.FIELDS[:6]:
            assert digest(s[k]) == str(ref[f"optim_{scheme}_{step}_{k}"]), (step, k)


def test_naive_close(ref, O):
    n = 700
    s = O.init_bodies(n, "random")
    O.simulate(s, 2, "cpu+naive", SOFT, DT)
    for k in ("qx", "qy", "qz"):
        np.testing.assert_allclose(s[k], ref["naive_" + k], rtol=1e-5)


def test_integrator_bit_exact(ref, O):
    n = 1234
    acc = integrator_acc(n)
    for scheme, dt in INTEGRATE:
        s = O.init_bodies(n, scheme)
        for _ in range(3):
            O.integrate(s, acc, dt)
        for k in O.FIELDS[:6]:
            assert digest(s[k]) == str(ref[f"integrate_{scheme}_{k}"]), (scheme, k)


def test_simd_and_omp_are_speed_baselines_only(ref, O):
    """cpu+simd / cpu+omp use a 12-bit rsqrt (SimulationNBodySIMD.cpp:12-32): ~8e-4 from cpu+optim."""
    opt = [ref[f"acc1024_cpu+optim_a{c}"] for c in "xyz"]
    for tag in ("cpu+simd", "cpu+omp"):
        e = O.rel_err([ref[f"acc1024_{tag}_a{c}"] for c in "xyz"], opt)
        assert 1e-5 < e.max() < 5e-3


def test_file_scheme_matches_reference(ref, O, tmp_path, monkeypatch):
    """Any scheme other than galaxy/random reads `milkyway_andromeda.tab` from the working directory
    (Bodies.cpp:14-25, 83-153; the file itself is not in the reference repository): one body per non-empty
    line, rescaled by component galaxy.  A synthetic 70 000-line file reaches five of the six index ranges;
    the product's host mirror must produce the reference's arrays bit for bit, and both must refuse a
    missing file."""
    import murbhip
    n = 70000
    rows = write_tab(tmp_path / "milkyway_andromeda.tab", n)
    monkeypatch.chdir(tmp_path)
    assert int(ref["file_n"][0]) == n and int(ref["file_padding"][0]) == 0
    got = murbhip.init_bodies(n, "collision")
    for k in O.FIELDS:
        assert digest(got[k]) == str(ref["file_" + k]), k
    assert np.all(got["r"] == np.float32(1e5))
    # Milky Way ranges use 4.5e10 / 4.0 / 220, Andromeda ranges 9.4e10 / 6.0 / 260
    assert got["m"][0] == np.float32(np.float64(rows[0, 0]) * 4.5e10) and got["qx"][20000] == np.float32(np.float64(rows[20000, 1]) * 6.0)
    assert got["vz"][66000] == np.float32(np.float64(rows[66000, 6]) * 260)

"""CPU: the massless tracers' entry points in the built libraries and the Python interface, the refusals that need no device,
the fp64 restatement (tests/helpers/tracer_ref.py) and its order of convergence, and the sweep kernel's code object."""
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
import tracer_ref as T        # noqa: E402

E_INVALID = -2000
_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def mh():
    import murbhip
    murbhip.lib()
    return murbhip


# -------------------------------------------------------------------------------------------------------------- entry points
def test_tracer_entry_points_are_exported(mh):
    """include/murbtracer.h, the binding's list and the library's exports name the same entry points with the declared
    signatures; the options are documented where they are set; murbhip.h's and murbfield.h's interfaces are what they were."""
    header = open(os.path.join(ROOT, "include", "murbtracer.h")).read()
    declared = sorted(re.findall(r"^int (murbtracer_\w+)\(", header, re.M))
    assert declared == sorted(mh.TRACER_EXPORTS) and len(declared) == 9
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.normpath(mh.LIB_PATH)], capture_output=True, text=True)
    exported = sorted(re.findall(r" T (murbtracer_[a-z_0-9]+)", nm.stdout))
    assert exported == declared, set(exported) ^ set(declared)
    for key in mh.TRACER_OPTIONS:
        assert re.search(r'^ \*   "%s" ' % key, header, re.M), key
    assert not set(mh.TRACER_EXPORTS) & (set(mh.EXPORTS) | set(mh.FIELD_EXPORTS) | set(mh.TIDAL_EXPORTS))
    # the declared parameter lists, by count and kind
    params = {name: [p.strip() for p in args.split(",")] for name, args in
              re.findall(r"^int (murbtracer_\w+)\(([^;]*?)\);", header, re.M | re.S)}
    assert [p.split()[0] for p in params["murbtracer_upload"]] == ["murbhip_ctx*", "unsigned"] + ["const"] * 6
    assert len(params["murbtracer_download"]) == 7 and len(params["murbtracer_download_forces"]) == 7
    assert len(params["murbtracer_compute"]) == 1 and len(params["murbtracer_clear"]) == 1 and len(params["murbtracer_count"]) == 2
    assert len(params["murbtracer_set_option"]) == 3 and len(params["murbtracer_get_option"]) == 3
    for name, args in params.items():
        assert len(getattr(mh.lib(), name).argtypes) == len(args), name
    # "Not covered" and the state rules are written where the others' are
    for words in ("Not covered:", "block steps", "several shards", "tracers with mass", "A refused call changes nothing"):
        assert words in header, words


def test_calls_without_a_context_are_refused(mh):
    L = mh.lib()
    v, n = C.c_long(), C.c_ulong()
    assert L.murbtracer_upload(None, 0, *([None] * 6)) == E_INVALID
    assert L.murbtracer_download(None, *([None] * 6)) == E_INVALID
    assert L.murbtracer_download_forces(None, *([None] * 6)) == E_INVALID
    assert L.murbtracer_compute(None) == E_INVALID and L.murbtracer_clear(None) == E_INVALID
    assert L.murbtracer_count(None, C.byref(n)) == E_INVALID
    assert L.murbtracer_set_option(None, b"tracer_dt", 1) == E_INVALID
    assert L.murbtracer_get_option(None, b"tracer_dt", C.byref(v)) == E_INVALID


def test_upload_arguments_are_checked_on_the_host(mh):
    """murbtracer_validate is murbtracer_upload's argument check without a device: NULL position arrays, some but not all
    velocity pointers NULL, a value that is not finite."""
    L = mh.lib()
    a = [np.linspace(0, 1, 5, dtype=np.float32) + k for k in range(6)]
    p = [x.ctypes.data_as(_fp) for x in a]
    assert L.murbtracer_validate(5, *p) == 0
    assert L.murbtracer_validate(5, *p[:3], None, None, None) == 0
    assert L.murbtracer_validate(0, *([None] * 6)) == 0, "count 0 clears: no array is read"
    for k in range(3):
        q = list(p)
        q[k] = None
        assert L.murbtracer_validate(5, *q) == E_INVALID, f"position array {k} NULL"
    for missing in ((3,), (4,), (5,), (3, 4), (4, 5), (3, 5)):
        q = [None if k in missing else x for k, x in enumerate(p)]
        assert L.murbtracer_validate(5, *q) == E_INVALID, f"velocity pointers {missing} NULL alone"
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            b = [x.copy() for x in a]
            b[k][4] = bad
            assert L.murbtracer_validate(5, *[x.ctypes.data_as(_fp) for x in b]) == E_INVALID, (k, bad)
            assert L.murbtracer_validate(4, *[x.ctypes.data_as(_fp) for x in b]) == 0, "only `count` values are read"


def test_python_layer_refuses_without_a_device(mh):
    """Simulation.upload_tracers and HostSim(tracers=) raise for what the header refuses before any device call: the checks are
    host-side (a Simulation made without its constructor has no context to call)."""
    sim = object.__new__(mh.Simulation)
    sim._h = C.c_void_p()
    good = np.zeros((3, 4), np.float32)
    bad = good.copy()
    bad[1, 2] = np.nan
    with pytest.raises(mh.MurbHipError) as e:
        sim.upload_tracers(bad)
    assert e.value.code == E_INVALID
    with pytest.raises(mh.MurbHipError) as e:
        sim.upload_tracers(good, bad)
    assert e.value.code == E_INVALID
    with pytest.raises(ValueError):
        sim.upload_tracers(good[:2])
    with pytest.raises(ValueError):
        sim.upload_tracers(good, good[:, :3])
    with pytest.raises(mh.MurbHipError) as e:
        sim.upload_tracers(good)          # valid arrays, no context
    assert e.value.code == E_INVALID
    for call in (sim.tracers, sim.tracer_forces, sim.compute_tracers, sim.clear_tracers, lambda: sim.set_tracer_option("tracer_dt", 1)):
        with pytest.raises(mh.MurbHipError) as e:
            call()
        assert e.value.code == E_INVALID
    sim._h = C.c_void_p()                 # nothing for __del__ to destroy
    with pytest.raises(ValueError):
        mh.HostSim(64, integrator=0, tracers=(good, None))
    with pytest.raises(ValueError):
        mh.HostSim(64, integrator=4, tracers=(good, None))
    with pytest.raises(mh.MurbHipError):
        mh.HostSim(64, integrator=2, tracers=(bad, None))


def test_python_interface_has_the_methods(mh):
    for method in ("upload_tracers", "tracers", "tracer_forces", "compute_tracers", "clear_tracers", "set_tracer_option",
                   "tracer_option", "tracer_count"):
        assert callable(getattr(mh.Simulation, method)), method
    assert callable(mh.HostSim.tracers)
    for name in ("murbhost_sim_set_tracers", "murbhost_sim_get_tracers"):
        assert hasattr(mh.host_lib(), name)
    hpp = open(os.path.join(ROOT, "nbody-eurohpc_amd", "host", "implem", "SimulationNBodyHIP.hpp")).read()
    assert re.search(r"\bint setTracers\(", hpp) and re.search(r"\bint getTracers\(", hpp)


def test_host_logic_compiles_without_a_device():
    """csrc/murb_tracer.h is plain C++: g++ checks it alone."""
    src = os.path.join(ROOT, "nbody-eurohpc_amd", "csrc", "murb_tracer.h")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_is_the_bodies_for_a_massless_body():
    """A tracer and a massless body from the same state feel the same bodies: the two fp64 restatements agree to rounding (the
    body's sum holds its own exact-zero term), and with state32 the tracer's predictor and corrector have the body's bits
    given the same forces."""
    s = F.system(63)
    s = {k: v.copy() for k, v in s.items()}
    s["m"][62] = 0.0
    tq = np.stack([s[k][62:63] for k in T.Q]).astype(np.float64)
    tv = np.stack([s[k][62:63] for k in T.V]).astype(np.float64)
    body = H.hermite_f64(s, 5, T.SOFT, T.DT)
    _, q, v = T.run(s, tq, tv, 5, T.SOFT, T.DT)
    for k, c in enumerate(T.Q):
        assert abs(q[k, 0] - body[c][62]) <= 1e-13 * max(1.0, abs(body[c][62])), c
    for k, c in enumerate(T.V):
        assert abs(v[k, 0] - body[c][62]) <= 1e-13 * max(1e-3, abs(body[c][62])), c


def _kepler_errors(run_one, dts, period):
    out = []
    for dt in dts:
        steps = int(round(period / 4 / dt))
        x, y = run_one(dt, steps)
        t = steps * float(np.float32(dt))
        w = 2.0 * np.pi / period
        out.append(np.hypot(x - np.cos(w * t), y - np.sin(w * t)))
    return out


def test_restatement_converges_at_fourth_order():
    """A circular Kepler orbit about one body (G m = 1, r = 1, softening 1e-8: its effect on the force is 1e-16), a quarter
    period at dt, dt / 2, dt / 4: the error ratios of the tracer restatement against those of hermite_ref's own integrator
    carrying the same particle as a massless BODY.  The band comes from the body integrator: its ratios must sit within a
    factor 1.25 of 2^4 (the scheme's order; the next term of the error expansion is of relative size dt^2 = 1e-4 here), and
    the tracer's ratios within 1 % of the body's (the two are the same arithmetic up to fp64 rounding of sums of size 1, which
    is 1e-16 against errors of 1e-9 and more)."""
    state, tq, tv, period = T.kepler()
    soft = 1e-8
    dts = [period / 4 / 64, period / 4 / 128, period / 4 / 256]
    dts = [float(np.float32(d)) for d in dts]

    def as_tracer(dt, steps):
        _, q, _ = T.run(state, tq, tv, steps, soft, dt)
        return q[0, 0], q[1, 0]

    two = {k: np.array([state[k][0], (tq if k in T.Q else tv)[(T.Q + T.V).index(k) % 3, 0]]) for k in T.Q + T.V}
    two["m"] = np.array([state["m"][0], 0.0])

    def as_body(dt, steps):
        out = H.hermite_f64(two, steps, soft, dt)
        return out["qx"][1], out["qy"][1]

    eb = _kepler_errors(as_body, dts, period)
    et = _kepler_errors(as_tracer, dts, period)
    rb = [eb[0] / eb[1], eb[1] / eb[2]]
    rt = [et[0] / et[1], et[1] / et[2]]
    print("body errors", eb, "ratios", rb, "tracer errors", et, "ratios", rt)
    for r in rb:
        assert 16 / 1.25 <= r <= 16 * 1.25, f"hermite_ref's own integrator is not 4th order here: {rb}"
    for a, b in zip(rt, rb):
        assert abs(a - b) <= 0.01 * b, f"tracer ratios {rt} outside the band of the body integrator's {rb}"


# --------------------------------------------------------------------------------------------------------------- code object
def test_tracer_sweep_code_object():
    """Code-object metadata of a fresh gfx950 build (the method of test_field_host.py): murb_tracer_sweep_kernel<4, 4, 2> is
    there with 0 bytes of scratch, no spilled register and at most 128 vector registers (4 waves per SIMD), and its packed
    arithmetic is the plain Hermite sweep's, instruction for instruction; its loop, one basic block, holds 26 packed
    instructions (counted, six of them subtractions) and 2 v_rsq_f32 per pair of interactions, against the field kernel's 28."""
    assert CO.hipcc(), "hipcc is needed: the library itself is built with it"
    kernels = CO.metadata(r"murb_tracer_sweep_kernel")
    assert len(kernels) == 1, "murb_tracer_sweep_kernel missing from the code object"
    (name, num), = kernels.items()
    print(name, num)
    assert "ILi4ELi4ELi2EE" in name
    assert num["private_segment_fixed_size"] == 0 and num["vgpr_spill_count"] == 0 and num["sgpr_spill_count"] == 0
    assert num["vgpr_count"] <= 128, "no longer fits 4 waves per SIMD"
    for other, meta in CO.metadata(r"murb_tracer_\w+_kernel").items():
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, other

    def counts(kernel):
        ops = [re.sub(r"_e(32|64)$", "", op) for op in CO.ops(kernel, r"^\s*(v_pk_\w+|v_rsq_f32\w*)\b")]
        return {k: ops.count(k) for k in set(ops)}, CO.body(kernel)

    plain, _ = counts("murb_force_jerk_kernel")
    mine, body = counts(name)
    print("plain sweep", plain, "tracer sweep", mine)
    pairs = plain["v_rsq_f32"] // 2          # pairs of interactions of the unrolled tile: 4 lane steps x 4 points
    assert pairs == 16 and mine["v_rsq_f32"] == 2 * pairs, "one copy of the loop, nothing behind it"
    assert mine["v_pk_mul_f32"] == plain["v_pk_mul_f32"] and mine["v_pk_fma_f32"] == plain["v_pk_fma_f32"]
    assert mine["v_pk_add_f32"] == plain["v_pk_add_f32"], "the folds' additions beside the loop's, no more"
    # the loop itself, counted: the one basic block that branches back to its own label and holds every v_rsq_f32
    blocks = re.split(r"^(\.LBB\d+_\d+):", body, flags=re.M)
    loops = [code for label, code in zip(blocks[1::2], blocks[2::2])
             if "v_rsq_f32" in code and re.search(r"s_cbranch_\w+\s+" + re.escape(label) + r"\s*$", code, re.M)]
    assert len(loops) == 1, "the sweep's loop is one basic block"
    in_loop = {op: len(re.findall(r"^\s*" + op + r"(_e32|_e64)?\s", loops[0], re.M))
               for op in ("v_rsq_f32", "v_pk_mul_f32", "v_pk_fma_f32", "v_pk_add_f32")}
    print("in the loop", in_loop)
    assert in_loop["v_rsq_f32"] == 2 * pairs and in_loop["v_pk_mul_f32"] == mine["v_pk_mul_f32"] and in_loop["v_pk_fma_f32"] == mine["v_pk_fma_f32"]
    packed = in_loop["v_pk_mul_f32"] + in_loop["v_pk_fma_f32"] + in_loop["v_pk_add_f32"]
    assert packed == 26 * pairs and in_loop["v_pk_add_f32"] == 6 * pairs, "26 packed instructions per pair of interactions, six of them subtractions"
    assert len(re.findall(r"^\s*v_pk_\w+", loops[0], re.M)) == packed, "a packed instruction of another kind in the loop"
    assert not re.search(r"\bscratch_|\bbuffer_", body)

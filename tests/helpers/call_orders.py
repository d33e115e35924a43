"""Call orders of a context: which calls may change a later result, and sequences that check it (include/murbhip.h, "Call
orders").

The contract, in the header's words: calls are body-changing, observers or refused.  C1: deleting every observer and every
refused call from a sequence changes no bit of anything read afterwards.  C2: an observer returns the bits it returns when it
is the only observer at that point.  C3: a refused call returns its documented code and changes nothing.  Everything here is
differential, bit for bit, between two contexts of one build: run() interprets a sequence on a murbhip.Simulation and returns a
record, twin() and solo() derive the sequences it is compared with, family_f / family_k / family_h generate the sequences.

Pure Python: numpy alone is imported, the Simulation is handed in.  tests/test_call_orders_host.py pins the table against the
header and the generators' counts and coverage; tests/test_call_orders_gpu.py runs them."""
import struct
from collections import namedtuple

import numpy as np

E_INVALID, E_STATE = -2000, -2001

# ------------------------------------------------------------------------------------------------------------ classification
# Every entry point of include/murbhip.h in exactly one class.
FUNCTIONS = {
    "host_only": ("murbhip_version", "murbhip_error_string", "murbhip_partition", "murbhip_slice_slots", "murbhip_slot_of_body",
                  "murbhip_schedule_items", "murbhip_schedule_layout"),
    "life_cycle": ("murbhip_device_count", "murbhip_create", "murbhip_create_sharded", "murbhip_unique_id", "murbhip_create_rank",
                   "murbhip_destroy"),
    "body_changing": ("murbhip_upload", "murbhip_init_bodies", "murbhip_upload_radii", "murbhip_step", "murbhip_steps",
                      "murbhip_evolve", "murbhip_evolve_block", "murbhip_integrate_host_acc", "murbhip_block_set_levels",
                      "murbhip_set_encounter"),      # set_encounter(r) put back by (0) before the next body change: an observer
    "observer": ("murbhip_compute_acc", "murbhip_compute_acc_jerk", "murbhip_energy", "murbhip_moments", "murbhip_potential_energy",
                 "murbhip_download_mass", "murbhip_download_state", "murbhip_download_acc", "murbhip_download_jerk",
                 "murbhip_download_nearest", "murbhip_download_contact", "murbhip_download_potential", "murbhip_block_state",
                 "murbhip_evolve_dts", "murbhip_encounters", "murbhip_contacts", "murbhip_sync", "murbhip_warmup", "murbhip_get_info"),
    "by_key": ("murbhip_set_option",),               # OPTION_KEYS says which
}
# Every key of murbhip_set_option in exactly one class.  A value-changing set of a "plan" key drops the remembered forces and
# pair potential (C4) and of a "result" key changes later results in its own documented way: both are body-changing calls.  A
# value-changing set of a "neutral" key is an observer.
OPTION_KEYS = {
    "plan": ("variant", "jsplit", "taper", "sym_pass_mb", "diag_tri", "sym_red", "sym_waves", "sym_wide", "pad_aware", "tri_div",
             "xcd_order", "overlap", "tri_first_pct", "fuse_integrate"),
    "result": ("integrator", "block_units", "nearest", "contact", "potential", "exchange_p2p", "cu_reserve", "solo_shard",
               "force_exchange"),
    "neutral": ("energy_sweep", "profile", "evolve_batch", "init_libm_fma"),
}

# ------------------------------------------------------------------------------------------------------------------ operations
# kind: "M" body-changing, "O" observer, "R" refused (args[0] = the code it must return).  name: a key of CALLS.
Op = namedtuple("Op", "kind name args")


def M(name, *args):
    return Op("M", name, args)


def Obs(name, *args):
    return Op("O", name, args)


def R(code, name, *args):
    return Op("R", name, (code,) + args)


KMAX = 3                                  # murbhip_evolve_block of the sequences: blocks of 8 ticks
BLOCK_OPS = ("block", "block_open", "block_resume")


def _option_arrays(sim, ctx):
    o = ctx.get("option")
    if o == "nearest":
        return sim.nearest()
    if o == "contact":
        return sim.contact()
    if o == "potential":
        return sim.potential(), sim.potential_energy()
    raise KeyError("no sweep option in this configuration")


def _upload(sim, ctx):
    sim.upload(ctx["s"])                  # closes a block the sequence before left open
    if ctx.get("radii") is not None:      # the contact configuration: every sequence starts from the same radii
        sim.upload_radii(ctx["radii"])


def _int0_step(sim, ctx):
    sim.set_option("integrator", 0)
    sim.step(ctx["dt"])
    sim.set_option("integrator", 2)


def _set_then(key, value, then):
    def call(sim, ctx):
        sim.set_option(key, value)
        return then(sim, ctx)
    return call


def _pair(first, then):
    def call(sim, ctx):
        getattr(sim, first)()
        return then(sim, ctx)
    return call


def _profile_info(sim, ctx):
    sim.set_option("profile", 1)
    return sim.info("force_launches")


def _contact_121(sim, ctx):
    sim.set_option("contact", 2)
    sim.set_option("contact", 1)


def _encounter_r0(sim, ctx):
    sim.set_encounter(ctx["enc_r"])
    sim.set_encounter(0.0)


def _block(**kw):
    return lambda sim, ctx: sim.evolve_block(ctx["dt_max"], blocks=1, kmax=KMAX, **kw)


CALLS = {
    # body-changing
    "upload": _upload,
    "init_bodies": lambda sim, ctx: sim.init_bodies("random", 1),
    "step": lambda sim, ctx: sim.step(ctx["dt"]),
    "steps": lambda sim, ctx: sim.steps(ctx["dt"], 2),
    "evolve": lambda sim, ctx: sim.evolve(ctx["T"], max_steps=3),
    "block": _block(),
    "block_open": _block(max_steps=2),
    "block_resume": _block(),
    "set_levels": lambda sim, ctx: sim.set_block_levels(ctx["levels"], KMAX),
    "upload_radii": lambda sim, ctx: sim.upload_radii(ctx["radii2"]),
    "host_acc": lambda sim, ctx: sim.integrate_host_acc(ctx["host_acc"], ctx["dt"]),
    "int0_step": _int0_step,
    "set": lambda sim, ctx, key, value: sim.set_option(key, value),
    # observers
    "compute_acc": lambda sim, ctx: sim.compute_acc(),
    "acc_pair": _pair("compute_acc", lambda sim, ctx: sim.acc()),
    "caj": lambda sim, ctx: sim.compute_acc_jerk(),
    "caj_acc_jerk": _pair("compute_acc_jerk", lambda sim, ctx: (sim.acc(), sim.jerk())),
    "caj_option": _pair("compute_acc_jerk", _option_arrays),
    "option": _option_arrays,
    "energy": lambda sim, ctx: sim.energy(),
    "energy0": _set_then("energy_sweep", 0, lambda sim, ctx: sim.energy()),
    "energy1": _set_then("energy_sweep", 1, lambda sim, ctx: sim.energy()),     # leaves the option at 1: every energy names its own
    "moments": lambda sim, ctx: sim.moments(),
    "state": lambda sim, ctx: sim.state(),
    "masses": lambda sim, ctx: sim.masses(),
    "warmup": lambda sim, ctx: sim.warmup(1.0),
    "sync": lambda sim, ctx: sim.sync(),
    "profile_info": _profile_info,
    "acc": lambda sim, ctx: sim.acc(),
    "jerk": lambda sim, ctx: sim.jerk(),
    "block_state": lambda sim, ctx: sim.block_state(),
    "block_info": lambda sim, ctx: tuple(sim.info(k) for k in ("block_steps", "block_body_steps", "block_clamped", "block_max_active")),
    "evolve_dts": lambda sim, ctx: sim.evolve_dts(),
    "hits": lambda sim, ctx: (sim.encounters(), sim.contacts()),
    "contact_121": _contact_121,
    "encounter_r0": _encounter_r0,
    # calls that must be refused
    "evolve_bad": lambda sim, ctx: sim.evolve(-1.0),
    "block_bad": lambda sim, ctx: sim.evolve_block(ctx["dt_max"], kmax=21),
    "block_other_dt": lambda sim, ctx: sim.evolve_block(2.0 * ctx["dt_max"], blocks=1, kmax=KMAX),
    "block_other_kmax": lambda sim, ctx: sim.evolve_block(ctx["dt_max"], blocks=1, kmax=KMAX + 1),
    "set_encounter": lambda sim, ctx, r: sim.set_encounter(r),
    "radii_nan": lambda sim, ctx: sim.upload_radii(np.full(sim.n, np.nan, np.float32)),
}


def freeze(x):
    """A value as something `==` compares bit for bit (floats by their bytes: -0.0 != 0.0, NaN == NaN)."""
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, freeze(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(freeze(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return struct.pack("<d", float(x))
    if isinstance(x, np.integer):
        return int(x)
    raise TypeError(type(x))


def _names(seq, names):
    return any(op.kind == "M" and op.name in names for op in seq)


def read_end(sim, seq, ctx, open_block):
    """The end read-out.  State first, except under leapfrog, where murbhip_download_state is itself an evaluation and comes last."""
    integrator = ctx["integrator"]
    end = {}
    if integrator != 1:
        end["state"] = sim.state()
    if integrator == 2:
        if not open_block:
            sim.compute_acc_jerk()
        end["acc"], end["jerk"] = sim.acc(), sim.jerk()
        if ctx.get("option"):
            end["option"] = _option_arrays(sim, ctx)
        if _names(seq, BLOCK_OPS + ("set_levels",)):
            end["block_state"] = sim.block_state()
        if _names(seq, BLOCK_OPS):
            end["block_info"] = CALLS["block_info"](sim, ctx)
        if _names(seq, ("evolve",)):
            end["evolve_dts"] = sim.evolve_dts()
        if _names(seq, BLOCK_OPS + ("evolve",)):
            end["hits"] = CALLS["hits"](sim, ctx)
    if not open_block:
        sim.set_option("energy_sweep", 0)
        end["energy"] = sim.energy()
        end["moments"] = sim.moments()
    if integrator == 1:
        end["state"] = sim.state()
    return end


def run(sim, seq, ctx, error=Exception):
    """Interpret `seq` on `sim`.  The record: "values" {position: an observer's value}, "refused" {position: (name, code wanted,
    code got; 0 = it was not refused)}, "outs" [(name, what the body-changing call returned)], "raw_outs" the same unfrozen,
    "end" the end read-out, "open" whether it ended inside a block.  `error`: murbhip.MurbHipError."""
    rec = {"values": {}, "refused": {}, "outs": [], "raw_outs": [], "open": False}
    for pos, op in enumerate(seq):
        call = CALLS[op.name]
        if op.kind == "R":
            try:
                call(sim, ctx, *op.args[1:])
                got = 0
            except error as e:
                got = e.code
            rec["refused"][pos] = (op.name, op.args[0], got)
        elif op.kind == "O":
            rec["values"][pos] = freeze(call(sim, ctx, *op.args))
        else:
            out = call(sim, ctx, *op.args)
            rec["outs"].append((op.name, freeze(out)))
            rec["raw_outs"].append((op.name, out))
            rec["open"] = op.name in BLOCK_OPS and not out["synchronised"]
    rec["end"] = {k: freeze(v) for k, v in read_end(sim, seq, ctx, rec["open"]).items()}
    return rec


def twin(seq):
    """The sequence without its observers and refused calls."""
    return [op for op in seq if op.kind == "M"]


def solo(seq):
    """{position of an observer: the twin plus that observer alone}."""
    return {i: [op for j, op in enumerate(seq) if op.kind == "M" or j == i] for i, o in enumerate(seq) if o.kind == "O"}


def differing(a, b):
    """Names of the end read-out's entries (and "outs") in which two records differ."""
    keys = sorted(set(a["end"]) | set(b["end"]))
    outs = [[o for o in r["outs"] if o[0] != "set"] for r in (a, b)]      # a set_option returns nothing
    return [k for k in keys if a["end"].get(k) != b["end"].get(k)] + (["outs"] if outs[0] != outs[1] else [])


def diagnose(seq, twin_rec, run_solo):
    """Used only when a comparison failed: rerun the sequence with each observer alone (run_solo(sequence) -> record) and name
    those that break the end read-out on their own."""
    bad = []
    for pos, alone in solo(seq).items():
        d = differing(run_solo(alone), twin_rec)
        if d:
            bad.append(f"{pos}:{describe(seq[pos])} alone changes {d}")
    return bad or ["no observer breaks it alone: an interaction of several, or a refused call that was not"]


def describe(op):
    return op.name + ("(" + ", ".join(str(a) for a in op.args) + ")" if op.args else "")


def show(seq):
    return " ; ".join(("" if op.kind == "M" else op.kind.lower() + ":") + describe(op) for op in seq)


# ---------------------------------------------------------------------------------------------------------------- family F
# Force plans under "integrator" 0 and 1.
UPLOAD, STEP = M("upload"), M("step")
F_OBSERVERS = (Obs("acc_pair"), Obs("energy0"), Obs("energy1"), Obs("moments"), Obs("state"), Obs("masses"), Obs("warmup"),
               Obs("sync"), Obs("profile_info"))
F_PREFIXES = ((UPLOAD,), (UPLOAD, STEP))      # the second leaves half-step velocities on the device under leapfrog
F_INTEGRATORS = (0, 1)
MULTIPASS_N = 4097    # "variant" 8 with "sym_pass_mb" 1: the smallest n with info("sym_passes") >= 2, read on an MI355X (4 096: 1)
# id, n, devices, options before the upload, info keys the plan must show
F_CONFIGS = (
    ("sym5", 4609, None, {}, {"variant": 8, "world": 1}),
    ("fused3", 2049, None, {}, {"variant": 1, "jsplit": 1, "world": 1}),
    ("shards3_overlap1", 6151, (0, 0, 0), {"variant": 8, "overlap": 1}, {"variant": 8, "world": 3}),
    ("shards3_overlap2", 6151, (0, 0, 0), {"variant": 8, "overlap": 2}, {"variant": 8, "world": 3}),
    ("shards2_onesided", 6151, (0, 0), {"variant": 1}, {"variant": 1, "world": 2}),
    ("multipass", MULTIPASS_N, None, {"variant": 8, "sym_pass_mb": 1}, {"variant": 8, "world": 1, "sym_passes": 2}),
)


def family_f():
    """prefix, o1, o2, step, step for both prefixes and every ordered pair of observers, (o, o) included."""
    return [list(prefix) + [o1, o2, STEP, STEP] for prefix in F_PREFIXES for o1 in F_OBSERVERS for o2 in F_OBSERVERS]


# ---------------------------------------------------------------------------------------------------------------- family K
# Plan keys (C4).  Per configuration its entries (key, value set, options in force beside it).  Where the automatic value of a
# key is not exposed two values are listed whose plans differ from each other, so that at least one differs from the automatic
# one (setting the automatic value itself changes nothing and passes trivially): "diag_tri" and "sym_red" have no third value;
# for "jsplit", "sym_waves", "taper", "tri_first_pct" and "tri_div" tests/test_call_orders_host.py compares the two layouts
# with murbhip_schedule_layout, and tests/test_call_orders_gpu.py asserts from get_info that the plan moved wherever it is
# exposed (K_VISIBLE).  "taper" and "tri_div" cut items finer: under the automatic 16 sub-blocks per block the items are at
# their finest already and neither changes anything, so they run with "jsplit" 2 in force.
COARSE = {"jsplit": 2}
K_SINGLE = (("variant", 1, {}), ("jsplit", 2, {}), ("jsplit", 4, {}), ("taper", 0, COARSE), ("taper", 100, COARSE), ("diag_tri", 0, {}),
            ("diag_tri", 1, {}), ("sym_red", 0, {}), ("sym_red", 1, {}), ("sym_waves", 4, {}), ("sym_waves", 8, {}), ("sym_pass_mb", 1, {}),
            ("pad_aware", 0, {}), ("xcd_order", 1, {}), ("sym_wide", 1, {}))
K_SHARDED = K_SINGLE + (("overlap", 0, {}), ("overlap", 2, {}), ("tri_first_pct", 0, {}), ("tri_first_pct", 100, {}), ("tri_div", 2, COARSE),
                        ("tri_div", 8, COARSE))
# key -> the get_info key that shows its effect on the plan ("sym_pass_mb" is a one-GPU option: several shards ignore it)
K_VISIBLE = {"variant": "variant", "fuse_integrate": "variant", "jsplit": "jsplit", "sym_waves": "sym_waves", "taper": "taper",
             "sym_wide": "sym_wide", "sym_pass_mb": "sym_passes"}
# key -> murbhip.schedule_layout's argument
K_LAYOUT_ARG = {"jsplit": "split", "sym_waves": "waves", "taper": "taper", "diag_tri": "diag_tri", "tri_first_pct": "tri_first_pct",
                "tri_div": "tri_div"}
# id, n, devices, options before the upload, info keys the plan must show before a key is set, entries
K_CONFIGS = (
    ("sym5", 4609, None, {}, {"variant": 8, "world": 1}, K_SINGLE),
    ("shards3_overlap1", 6151, (0, 0, 0), {"variant": 8, "overlap": 1}, {"variant": 8, "world": 3}, K_SHARDED),
    ("fused3", 2049, None, {}, {"variant": 1, "jsplit": 1, "world": 1}, (("fuse_integrate", 0, {}),)),
    ("unfused3_onesided", 2049, None, {"fuse_integrate": 0, "variant": 1}, {"variant": 1, "world": 1}, (("variant", 8, {}),)),
)


def k_variant_after(start, key, value):
    """info("variant") once the key is set: the keys meant to switch the plan say which, every other key leaves it."""
    return value if key == "variant" else 8 if key == "fuse_integrate" else start


K_CASES = ("a", "b", "c")
# what every key goes back to between two cases (a configuration's own options override it)
K_DEFAULTS = {"variant": 0, "jsplit": 0, "taper": -1, "diag_tri": -1, "sym_red": -1, "sym_waves": 0, "sym_pass_mb": 0, "pad_aware": 1,
              "xcd_order": 0, "sym_wide": -1, "overlap": 1, "tri_first_pct": 50, "tri_div": 0, "fuse_integrate": 1}
K_FRESH_A = [UPLOAD, STEP, STEP]      # what case a must end like, on a context that had the key before its upload


def family_k(key, value):
    """{case: (sequence on the context under test, which observer positions are compared, sequences on a fresh context that had
    the key set before its upload, in the same order)}.  The end read-out of case a is compared too."""
    setk, sweep1, sweep0 = M("set", key, value), Obs("set", "energy_sweep", 1), Obs("set", "energy_sweep", 0)
    e = Obs("energy")
    return {
        "a": ([UPLOAD, Obs("compute_acc"), setk, STEP, STEP], (), ()),
        "b": ([UPLOAD, sweep0, e, setk, e], (4,), ([UPLOAD, sweep0, e],)),
        "c": ([UPLOAD, sweep0, e, setk, sweep1, e, sweep0, e], (5, 7), ([UPLOAD, sweep1, e], [UPLOAD, sweep0, e])),
    }


K_D = [UPLOAD, Obs("set", "energy_sweep", 0), Obs("energy"), Obs("set", "energy_sweep", 1), Obs("energy"), Obs("set", "energy_sweep", 0),
       Obs("energy")]      # K-c without the key change: values 2 and 6 are one evaluation's


# ---------------------------------------------------------------------------------------------------------------- family H
# "integrator" 2, one shard.  id, n, sweep option (None, "nearest", "contact", "potential"), options before the upload
H_CONFIGS = (
    ("plain", 2561, None, {}),
    ("jsplit3", 2561, None, {"jsplit": 3}),
    ("nearest", 2561, "nearest", {"nearest": 1}),
    ("contact", 2561, "contact", {"contact": 1}),
    ("potential", 2561, "potential", {"potential": 1}),
    ("sym5", 4609, None, {}),
)
H_INFO = {"plain": {"hermite_parts": 1, "variant": 1}, "jsplit3": {"hermite_parts": 3, "variant": 8}, "nearest": {"variant": 1},
          "contact": {"variant": 1}, "potential": {"variant": 1}, "sym5": {"variant": 8}}


def h_body_calls(option):
    calls = ["step", "evolve", "block", "block_open", "block_resume", "set_levels"]
    if option == "contact":
        calls.append("upload_radii")
    calls += ["host_acc", "upload", "init_bodies"]
    if option is None:
        calls.append("int0_step")     # set integrator 0; step; set integrator 2: refused while a sweep option is on
    return calls


def h_may_follow(m1, m2):
    """An open block is resumed or closed by a change of all bodies; everything else is refused while it is open."""
    if m1 == "block_open":
        return m2 in ("block_resume", "upload", "init_bodies", "host_acc")
    return m1 != "block_resume" and m2 != "block_resume"     # a resumed block needs three body-changing calls: not covered


def h_between(option, m1):
    """Every observer and refused call legal between m1 and the next body-changing call, in table order."""
    opened = m1 == "block_open"
    evolved = m1 in ("evolve", "block", "block_open")
    ops = []
    if not opened:
        ops += [Obs("caj"), Obs("caj_acc_jerk"), Obs("acc_pair"), Obs("energy0"), Obs("energy1"), Obs("moments"), Obs("state"), Obs("caj")]
        if option:
            ops.append(Obs("caj_option"))
        if m1 in ("step", "evolve", "block"):      # these leave a remembered evaluation: the bare downloads are legal alone
            ops += [Obs("jerk")] + ([Obs("option")] if option else [])
        if m1 in ("block", "set_levels"):
            ops.append(Obs("block_state"))
        if m1 == "block":
            ops.append(Obs("block_info"))
        if m1 == "evolve":
            ops.append(Obs("evolve_dts"))
        if evolved:
            ops.append(Obs("hits"))
        ops += [Obs("warmup"), Obs("masses"), Obs("sync"), Obs("set", "evolve_batch", 5)]
    else:
        ops += [Obs("state"), Obs("acc"), Obs("jerk")] + ([Obs("option")] if option else [])
        ops += [Obs("block_state"), Obs("block_info"), Obs("hits"), Obs("masses"), Obs("sync"), Obs("set", "evolve_batch", 5)]
    if option == "contact":
        ops.append(Obs("contact_121"))
    if option == "nearest" and not opened:
        ops.append(Obs("encounter_r0"))
    if opened:
        ops += [R(E_STATE, "step"), R(E_STATE, "steps"), R(E_STATE, "evolve"), R(E_STATE, "compute_acc"), R(E_STATE, "caj"),
                R(E_STATE, "energy"), R(E_STATE, "moments"), R(E_STATE, "warmup"), R(E_STATE, "set_levels"),
                R(E_STATE, "block_other_dt"), R(E_STATE, "block_other_kmax"),
                R(E_STATE, "set", "potential", 0 if option == "potential" else 1),
                R(E_STATE, "set", "contact", 0 if option == "contact" else 1),
                # C5 where no sweep option is on (0 -> 1) and under "nearest" (1 -> 0); under "contact" and "potential" the
                # value 1 is refused anyway, open block or not (the options exclude each other): that is C3 only.  Likewise
                # the two sets above are refused for the open block only where the exclusion does not refuse them first
                R(E_STATE, "set", "nearest", 0 if option == "nearest" else 1),
                R(E_STATE, "upload_radii")]
    ops += [R(E_INVALID, "evolve_bad"), R(E_INVALID, "block_bad"), R(E_INVALID, "set", "contact", 3), R(E_INVALID, "set", "no_such_key", 0),
            R(E_INVALID, "set_encounter", -1.0), R(E_INVALID, "radii_nan")]
    if option:
        ops.append(R(E_STATE, "set", "integrator", 0))
    return ops


def family_h(option):
    """upload, m1, <everything legal there>, m2 for every ordered pair of body-changing calls that may follow each other, each a
    second time with the list in between reversed."""
    calls = h_body_calls(option)
    out = []
    for m1 in calls:
        for m2 in calls:
            if not h_may_follow(m1, m2):
                continue
            between = h_between(option, m1)
            for order in (between, between[::-1]):
                out.append([UPLOAD, M(m1)] + list(order) + [M(m2)])
    return out


# What tests/test_call_orders_gpu.py must have run, per configuration (tests/test_call_orders_host.py pins the numbers).
def counts():
    out = {"F": {cfg[0]: len(F_INTEGRATORS) * len(family_f()) for cfg in F_CONFIGS},
           "K": {cfg[0]: len(cfg[5]) * len(K_CASES) + 1 for cfg in K_CONFIGS},      # + K-d
           "H": {cfg[0]: len(family_h(cfg[2])) for cfg in H_CONFIGS}}
    return out

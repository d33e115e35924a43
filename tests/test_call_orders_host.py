"""CPU: the classification table of tests/helpers/call_orders.py against include/murbhip.h, and its generators pinned: how many
sequences each family has per configuration and what they cover.  A new entry point or option key fails here until it is
classified."""
import os
import re
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import call_orders as C   # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "murbhip.h")).read()


def once_each(table, names, what):
    listed = [x for members in table.values() for x in members]
    assert sorted(listed) == sorted(set(listed)), f"{what}: listed twice: {sorted(x for x in set(listed) if listed.count(x) > 1)}"
    assert sorted(listed) == sorted(names), f"{what}: unclassified {sorted(set(names) - set(listed))}, unknown {sorted(set(listed) - set(names))}"


def test_every_entry_point_is_classified():
    declared = re.findall(r"^(?:const char\*|int|unsigned long) (murbhip_\w+)\(", HEADER, re.M)
    assert len(declared) >= 43 and len(set(declared)) == len(declared)
    once_each(C.FUNCTIONS, declared, "entry points")
    import murbhip
    assert sorted(declared) == sorted(murbhip.EXPORTS)      # the binding's own list agrees


def test_every_option_key_is_classified():
    comment = HEADER[HEADER.index("/* Integer options.  Keys:"):HEADER.index("int murbhip_set_option(")]
    keys = re.findall(r'^ \*   "(\w+)" ', comment, re.M)
    assert len(keys) >= 27 and len(set(keys)) == len(keys)
    once_each(C.OPTION_KEYS, keys, "option keys")
    # the contract paragraph names the same plan keys and neutral keys as the table
    contract = HEADER[HEADER.index("Call orders."):HEADER.index("typedef struct murbhip_ctx")]
    for key in C.OPTION_KEYS["plan"] + C.OPTION_KEYS["neutral"]:
        assert f'"{key}"' in contract, key
    for key in C.OPTION_KEYS["result"]:
        assert f'"{key}"' not in contract or key in ("contact", "nearest", "potential", "integrator"), key
    # and every key under which the comment promises the drop is a plan key: C4 stated under its keys
    for key in C.OPTION_KEYS["plan"]:
        entry = re.search(r'^ \*   "%s" .*?(?=^ \*   "\w+" |\Z)' % key, comment, re.M | re.S).group(0)
        assert "C4" in entry, key
    assert "C5" in re.search(r'^ \*   "nearest" .*?(?=^ \*   "\w+" )', comment, re.M | re.S).group(0)


def test_counts_are_pinned():
    assert C.counts() == {
        "F": {"sym5": 324, "fused3": 324, "shards3_overlap1": 324, "shards3_overlap2": 324, "shards2_onesided": 324, "multipass": 324},
        "K": {"sym5": 46, "shards3_overlap1": 64, "fused3": 4, "unfused3_onesided": 4},
        "H": {"plain": 152, "jsplit3": 152, "nearest": 120, "contact": 152, "potential": 120, "sym5": 152},
    }
    assert len(C.family_f()) == 2 * 9 * 9
    assert [c[1] for c in C.F_CONFIGS] == [4609, 2049, 6151, 6151, 6151, C.MULTIPASS_N]
    assert [(c[1], c[2]) for c in C.H_CONFIGS] == [(2561, None), (2561, None), (2561, "nearest"), (2561, "contact"), (2561, "potential"), (4609, None)]


def neighbours(seq):
    """(body-changing call, observer or refused call after it) and (the one before it, body-changing call) of a sequence, with
    other observers and refused calls in between: by the contract they are not there."""
    after, before = set(), set()
    last = None
    pending = []
    for op in seq:
        if op.kind == "M":
            before.update((o, op.name) for o in pending)
            last, pending = op.name, []
        else:
            after.add((last, op))
            pending.append(op)
    return after, before


def test_family_f_coverage():
    seqs = C.family_f()
    assert len({tuple(s) for s in seqs}) == len(seqs)
    assert {(s[-4], s[-3]) for s in seqs if len(s) == 5} == {(a, b) for a in C.F_OBSERVERS for b in C.F_OBSERVERS}      # every ordered pair,
    assert {(s[-4], s[-3]) for s in seqs if len(s) == 6} == {(a, b) for a in C.F_OBSERVERS for b in C.F_OBSERVERS}      # after either prefix
    assert len(C.F_OBSERVERS) == 9 and all(o.kind == "O" for o in C.F_OBSERVERS)
    after, before = set(), set()
    for s in seqs:
        a, b = neighbours(s)
        after |= a
        before |= b
        assert [op.name for op in C.twin(s)] in (["upload", "step", "step"], ["upload", "step", "step", "step"])
    for o in C.F_OBSERVERS:      # the upload only ever starts a sequence of this family
        assert ("upload", o) in after and ("step", o) in after and (o, "step") in before


def test_family_h_coverage():
    for name, n, option, options in C.H_CONFIGS:
        calls = C.h_body_calls(option)
        seqs = C.family_h(option)
        assert len({tuple(s) for s in seqs}) == len(seqs)
        pairs = {(s[1].name, s[-1].name) for s in seqs}
        assert pairs == {(a, b) for a in calls for b in calls if C.h_may_follow(a, b)}
        assert all(s[0] == C.UPLOAD and s[1].kind == "M" and s[-1].kind == "M" and len(C.twin(s)) == 3 for s in seqs)
        assert ("block_open", "block_resume") in pairs and ("block_open", "upload") in pairs and ("block_open", "step") not in pairs
        assert ("upload_radii" in calls) == (option == "contact") and ("int0_step" in calls) == (option is None)
        for m1 in calls:
            if m1 == "block_resume":
                continue
            legal = C.h_between(option, m1)
            followers = [m2 for m2 in calls if C.h_may_follow(m1, m2)]
            assert followers
            for m2 in followers:
                both = [s[2:-1] for s in seqs if s[1].name == m1 and s[-1].name == m2]
                assert both == [legal, legal[::-1]]      # everything legal there, in table order and reversed
        # the refusals of an open block, C5's among them, and the observers that stay legal inside it
        inside = C.h_between(option, "block_open")
        refused = {(op.name,) + op.args[1:] for op in inside if op.kind == "R" and op.args[0] == C.E_STATE}
        assert {("step",), ("steps",), ("evolve",), ("compute_acc",), ("caj",), ("energy",), ("moments",), ("warmup",), ("set_levels",),
                ("block_other_dt",), ("block_other_kmax",), ("upload_radii",)} <= refused
        assert {k for k in ("potential", "contact", "nearest") if any(r[:2] == ("set", k) for r in refused)} == {"potential", "contact", "nearest"}
        assert {op.name for op in inside if op.kind == "O"} >= {"state", "acc", "jerk", "block_state", "block_info"}
        assert not {op.name for op in inside if op.kind == "O"} & {"energy0", "energy1", "moments", "warmup", "caj", "acc_pair"}
        outside = {op.name for op in C.h_between(option, "step") if op.kind == "O"}
        assert outside >= {"caj", "caj_acc_jerk", "acc_pair", "energy0", "energy1", "moments", "state", "jerk", "warmup", "masses"}
        assert ("caj_option" in outside) == bool(option) and ("contact_121" in outside) == (option == "contact")
        assert ("encounter_r0" in outside) == (option == "nearest")
        assert sum(op.kind == "R" and op.args[0] == C.E_INVALID for op in inside) == 6


def test_family_k_cases():
    assert [c[0] for c in C.K_CONFIGS] == ["sym5", "shards3_overlap1", "fused3", "unfused3_onesided"]
    for cfg in C.K_CONFIGS:
        assert {k for k, _, _ in cfg[5]} <= set(C.OPTION_KEYS["plan"]) and "variant" in cfg[4]
        for key, value, beside in cfg[5]:
            assert {**C.K_DEFAULTS, **cfg[3], **beside}[key] != value      # a value-changing set
            assert key not in beside and set(beside) <= set(C.OPTION_KEYS["plan"])
    assert {k for k, _, _ in C.K_SHARDED} == set(C.OPTION_KEYS["plan"]) - {"fuse_integrate"}
    assert {k for k, _, _ in C.K_SINGLE} == set(C.OPTION_KEYS["plan"]) - {"fuse_integrate", "overlap", "tri_first_pct", "tri_div"}
    assert C.k_variant_after(8, "variant", 1) == 1 and C.k_variant_after(1, "fuse_integrate", 0) == 8 and C.k_variant_after(8, "taper", 0) == 8
    assert set(C.K_DEFAULTS) == set(C.OPTION_KEYS["plan"])
    cases = C.family_k("jsplit", 2)
    assert list(cases) == list(C.K_CASES)
    assert C.show(cases["a"][0]) == "upload ; o:compute_acc ; set(jsplit, 2) ; step ; step"
    assert C.show(cases["c"][0]) == ("upload ; o:set(energy_sweep, 0) ; o:energy ; set(jsplit, 2) ; o:set(energy_sweep, 1) ; o:energy ; "
                                     "o:set(energy_sweep, 0) ; o:energy")
    for seq, positions, fresh in cases.values():
        assert all(seq[p] == C.Obs("energy") for p in positions) and len(positions) == len(fresh)
        assert all(f[-1] == C.Obs("energy") for f in fresh)


def test_family_k_values_change_the_plan():
    """Every key has a listed value whose plan or layout differs from the automatic one.  A key with one listed value: that value
    is not the default, which is a fixed value ("pad_aware", "xcd_order", "overlap", "tri_first_pct") or is asserted on the device
    from get_info (K_VISIBLE).  A key with two: they are the key's whole domain ("diag_tri", "sym_red": 0 and 1), or their work
    lists differ from each other (murbhip_schedule_layout at the configuration's n and shards, whatever the other keys are), so at
    least one differs from the automatic one's."""
    import murbhip
    for name, n, devices, options, info, entries in C.K_CONFIGS[:2]:
        world = len(devices) if devices else 1
        values = {}
        for key, value, beside in entries:
            values.setdefault(key, []).append((value, beside))
        for key, listed in values.items():
            if len(listed) == 1:
                fixed = {"pad_aware": 1, "xcd_order": 0}
                assert key in C.K_VISIBLE or fixed[key] != listed[0][0], key
                continue
            assert len(listed) == 2 and listed[0][1] == listed[1][1]
            (a, beside), (b, _) = listed
            if key in ("diag_tri", "sym_red"):
                assert {a, b} == {0, 1}
            if key == "sym_red":      # the fold over the wave: no part of the work list
                continue
            if key == "overlap":      # default 1 (K_DEFAULTS, the configuration's own option): both differ from it
                assert 1 not in (a, b) and options["overlap"] == 1
                continue
            arg = C.K_LAYOUT_ARG[key]
            compared = 0
            # the other keys: the automatic plan's 16 sub-blocks per block (8 under 8 waves: 1024 / split >= 16 waves), or what the
            # entry puts in force; both forms of the diagonal blocks; the automatic taper of either configuration
            for split in ([beside["jsplit"]] if "jsplit" in beside else [8] if key == "sym_waves" else [16]):
                for diag_tri in (False, True):
                    for taper in (0, 5):
                        base = dict(split=split, waves=4, taper=taper, diag_tri=diag_tri, tri_first_pct=50, tri_div=1, exchange_mode=world > 1)
                        lay = [murbhip.schedule_layout(n, world, 0, **{**base, arg: bool(v) if key == "diag_tri" else v}) for v in (a, b)]
                        same = all(np.array_equal(x, y) for x, y in zip(lay[0][:2], lay[1][:2])) and lay[0][2:] == lay[1][2:]
                        assert not same, (name, key, a, b, base)
                        compared += 1
            assert compared == 4


def test_twin_and_solo():
    up, st, e0, acc = C.UPLOAD, C.STEP, C.Obs("energy0"), C.Obs("acc_pair")
    refused = C.R(C.E_STATE, "step")
    seq = [up, e0, st, refused, acc, e0, C.M("block_open")]
    assert C.twin(seq) == [up, st, C.M("block_open")]
    assert C.solo(seq) == {1: [up, e0, st, C.M("block_open")], 4: [up, st, acc, C.M("block_open")], 5: [up, st, e0, C.M("block_open")]}
    assert C.twin(C.twin(seq)) == C.twin(seq) and C.solo(C.twin(seq)) == {}
    for s in C.family_f()[:3] + C.family_h("contact")[:3]:
        assert all(C.twin(alone) == C.twin(s) and sum(op.kind == "O" for op in alone) == 1 for alone in C.solo(s).values())
        assert len(C.solo(s)) == sum(op.kind == "O" for op in s)


class FakeSim:
    """Enough of a Simulation for the interpreter: a counter that observers must not move unless `leaky`."""

    class Error(Exception):
        def __init__(self, code):
            self.code = code

    def __init__(self, leaky=False):
        self.x, self.leaky, self.n = 0, leaky, 4

    def upload(self, s):
        self.x = 1

    def step(self, dt):
        self.x = 3 * self.x + 1

    def steps(self, dt, k):
        raise FakeSim.Error(C.E_STATE)

    def energy(self):
        if self.leaky and self.x == 1:      # only straight after the upload: the end read-out's own call does not leak
            self.x += 1
        return float(self.x), -0.0

    def moments(self):
        return {"P": np.arange(3.0) * self.x, "M": 1.0}

    def state(self):
        return {"qx": np.full(4, self.x, np.float32)}

    def set_option(self, key, value):
        pass


def test_interpreter_records_and_diagnoses():
    ctx = {"s": None, "dt": 1.0, "integrator": 0}
    seq = [C.UPLOAD, C.Obs("energy0"), C.R(C.E_STATE, "steps"), C.R(C.E_INVALID, "steps"), C.Obs("moments"), C.STEP]
    run = lambda sim, s: C.run(sim, s, ctx, FakeSim.Error)
    rec, tw = run(FakeSim(), seq), run(FakeSim(), C.twin(seq))
    assert sorted(rec["values"]) == [1, 4] and rec["refused"] == {2: ("steps", C.E_STATE, C.E_STATE), 3: ("steps", C.E_INVALID, C.E_STATE)}
    assert [name for name, _ in rec["outs"]] == ["upload", "step"] and not rec["open"]
    assert sorted(rec["end"]) == ["energy", "moments", "state"] and C.differing(rec, tw) == []
    leaky = run(FakeSim(leaky=True), seq)
    assert C.differing(leaky, tw) == ["energy", "moments", "state"]
    named = C.diagnose(seq, tw, lambda s: run(FakeSim(leaky=True), s))
    assert len(named) == 1 and named[0].startswith("1:energy0 alone changes")
    assert C.freeze(0.0) != C.freeze(-0.0) and C.freeze(float("nan")) == C.freeze(float("nan"))
    assert C.freeze(np.float32([1, 2])) != C.freeze(np.float64([1, 2]))

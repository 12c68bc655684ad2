"""The host side of the three any-size train steps and of the module entry points of the M1 / M2 step, pinned call by call (no GPU;
tests/test_train_host_cpu.py replays the list against tests/train_host_refusals.json).

Every call here ends on the host: a planner fills a plan struct, and every other call is REFUSED by a check that runs before anything
touches the device -- which check, with which return code and which words, is what the recorded outcomes hold.  The pointers are made-up
addresses that nothing dereferences; no case may pass every check (the replay asserts a refusal code for each of them).

    python tests/train_host_cases.py            prints the outcomes as JSON for the library in force (DVAE_LIB, or the in-tree one), cases
                                                that differ in the entry point alone grouped (pack, below); an outcome is [return code,
                                                text of dvae_last_error (, sha256 of the plan's bytes)]

The outcomes in tests/train_host_refusals.json were recorded with the library of the commit BEFORE the host code of the three steps moved
into csrc/train_step_host.hpp, and are committed unchanged: the code under test supplies no expected value.
"""
import ctypes
import hashlib
import importlib
import json
import math
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = importlib.import_module("disentangled-vae_amd.native")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")
TC = importlib.import_module("disentangled-vae_amd.trainer_classifier")

BADARG, UNSUPPORTED = 1001, 1003
M1, M2, M2_INFO, M2_DEC = 1, 2, 3, 4
INF, NAN = math.inf, math.nan

# every extern "C" entry point of csrc/train_generic.hip, train_info.hip, train_classifier.hip and train_tables.hip, copied by hand from
# include/dvae_train.h: a new entry point without a case here fails test_every_entry_point_has_a_case
ENTRY_POINTS = """
dvae_train_generic_plan dvae_train_generic_plan_norm dvae_train_generic_init dvae_train_generic_repack dvae_train_generic_grads
dvae_train_generic_apply dvae_train_generic_step dvae_train_generic_eval dvae_train_generic_reduce dvae_train_generic_apply_flat
dvae_train_gradnorm_scratch_bytes dvae_train_generic_apply_flat_clipped dvae_module_generic_forward dvae_module_generic_backward
dvae_module_generic_plan dvae_module_generic_backward_y
dvae_train_clf_plan dvae_train_clf_init dvae_train_clf_repack dvae_train_clf_grads dvae_train_clf_apply dvae_train_clf_step
dvae_train_clf_eval dvae_train_clf_reduce dvae_train_clf_apply_flat dvae_train_clf_apply_flat_clipped
dvae_train_info_plan dvae_train_info_plan_mode dvae_train_info_init dvae_train_info_repack dvae_train_info_grads dvae_train_info_apply
dvae_train_info_step dvae_train_info_eval dvae_train_info_reduce dvae_train_info_apply_flat dvae_train_info_apply_flat_clipped
""".split()

PLAN_TYPE = {"generic": G.GenericPlan, "info": TI.InfoPlan, "clf": TC.ClassifierPlan}
Y, Z, H1, H2, B = 3, 17, 129, 127, 50         # no dimension a multiple of 16


def _ptrs():
    """A made-up, 256-byte aligned address per argument name (never dereferenced: every call is refused on the host)."""
    names = ("params m v ws x y eps losses counts flat scratch norm2_out skipped out_r out_mu out_lv out_z g_r g_mu g_lv g_z g_y "
             "row_index norm_mean norm_div").split()
    return {n: 0x10000 + 0x1000 * i for i, n in enumerate(names)}


PTR = _ptrs()
ADAM = [("step", 1), ("lr", 1e-3), ("beta1", 0.9), ("beta2", 0.999), ("adam_eps", 1e-8)]
CLIP = [("max_norm", 1.0), ("scratch", PTR["scratch"]), ("norm2_out", PTR["norm2_out"]), ("skipped", PTR["skipped"])]


def _p(*names):
    return [(n, PTR[n]) for n in names]


def _signatures(kind):
    """{entry point: [(argument, a value that passes every check)]} in the order of include/dvae_train.h, behind the plan and without the stream."""
    clf = kind == "clf"
    inputs = _p("x") + [("ldx", 513)] + _p("y") + [("ldy", Y)] + ([("loss_eps", 1e-8)] if clf else _p("eps") + [("loss_eps", 1e-8)])
    out = _p("losses", "counts") if clf else _p("losses")
    sig = {
        "init": _p("params", "ws"),
        "repack": _p("params", "ws"),
        "grads": _p("ws") + inputs,
        "apply": _p("params", "m", "v", "ws") + ADAM + [("grad_scale", 1.0)] + out,
        "step": _p("params", "m", "v", "ws") + inputs + ADAM + out,
        "eval": _p("ws") + inputs + out,
        "reduce": _p("ws", "flat") + [("accumulate", 0), ("weight", 1.0)] + out,
        "apply_flat": _p("params", "m", "v", "ws", "flat") + ADAM + [("grad_scale", 1.0)],
        "apply_flat_clipped": _p("params", "m", "v", "ws", "flat") + ADAM + [("grad_scale", 1.0)] + CLIP,
    }
    prefix = {"generic": "dvae_train_generic_", "info": "dvae_train_info_", "clf": "dvae_train_clf_"}[kind]
    sig = {prefix + k: v for k, v in sig.items()}
    if kind == "generic":
        fwd = _p("params", "ws") + inputs[:-1]
        bwd = fwd + _p("g_r") + [("ld_gr", 513)] + _p("g_mu", "g_lv", "g_z", "flat") + [("accumulate", 0)]
        sig["dvae_module_generic_forward"] = fwd + _p("out_r") + [("ld_r", 513)] + _p("out_mu", "out_lv", "out_z") + [("repack", 0)]
        sig["dvae_module_generic_backward"] = bwd
        sig["dvae_module_generic_backward_y"] = bwd + _p("g_y") + [("ld_gy", Y)]
    return sig


# the pointer arguments an entry point may be given as null (no refusal to record)
OPTIONAL = {"out_z", "g_r", "g_mu", "g_lv", "g_z", "g_y"}
SETUP = ("_init", "_repack")                    # serve an M2_DEC plan; so do the module entry points


def _plan(lib, kind, model=M2, std_norm=0, mode=0, ksplit=0):
    plan = PLAN_TYPE[kind]()
    if kind == "generic" and model == M2_DEC:
        rc = lib.dvae_module_generic_plan(M2_DEC, Y, Z, H1, H2, B, ksplit, ctypes.byref(plan))
    elif kind == "generic":
        rc = lib.dvae_train_generic_plan_norm(model, 0 if model == M1 else Y, Z, H1, H2, 0, B, ksplit, std_norm, ctypes.byref(plan))
    elif kind == "info":
        rc = lib.dvae_train_info_plan_mode(Y, Z, H1, H2, B, ksplit, mode, ctypes.byref(plan))
    else:
        rc = lib.dvae_train_clf_plan(H1, H2, Y, 0, B, ksplit, ctypes.byref(plan))
    assert rc == 0, (kind, model, lib.dvae_last_error())
    return plan


def _as_kind(plan, kind):
    """The bytes of a plan of another step in the struct of this one (zero padded): a plan of the wrong kind."""
    T = PLAN_TYPE[kind]
    return T.from_buffer_copy(bytes(plan).ljust(ctypes.sizeof(T), b"\0")[:ctypes.sizeof(T)])


def _edit(field, value):
    def f(plan):
        setattr(plan, field, value(getattr(plan, field)) if callable(value) else value)
    return f


def _outcome(lib, rc):
    return [int(rc), lib.dvae_last_error().decode("utf-8", "replace") if rc != 0 else ""]


def _refused(name, sig, plan_of, edits=(), **changes):
    """A case: entry point `name` on plan_of(lib) after `edits`, its arguments the passing values of `sig` but for `changes`."""
    unknown = set(changes) - {a for a, _ in sig} - {"plan"}
    assert not unknown, (name, unknown)

    def run(lib):
        plan = None
        if changes.get("plan", 1) is not None:
            plan = plan_of(lib)
            for e in edits:
                e(plan)
        args = [changes.get(a, v) for a, v in sig]
        rc = getattr(lib, name)(None if plan is None else ctypes.byref(plan), *args, None)
        return _outcome(lib, rc)
    return name, run


def _planner(name, plan_type, *args, null_plan=False):
    def run(lib):
        plan = plan_type()
        rc = getattr(lib, name)(*args, None if null_plan else ctypes.byref(plan))
        out = _outcome(lib, rc)
        if rc == 0:
            out.append(hashlib.sha256(bytes(plan)).hexdigest())
        return out
    return name, run


def _planner_cases():
    c = {}
    gp, gn, mp = "dvae_train_generic_plan", "dvae_train_generic_plan_norm", "dvae_module_generic_plan"
    ip, im, cp = "dvae_train_info_plan", "dvae_train_info_plan_mode", "dvae_train_clf_plan"
    GP, IP, CP = G.GenericPlan, TI.InfoPlan, TC.ClassifierPlan
    # valid sizes: (y, z, h1, h2, B); the first has no dimension a multiple of 16, the second is every limit
    for y, z, h1, h2, b in ((Y, Z, H1, H2, B), (513, 128, 512, 512, 1000)):
        for ks in (0, 3):
            tag = f"y{y}-z{z}-h{h1}x{h2}-B{b}-ksplit{ks}"
            c[f"train_generic_plan/M2-{tag}"] = _planner(gp, GP, M2, y, z, h1, h2, 0, b, ks)
            c[f"train_generic_plan_norm/M2-{tag}-std_norm"] = _planner(gn, GP, M2, y, z, h1, h2, 0, b, ks, 1)
            c[f"module_generic_plan/M2_DEC-{tag}"] = _planner(mp, GP, M2_DEC, y, z, h1, h2, b, ks)
            c[f"train_info_plan/{tag}"] = _planner(ip, IP, y, z, h1, h2, b, ks)
            c[f"train_clf_plan/{tag}"] = _planner(cp, CP, h1, h2, y, 0, b, ks)
    c["train_generic_plan/M1"] = _planner(gp, GP, M1, 0, Z, H1, H2, 0, B, 0)
    c["module_generic_plan/M2"] = _planner(mp, GP, M2, Y, Z, H1, H2, B, 0)
    for mode in (0, 1, 2, 3, 4, 5):             # every legal info_mode: DEC_CLASSIFIER 1, AUX_UNIFORM 2, AUX_ENTROPY 4, not 2 | 4
        c[f"train_info_plan_mode/mode{mode}"] = _planner(im, IP, Y, Z, H1, H2, B, 0, mode)
    # the planners' refusals
    ok = (Y, Z, H1, H2)
    c["train_generic_plan/null-plan"] = _planner(gp, GP, M2, *ok, 0, B, 0, null_plan=True)
    c["train_generic_plan_norm/std_norm-2"] = _planner(gn, GP, M2, *ok, 0, B, 0, 2)
    c["train_generic_plan_norm/std_norm-2-and-model-3"] = _planner(gn, GP, M2_INFO, *ok, 0, B, 0, 2)
    for model in (M2_INFO, M2_DEC):
        c[f"train_generic_plan/model-{model}"] = _planner(gp, GP, model, *ok, 0, B, 0)
    c["train_generic_plan/precision-1"] = _planner(gp, GP, M2, *ok, 1, B, 0)
    c["train_generic_plan/model-3-and-precision-1"] = _planner(gp, GP, M2_INFO, *ok, 1, B, 0)
    for dims in ((514, Z, H1, H2), (Y, 129, H1, H2), (Y, Z, 0, H2), (Y, Z, H1, 513)):
        tag = "y{}-z{}-h{}x{}".format(*dims)
        c[f"train_generic_plan/dims-{tag}"] = _planner(gp, GP, M2, *dims, 0, B, 0)
        c[f"module_generic_plan/M2_DEC-dims-{tag}"] = _planner(mp, GP, M2_DEC, *dims, B, 0)
        c[f"train_info_plan/dims-{tag}"] = _planner(ip, IP, *dims, B, 0)
        if dims[1] == Z:
            c[f"train_clf_plan/dims-{tag}"] = _planner(cp, CP, dims[2], dims[3], dims[0], 0, B, 0)
    c["train_generic_plan/M1-with-y"] = _planner(gp, GP, M1, *ok, 0, B, 0)
    c["train_generic_plan/M2-without-y"] = _planner(gp, GP, M2, 0, Z, H1, H2, 0, B, 0)
    c["module_generic_plan/M2_DEC-without-y"] = _planner(mp, GP, M2_DEC, 0, Z, H1, H2, B, 0)
    c["module_generic_plan/null-plan"] = _planner(mp, GP, M2_DEC, *ok, B, 0, null_plan=True)
    c["module_generic_plan/model-3"] = _planner(mp, GP, M2_INFO, *ok, B, 0)
    c["train_info_plan/null-plan"] = _planner(ip, IP, *ok, B, 0, null_plan=True)
    for mode in (6, 8):
        c[f"train_info_plan_mode/mode-{mode}"] = _planner(im, IP, *ok, B, 0, mode)
    c["train_info_plan_mode/mode-6-and-dims"] = _planner(im, IP, Y, 0, H1, H2, B, 0, 6)
    c["train_clf_plan/null-plan"] = _planner(cp, CP, H1, H2, Y, 0, B, 0, null_plan=True)
    c["train_clf_plan/precision-1"] = _planner(cp, CP, H1, H2, Y, 1, B, 0)
    c["train_clf_plan/precision-1-and-dims"] = _planner(cp, CP, 0, H2, Y, 1, B, 0)
    for tag, b, ks in (("B-0", 0, 0), ("B-2^31", 1 << 31, 0), ("ksplit--1", B, -1), ("ksplit-17", B, 17), ("B-0-and-ksplit-17", 0, 17)):
        c[f"train_generic_plan/{tag}"] = _planner(gp, GP, M2, *ok, 0, b, ks)
        c[f"module_generic_plan/M2_DEC-{tag}"] = _planner(mp, GP, M2_DEC, *ok, b, ks)
        c[f"train_info_plan/{tag}"] = _planner(ip, IP, *ok, b, ks)
        c[f"train_clf_plan/{tag}"] = _planner(cp, CP, H1, H2, Y, 0, b, ks)
    for n in (0, 1, 4097, 1 << 31):
        def run(lib, n=n):
            got = lib.dvae_train_gradnorm_scratch_bytes(n)
            return [int(got), lib.dvae_last_error().decode("utf-8", "replace") if got == 0 else ""]
        c[f"train_gradnorm_scratch_bytes/n-{n}"] = ("dvae_train_gradnorm_scratch_bytes", run)
    return c


def _entry_cases(kind):
    c = {}
    base = lambda lib: _plan(lib, kind)
    other = {"generic": "info", "info": "clf", "clf": "generic"}[kind]
    bigger = _edit("workspace_bytes", lambda v: v + 256)
    for name, sig in _signatures(kind).items():
        short = name[len("dvae_"):]
        args = [a for a, _ in sig]
        module = "module" in name

        def add(tag, plan_of=base, edits=(), **changes):
            assert f"{short}/{tag}" not in c
            c[f"{short}/{tag}"] = _refused(name, sig, plan_of, edits, **changes)

        add("null-plan", plan=None)
        add("plan-of-another-step", lambda lib: _as_kind(_plan(lib, other), kind))
        add("plan-edited", edits=[bigger])
        if kind == "generic":
            add("plan-edited-std_norm-2", edits=[_edit("std_norm", 2)])
            if not module and not name.endswith(SETUP):
                add("M2_DEC-plan", lambda lib: _plan(lib, kind, model=M2_DEC))
                add("M2_DEC-plan-and-null-ws", lambda lib: _plan(lib, kind, model=M2_DEC), ws=None)
        if kind != "clf":
            for field, v in (("kl_weight", -1.0), ("kl_weight", INF), ("kl_floor", NAN)):
                add(f"plan-{field}-{v}", edits=[_edit(field, v)])
        for a in args:
            if a in PTR and a not in OPTIONAL:
                add(f"null-{a}", **{a: None})
        first = next(a for a in args if a in PTR)
        add(f"plan-edited-and-null-{first}", edits=[bigger], **{first: None})
        if "step" in args:
            add("step-0", step=0)
            for a in ("params", "ws", "scratch"):
                if a in args:
                    add(f"null-{a}-and-step-0", step=0, **{a: None})
            add("plan-edited-and-step-0", edits=[bigger], step=0)
        if "flat" in args and "lr" in args:
            add("lr-inf", lr=INF)
            add("grad_scale-nan", grad_scale=NAN)
            add("step-0-and-lr-nan", step=0, lr=NAN)
        if "weight" in args:
            add("weight-inf", weight=INF)
            add("null-losses-and-weight-nan", losses=None, weight=NAN)
        if "accumulate" in args:
            add("accumulate-2", accumulate=2)
            add("null-flat-and-accumulate-2", flat=None, accumulate=2)
            add("misaligned-flat", flat=PTR["flat"] + 4)
        if "max_norm" in args:
            add("max_norm-0", max_norm=0.0)
            add("max_norm-nan", max_norm=NAN)
            add("misaligned-flat", flat=PTR["flat"] + 4)
            add("misaligned-scratch", scratch=PTR["scratch"] + 4)
            add("null-scratch-and-max_norm-0", scratch=None, max_norm=0.0)
            add("max_norm-nan-and-misaligned-flat", max_norm=NAN, flat=PTR["flat"] + 4)
        if "ldx" in args:
            add("ldx-512", ldx=512)
            add("ldy-2", ldy=Y - 1)
            add("null-x-and-ldx-512", x=None, ldx=512)
            if not module:
                add("gather-row_count-0", edits=[_edit("row_index", PTR["row_index"])])
            if "losses" in args:
                add("ldx-512-and-null-losses", ldx=512, losses=None)
            if kind == "generic":
                add("M1-y-given", lambda lib: _plan(lib, kind, model=M1))
                add("M2-y-missing", y=None)
                add("std_norm-without-tables", lambda lib: _plan(lib, kind, std_norm=1))
        if module:
            dec = lambda lib: _plan(lib, kind, model=M2_DEC)
            add("gather-table-in-the-plan", edits=[_edit("row_index", PTR["row_index"]), _edit("row_count", 100)])
            add("M2_DEC-null-y", dec, y=None)
            if "ld_r" in args:
                add("ld_r-512", ld_r=512)
            if "ld_gr" in args:
                add("ld_gr-512", ld_gr=512)
                add("accumulate-2-and-ld_gr-512", accumulate=2, ld_gr=512)
            if "g_y" in args:
                add("g_y-on-an-M2-plan")
                add("M2_DEC-ld_gy-2", dec, ld_gy=Y - 1)
    return c


def cases():
    """{case id: (entry point, run(lib) -> outcome)}."""
    c = _planner_cases()
    for kind in ("generic", "info", "clf"):
        c.update(_entry_cases(kind))
    return c


def is_planner_case(case_id):
    return case_id.split("/")[0].endswith(("_plan", "_plan_norm", "_plan_mode", "scratch_bytes"))


def outcomes(lib):
    return {k: run(lib) for k, (_, run) in cases().items()}


# The recorded file groups the cases "<who>/<tag>" that differ in <who> alone: a record is [tag, [who, ...], return code, text (, sha256)],
# where a text that starts with its own "<who>:" is written "@:".  pack and unpack are exact inverses on every outcome of this list.
def pack(got):
    groups = {}
    for k in sorted(got):
        who, tag = k.split("/", 1)
        rc, text, *sha = got[k]
        assert not text.startswith("@:")
        if text.startswith(who + ":"):
            text = "@" + text[len(who):]
        groups.setdefault((tag, rc, text, *sha), []).append(who)
    return [[key[0], whos, *key[1:]] for key, whos in sorted(groups.items())]


def unpack(records):
    got = {}
    for tag, whos, rc, text, *sha in records:
        for who in whos:
            assert f"{who}/{tag}" not in got
            got[f"{who}/{tag}"] = [rc, who + text[1:] if text.startswith("@:") else text, *sha]
    return got


if __name__ == "__main__":
    got = outcomes(N.load())
    assert unpack(pack(got)) == got
    sys.stdout.write("[\n" + ",\n".join(json.dumps(r) for r in pack(got)) + "\n]\n")      # one record a line

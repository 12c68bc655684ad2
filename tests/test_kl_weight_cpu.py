"""CPU (no GPU): the premises of tests/test_gpu_train_kl_weight.py and the host side of the weighted KL term (kl_weight / kl_warmup /
kl_floor: disentangled-vae_amd/kl_weight.py).

* The float32 restatement of the truth of tests/kl_weight_cases.py stays inside the device bars on every case, batch and setting, and
  inside the bounds of tests/adam_bounds.py after the update: the bars ask nothing float32 arithmetic cannot give.
* The conditions on the floor lam* hold for every (case, batch).
* The schedule, the refusals, which step serves which options, and the plan's bytes under the default options."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import adam_bounds as ab
import kl_weight_cases as kc
import train_generic_cases as tc
import train_info_cases as ic
import train_info_modes_cases as mc
from oracle import vae_oracle as vo

KL = importlib.import_module("disentangled-vae_amd.kl_weight")
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")

REF = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
OTHER = dict(x_dim=513, y_dim=3, z_dim=17, h_dim=(129, 127))
HYPER = (1, 1e-4, 0.9, 0.999, 1e-8)


def _adam_worst(params32, grads32):
    """Worst error / bound of one float32 Adam step from zero moments (vo.adam_step in float32) under tests/adam_bounds.py."""
    worst = 0.0
    for k, g in grads32.items():
        P0, G32 = params32[k].ravel(), np.asarray(g, np.float32).ravel()
        z = np.zeros_like(P0)
        got = vo.adam_step(P0, G32, z, z, 1)
        for a, w, b in zip(got, ab.truth(P0, z, z, G32, HYPER), ab.bounds(P0, z, z, G32, HYPER)):
            worst = max(worst, float(np.max(ab.ratios(a, w, b))))
    return worst


@pytest.mark.parametrize("setting", kc.SETTINGS, ids=kc.setting_id)
@pytest.mark.parametrize("B", kc.BATCHES)
@pytest.mark.parametrize("case", kc.CASES, ids=tc.case_id)
def test_float32_restatement_inside_the_bars(case, B, setting):
    for w, lam in kc.expand("generic", case, B, setting):
        l64, g64 = kc.truth(case, B, w, lam)
        l32, g32 = kc.run(case, B, np.float32, w, lam)
        le, (ge, name) = tc.loss_err(l32, l64), tc.grad_err(g32, g64)
        p32 = tc._cast(case, B, np.float32)[0]
        aw = _adam_worst(p32, {k: v.astype(np.float32) for k, v in g32.items()})
        print(f"{tc.case_id(case)} B {B} w {w} floor {lam:.4f}: losses {le:.2e}, gradients {ge:.2e} ({name}), adam {aw:.3f} of bound")
        assert le <= kc.LOSS_RTOL and ge <= kc.GRAD_TOL and aw <= 1.0, (le, ge, name, aw)


def test_float32_restatement_inside_the_bars_std_norm():
    case, B = kc.NORM_CASE, 50
    for setting in kc.SETTINGS:
        for w, lam in kc.expand("generic", case, B, setting, True):
            l64, g64 = kc.truth(case, B, w, lam, True)
            l32, g32 = kc.run(case, B, np.float32, w, lam, True)
            le, (ge, name) = tc.loss_err(l32, l64), tc.grad_err(g32, g64)
            print(f"std_norm {tc.case_id(case)} w {w} floor {lam:.4f}: losses {le:.2e}, gradients {ge:.2e} ({name})")
            assert le <= kc.LOSS_RTOL and ge <= kc.GRAD_TOL


@pytest.mark.parametrize("mode", kc.INFO_MODES, ids=mc.mode_id)
@pytest.mark.parametrize("B", kc.BATCHES)
@pytest.mark.parametrize("case", kc.INFO_CASES, ids=ic.case_id)
def test_float32_restatement_inside_the_bars_m2_info(case, B, mode):
    for setting in kc.SETTINGS:
        for w, lam in kc.expand("info", case, B, setting):
            l64, g64 = kc.info_truth(case, B, mode, w, lam)
            l32, g32 = kc.info_run(case, B, np.float32, mode, w, lam)
            le, (ge, name) = ic.loss_err(l32, l64), ic.grad_err(g32, g64)
            print(f"{ic.case_id(case)} {mc.mode_id(mode)} B {B} w {w} floor {lam:.4f}: losses {le:.2e}, gradients {ge:.2e} ({name})")
            assert le <= kc.LOSS_RTOL and ge <= kc.GRAD_TOL, (le, ge, name)


def test_the_truth_at_the_defaults_is_the_unweighted_truth():
    case, B = (3, 17, (129, 127)), 50
    l, g = kc.truth(case, B, 1.0, 0.0)
    l0, g0, _ = tc.truth(case, B)
    assert np.array_equal(l, l0[0]) and all(np.array_equal(g[k], g0[0][k]) for k in g)
    li, gi = kc.info_truth(case, B, ("truth", "bce"), 1.0, 0.0)
    l1, g1, _, _ = ic.truth(case, B)
    assert np.array_equal(li, l1[0]) and all(np.array_equal(gi[k], g1[0][k]) for k in gi)
    # and a weight moves it by far more than the bar
    assert tc.loss_err(kc.truth(case, B, 0.25, 0.0)[0][:1], l0[0][:1]) > 10 * kc.LOSS_RTOL


def test_floor_conditions():
    todo = [("generic", c, B, False) for c in kc.CASES for B in kc.BATCHES] + [("info", c, B, False) for c in kc.INFO_CASES for B in kc.BATCHES] + \
        [("generic", kc.NORM_CASE, 50, True)]
    for kind, case, B, norm in todo:
        f = kc.floor_figures(kind, case, B, norm)
        print(f"{kind} {tc.case_id(case)} B {B}{' std_norm' if norm else ''}: {f['n']} elements, floors {['%.4f' % v for v in f['floors']]}, half-gap "
              f"{f['half_gap']:.2e} = {f['half_gap'] / f['k_err']:.0f} k-errors, below {f['below']}")
        fl = kc.floors(kind, case, B, norm)             # asserts both conditions
        assert len(fl) == (2 if f["n"] < 5 else 1) and all(v > 0 for v in fl)
        if f["n"] >= 5:
            assert fl[0] > 0.5                          # above the minimum of an element: the floor clamps


def test_schedule():
    f32 = lambda v: float(np.float32(v))
    assert [KL.weight_at(0.5, 0, s) for s in range(1, 6)] == [0.5] * 5
    assert [KL.weight_at(0.5, 1, s) for s in range(1, 6)] == [0.5] * 5
    assert [KL.weight_at(0.5, 3, s) for s in range(1, 6)] == [f32(0.5 * (1 / 3)), f32(0.5 * (2 / 3)), 0.5, 0.5, 0.5]
    assert [KL.weight_at(0.3, 3, s) for s in range(1, 6)] == [f32(0.3 * (1 / 3)), f32(0.3 * (2 / 3)), f32(0.3), f32(0.3), f32(0.3)]
    assert KL.weight_at(1.0, 0, 1) == 1.0 and KL.weight_at(0.0, 3, 2) == 0.0
    for w in (KL.weight_at(0.3, 7, s) for s in range(1, 10)):
        assert w == f32(w)                              # rounded to float32 once


class _Host(KL.KLOptions):
    """The options on a trainer without a device: what GenericTrainer and InfoTrainer inherit."""

    def __init__(self, **kw):
        self._shared = {"step_count": 0}
        self.plan = G.GenericPlan()
        self._kl_init(kw.get("kl_weight", 1.0), kw.get("kl_warmup", 0), kw.get("kl_floor", 0.0), None)

    step_count = property(lambda self: self._shared["step_count"])


def test_options_follow_the_step_count():
    h = _Host(kl_weight=0.5, kl_warmup=3, kl_floor=0.7)
    seen = []
    for _ in range(5):
        seen.append(h.kl_weight_next)
        h._kl_plan(h.step_count + 1)
        assert h.plan.kl_weight == seen[-1] and h.plan.kl_floor == 0.7
        h._shared["step_count"] += 1
    assert seen == [KL.weight_at(0.5, 3, s) for s in range(1, 6)]
    h._kl_plan(None)                                    # evaluate(): the target weight
    assert h.plan.kl_weight == 0.5
    h.kl_weight = 0.25                                  # reassigned between steps
    assert h.kl_weight_next == 0.25 and (h.kl_weight, h.kl_warmup, h.kl_floor) == (0.25, 3, 0.7)
    with pytest.raises(AttributeError):
        h.kl_weight_next = 1.0
    with pytest.raises(ValueError):
        h.kl_weight = -1.0
    bare = _Host.__new__(_Host)                         # a trainer assembled without the constructor: the unweighted step
    bare._shared, bare.plan = {"step_count": 0}, G.GenericPlan()
    assert (bare.kl_weight, bare.kl_warmup, bare.kl_floor, bare.kl_weight_next) == (1.0, 0, 0.0, 1.0)


BAD = [dict(kl_weight=-0.1), dict(kl_weight=math.nan), dict(kl_weight=math.inf), dict(kl_floor=-1e-3), dict(kl_floor=math.nan),
       dict(kl_floor=math.inf), dict(kl_warmup=-1), dict(kl_warmup=2.5), dict(kl_warmup="3"), dict(kl_weight="x")]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_refusals_before_the_device(bad, monkeypatch):
    import torch
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append(1) or False)
    with pytest.raises(ValueError, match=next(iter(bad))):
        KL.check_options(**bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        G.GenericTrainer("M2", OTHER, batch=8, **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        TI.InfoTrainer(OTHER, batch=8, **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        T.make_trainer("M2", REF, batch=8, **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        TI.make_info_trainer(REF, batch=8, **bad)
    assert not touched


def test_good_options():
    assert KL.check_options(0, 0, 0) == (0.0, 0, 0.0) and KL.check_options(4, np.int64(200), np.float32(0.75)) == (4.0, 200, 0.75)
    assert KL.check_options(0.5, 3.0, 0.7) == (0.5, 3, 0.7)


def test_the_resident_trainer_refuses_naming_the_generic_step():
    for kw in (dict(kl_weight=0.5), dict(kl_warmup=10), dict(kl_floor=0.7), dict(kl_weight=1.0)):
        with pytest.raises(NotImplementedError, match="generic step"):
            T.Trainer("M2", REF, batch=8, **kw)


def test_kinds():
    # the defaults: today's answers
    assert T.trainer_kind("M2", REF) == "resident" and T.trainer_kind("M2", OTHER) == "generic" and T.trainer_kind("M1", dict(REF, y_dim=0)) == "resident"
    assert T.trainer_kind("M2", REF, std_norm=True) == "generic" and T.trainer_kind("M2_info", REF) == "resident"
    assert TI.info_trainer_kind(REF) == "resident" and TI.info_trainer_kind(OTHER) == "generic" and TI.info_trainer_kind(REF, aux_enc="entropy") == "generic"
    assert T.trainer_kind("M2", REF, kl_weight=1.0, kl_warmup=0, kl_floor=0.0) == "resident"
    assert TI.info_trainer_kind(REF, kl_weight=1.0, kl_warmup=0, kl_floor=0.0) == "resident"
    # any other value: the generic step, at the reference geometry too
    for kw in (dict(kl_weight=0.5), dict(kl_warmup=200), dict(kl_floor=0.7), dict(kl_weight=0.0)):
        assert T.trainer_kind("M2", REF, **kw) == "generic" and T.trainer_kind("M2", OTHER, **kw) == "generic"
        assert TI.info_trainer_kind(REF, **kw) == "generic" and TI.info_trainer_kind(OTHER, **kw) == "generic"
    out = dict(x_dim=513, y_dim=1, z_dim=200, h_dim=(128, 128))
    assert T.trainer_kind("M2", out, kl_weight=0.5) is None and TI.info_trainer_kind(out, kl_weight=0.5) is None
    with pytest.raises(NotImplementedError, match="kl_weight"):
        T.make_trainer("M2", out, batch=8, kl_weight=0.5)


@pytest.mark.parametrize("std_norm", [False, True])
def test_plan_bytes_under_the_default_options(std_norm):
    for case in ((3, 17, (129, 127)), (0, 32, (256, 64))):
        a = G.make_plan(tc.model_of(case), tc.dims_of(case), 50, std_norm=std_norm)
        b = G.make_plan(tc.model_of(case), tc.dims_of(case), 50, std_norm=std_norm)
        assert a.kl_weight == 1.0 and a.kl_floor == 0.0                   # the planner's
        b.kl_weight, b.kl_floor = KL.weight_at(*KL.check_options(1.0, 0, 0.0)[:2], 1), KL.check_options(1.0, 0, 0.0)[2]
        assert bytes(a) == bytes(b)
    a, b = TI.make_plan(OTHER, 50), TI.make_plan(OTHER, 50)
    assert a.kl_weight == 1.0 and a.kl_floor == 0.0
    b.kl_weight, b.kl_floor = KL.weight_at(1.0, 0, 7), 0.0
    assert bytes(a) == bytes(b)
    assert ctypes.sizeof(G.GenericPlan) % 8 == 0 and G.GenericPlan.kl_floor.offset + 8 == ctypes.sizeof(G.GenericPlan)
    assert TI.InfoPlan.kl_floor.offset + 8 == ctypes.sizeof(TI.InfoPlan)      # the structs grew at their end only


def test_the_library_refuses_a_bad_plan():
    native = importlib.import_module("disentangled-vae_amd.native")
    lib = native.load()
    for field, v in (("kl_weight", -1.0), ("kl_weight", math.nan), ("kl_floor", -0.5), ("kl_floor", math.inf)):
        p = G.make_plan("M2", OTHER, 50)
        setattr(p, field, v)
        assert lib.dvae_train_generic_eval(ctypes.byref(p), None, None, 513, None, 3, None, 1e-8, None, None) != 0
        assert b"kl_" in lib.dvae_last_error()
        q = TI.make_plan(OTHER, 50)
        setattr(q, field, v)
        assert lib.dvae_train_info_eval(ctypes.byref(q), None, None, 513, None, 3, None, 1e-8, None, None) != 0
        assert b"kl_" in lib.dvae_last_error()

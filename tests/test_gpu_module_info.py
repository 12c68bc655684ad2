"""The M2_info body ("M2_DEC") of any covered size on the generic module engine -- module_path.GenericModuleEngine on a plan of
dvae_module_generic_plan, the DEC variant of the generic rows kernel's two module modes, dvae_module_generic_backward_y for the label
gradient -- against the float64 oracle (tests/module_info_cases.py: truth, float32 restatement in two orders, statistics, bound, inputs,
cases; tests/test_module_info_cpu.py pins the truth against torch.float64 autograd and shows that the statistics see seeded faults).

The engine is driven as tests/test_gpu_module_generic.py drives it: module_path.engine_for(module, "M2_DEC", x, y), all four outputs from
module_path.run(eng, x, y, eps), gradients from torch.autograd.grad(outputs, eng.params [+ y], grad_outputs).

Checks: (1) outputs and all 14 gradients against float64 by the rule; (2) g_y per label column and over the tensor; (3) the C ABI with a
row-padded g_y over a NaN-filled buffer; (4) autograd behaviour through the modules; (5) both reference loop bodies on
DeepGenerativeModel_v5, switch on against off.

Measured on the MI355X: 48 cases, 6.9 s of wall time with the CPU references (the slowest: the 4149-frame reference, 1.2 s).  Worst
statistic / bound over all cases -- a device that errs exactly as the larger restatement draw does reaches 0.25:
  outputs        log r 0.30   mu 0.39   log_var 0.35   z 0.35
  gradients      encoder 0.41   decoder hidden layers 0.59 ((3, 17, (129, 127)) at ONE frame)   reconstruction layer 0.93: the per-row
                 figure of the reconstruction bias at (1, 1, (1, 1)), 50 frames, row 511 -- a frame sum that cancels, formed by the
                 weight-gradient kernel, which this variant does not edit -- and 0.51 elsewhere
  g_y            0.36 per label column (one frame), 0.34 at 50 frames, 0.29 at y 513 / 512 / 512 and on the 4149-frame batch; identically
                 zero truths (no g_r upstream) came back exactly 0.0
  loop bodies    gradients within 2.3e-7 ... 3.5e-7 of a tensor's maximum, every loss equal to the printed digit on both sides
Every bit-for-bit check holds.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import module_info_cases as mi
import train_generic_cases as gc

pytestmark = pytest.mark.gpu

mp = importlib.import_module("disentangled-vae_amd.module_path")
native = importlib.import_module("disentangled-vae_amd.native")
loops = importlib.import_module("disentangled-vae_amd.script_loops")
P = native.ptr
NAMES = list(importlib.import_module("disentangled-vae_amd.trainer").TENSOR_NAMES)

LOOPS_B = gc.loops_batch(lambda b: mp.make_body_plan(gc.dims_of(mi.LOOPS_CASE), b))[0]
FORWARD = mi.forward_cases(LOOPS_B)
BACKWARD = mi.backward_cases(LOOPS_B)

_ENGINES = {}


def _v3(case):
    from packages.models import models as M
    y, z, h = case
    m = M.DeepGenerativeModel_v3([513, y, z, list(h)])
    params = mi.inputs(case, 1)[0]
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=False)
    return m.cuda()


def _env(monkeypatch, mode):
    for k in ("DVAE_MODULE_PATH", "DVAE_MODULE_GENERIC", "DVAE_MODULE_INFO_BODY"):
        monkeypatch.delenv(k, raising=False)
    if mode is not None:
        monkeypatch.setenv("DVAE_MODULE_INFO_BODY", mode)


def engine(case, monkeypatch):
    """The generic engine of one _v3 per geometry, built once (the reference geometry under `force`)."""
    _env(monkeypatch, "force" if mi.forced(case) else "1")
    if case not in _ENGINES:
        m = _v3(case)
        x, y, e, _ = tensors(case, 17)
        assert mp.engine_kind(m, "M2_DEC") == "generic"
        eng = mp.engine_for(m, "M2_DEC", x, y)
        assert eng is not None and eng.kind == "generic" and eng.precision == "fp32" and eng.z_dim == case[1] and eng.y_dim == case[0]
        assert [n for n, _ in mp.vae_parameters(m, "M2_DEC")] == NAMES == list(mi.inputs(case, 1)[0])
        assert [tuple(p.shape) for p in eng.params] == [v.shape for v in mi.inputs(case, 1)[0].values()]
        _ENGINES[case] = (m, eng)
    return _ENGINES[case][1]


@functools.lru_cache(maxsize=None)
def tensors(case, B):
    """x, y, eps and the upstream gradients of a case on the device"""
    _, x, y, e = mi.inputs(case, B)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    return t(x), t(y), t(e), {k: t(v) for k, v in mi.mg.make_upstream(B, case[1]).items()}


def forward(eng, x, y, e):
    r, z, mu, lv = mp.run(eng, x, y, e)
    return dict(r=r, z=z, mu=mu, lv=lv)


def gradients(eng, out, up, key, extra=()):
    names = mi.UPSTREAMS[key]
    return torch.autograd.grad([out[k] for k in names], list(eng.params) + list(extra), [up[k] for k in names])


def host(ts, names):
    return {k: t.detach().cpu().numpy() for k, t in zip(names, ts)}


# ---- 1: outputs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,B", FORWARD, ids=[mi.case_id(*c) for c in FORWARD])
def test_forward_outputs_against_float64(case, B, monkeypatch):
    ref = mi.reference(case, B)
    eng = engine(case, monkeypatch)
    x, y, e, _ = tensors(case, B)
    out = forward(eng, x, y, e)
    assert out["r"].shape == (B, 513) and all(out[k].shape == (B, case[1]) for k in ("z", "mu", "lv"))
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(v).all() for v in got.values()) and (got["r"] > 0).all()
    label = f"[{mi.case_id(case, B)}]"
    fails, top, ratios = ref.check_outputs(got, label)
    print(f"{label} worst ratio to the bound: {top:.3f}   " + "   ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert not fails, fails


# ---- 1, 2: the 14 gradients and g_y ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,B,key,gy", BACKWARD, ids=[mi.case_id(*c) for c in BACKWARD])
def test_parameter_and_label_gradients_against_float64(case, B, key, gy, monkeypatch):
    ref = mi.reference(case, B)
    eng = engine(case, monkeypatch)
    x, y, e, up = tensors(case, B)
    if gy:
        y = y.clone().requires_grad_()
    assert mp.engine_for(_ENGINES[case][0], "M2_DEC", x, y) is eng
    got = gradients(eng, forward(eng, x, y, e), up, key, extra=[y] if gy else [])
    g = host(got, NAMES + ([mi.GY] if gy else []))
    assert not gy or g[mi.GY].shape == (B, case[0])
    label = f"[{mi.case_id(case, B, key, gy)}]"
    fails, top, ratios = ref.check_grads(g, key, label)
    fam = {f: max((v for k, v in ratios.items() if k.startswith(f)), default=0.0) for f in ("encoder.", "decoder.hidden", "decoder.reconstruction", mi.GY)}
    print(f"{label} worst ratio to the bound: {top:.3f}   " + "   ".join(f"{f} {v:.3f}" for f, v in fam.items()))
    assert (mi.GY in ratios and mi.GY_TENSOR in ratios) == gy
    for k, G in ref.truth[key].items():
        if k in g and not G.any():
            assert not g[k].any(), f"{k}: the float64 gradient is identically zero, the kernel's is not"
    assert not fails, fails


# ---- 3: the C ABI ----------------------------------------------------------------------------------------------------------------

ABI = [(mi.EDGE_CASE, 17), ((1, 1, (1, 1)), 50), ((513, 64, (16, 16)), 50), (mi.LOOPS_CASE, LOOPS_B)]


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("case,B", ABI, ids=[mi.case_id(*c) for c in ABI])
def test_c_abi_row_padded_g_y_over_a_nan_filled_buffer(case, B, monkeypatch):
    """ld_gy = y + 3 over NaNs: the padding, the rows of frames past B and everything under a NULL g_y stay unwritten; the parameter
    gradients have the same bits with and without g_y; two runs give the same bits."""
    eng = engine(case, monkeypatch)
    lib = native.load()
    x, y, e, up = tensors(case, B)
    forward(eng, x, y, e)                                    # parameters aliased, packed copies current
    plan, ws = eng._ready(B)
    Y, n = case[0], eng.n_params
    ld, tail = Y + 3, 16                                     # the rows of a whole tile past B
    head = (ctypes.byref(plan), P(eng.flat), P(ws), P(x), 513, P(y), Y, P(e), P(up["r"]), 513, P(up["mu"]), P(up["lv"]), P(up["z"]))

    def run(with_gy, ld_gy=ld):
        dst, buf = _nan(n), _nan((B + tail) * ld)
        rc = lib.dvae_module_generic_backward_y(*head, P(dst), 0, P(buf) if with_gy else None, ld_gy if with_gy else 0, native.stream())
        torch.cuda.synchronize()
        native.check(rc, "dvae_module_generic_backward_y")
        return dst, buf

    d1, b1 = run(True)
    d2, b2 = run(True)
    d0, b0 = run(False)
    body = b1[:B * ld].view(B, ld)
    assert bool(torch.isnan(body[:, Y:]).all()), "the padding between the rows of g_y was written"
    assert bool(torch.isnan(b1[B * ld:]).all()), "rows of frames past B were written"
    assert not bool(torch.isnan(body[:, :Y]).any()), "an element of g_y was not written"
    assert bool(torch.isnan(b0).all()), "something was written under a NULL g_y"
    assert torch.equal(body[:, :Y], b2[:B * ld].view(B, ld)[:, :Y]) and torch.equal(d1, d2), "two runs differ"
    assert not bool(torch.isnan(d1).any()) and torch.equal(d1, d0), "the parameter gradients depend on whether g_y was asked for"
    # _backward is _backward_y with a NULL g_y, and the tight layout holds the same label gradient
    dst = _nan(n)
    native.check(lib.dvae_module_generic_backward(*head, P(dst), 0, native.stream()), "dvae_module_generic_backward")
    tight = _nan(B * Y)
    native.check(lib.dvae_module_generic_backward_y(*head, P(_nan(n)), 0, P(tight), Y, native.stream()), "dvae_module_generic_backward_y")
    torch.cuda.synchronize()
    assert torch.equal(dst, d1) and torch.equal(tight.view(B, Y), body[:, :Y])
    # against float64 as well, so that "written" means "written with the label gradient"
    ref = mi.reference(case, B)
    g = host([d1[o:o + c].view(p.shape) for p, (o, c) in zip(eng.params, eng.spans)], NAMES)
    g[mi.GY] = body[:, :Y].cpu().numpy()
    fails, top, _ = ref.check_grads(g, "all", f"[abi {mi.case_id(case, B)}]")
    assert not fails, fails
    # refused by name, nothing written
    kept, keptg = _nan(n), _nan(B * ld)
    rc = lib.dvae_module_generic_backward_y(*head, P(kept), 0, P(keptg), Y - 1, native.stream())
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="ld_gy"):
        native.check(rc, "dvae_module_generic_backward_y")
    assert bool(torch.isnan(kept).all()) and bool(torch.isnan(keptg).all())


# ---- 4: autograd behaviour through the modules -----------------------------------------------------------------------------------

def _call(m, x, y, e):
    from packages.models import models as M
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        return m._forward_z(x, y)
    finally:
        M.Stochastic.epsilon_fn = None


def _loss(outs, up):
    r, z, mu, lv = outs
    return (r * up["r"]).sum() + (z * up["z"]).sum() + (mu * up["mu"]).sum() + (lv * up["lv"]).sum()


def test_y_grad_through_the_module_backward_grad_and_accumulation(monkeypatch):
    case, B = mi.EDGE_CASE, 17
    ref = mi.reference(case, B)
    _env(monkeypatch, "1")
    m = _v3(case)
    x, y0, e, up = tensors(case, B)
    y = y0.clone().requires_grad_()
    outs = _call(m, x, y, e)
    eng = m.__dict__.get("_dvae_engine")
    assert eng is not None and eng.kind == "generic" and type(outs[0].grad_fn).__name__ == "VaeFunctionBackward"
    _loss(outs, up).backward()
    first = y.grad.clone()
    g = {mi.GY: first.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in zip(NAMES, eng.params)}}
    fails, _, _ = ref.check_grads(g, "all", "[y.grad]")
    assert not fails, fails
    # torch.autograd.grad(loss, [y]) alone: the same bits, and no parameter gradient is touched
    before = [p.grad.clone() for p in eng.params]
    (only,) = torch.autograd.grad(_loss(_call(m, x, y, e), up), [y])
    assert torch.equal(only, first) and all(torch.equal(p.grad, b) for p, b in zip(eng.params, before))
    # a second backward accumulates
    _loss(_call(m, x, y, e), up).backward()
    assert torch.equal(y.grad, first + first) and all(torch.equal(p.grad, b + b) for p, b in zip(eng.params, before))
    # y as the output of another differentiable op (the pretrain script's classifier in small): the gradient flows on
    w = torch.full((1, case[0]), 0.5, device="cuda", requires_grad=True)
    _loss(_call(m, x, y0 * w, e), up).backward()
    half = (y0 * w).detach().requires_grad_()
    (at_half,) = torch.autograd.grad(_loss(_call(m, x, half, e), up), [half])
    want = (at_half.double() * y0.double()).sum(0, keepdim=True)
    assert w.grad is not None and bool(((w.grad.double() - want).abs() <= 1e-5 * (at_half.double() * y0.double()).abs().sum(0, keepdim=True) + 1e-30).all())
    # x.requires_grad stays a layer-path feature
    assert mp.engine_for(m, "M2_DEC", x.clone().requires_grad_(), y0) is None


def test_an_optimizer_step_between_forward_and_backward_raises(monkeypatch):
    case, B = mi.EDGE_CASE, 17
    _env(monkeypatch, "1")
    m = _v3(case)
    x, y0, e, up = tensors(case, B)
    y = y0.clone().requires_grad_()
    opt = torch.optim.Adam(list(m.encoder.parameters()) + list(m.decoder.parameters()), lr=1e-3)
    _loss(_call(m, x, y, e), up).backward()
    stale = _loss(_call(m, x, y, e), up)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        stale.backward()
    _loss(_call(m, x, y, e), up).backward()                  # a fresh forward is fine


def test_no_grad_and_a_frozen_body_stay_per_layer(monkeypatch):
    case, B = mi.EDGE_CASE, 17
    _env(monkeypatch, "1")
    m = _v3(case)
    x, y0, e, _ = tensors(case, B)
    with torch.no_grad():
        assert mp.engine_for(m, "M2_DEC", x, y0) is None
        r = _call(m, x, y0, e)[0]
    assert r.grad_fn is None
    for p in list(m.encoder.parameters()) + list(m.decoder.parameters()):
        p.requires_grad = False
    y = y0.clone().requires_grad_()
    assert mp.engine_for(m, "M2_DEC", x, y) is None
    r = _call(m, x, y, e)[0]
    assert type(r.grad_fn).__name__ != "VaeFunctionBackward"
    r.sum().backward()                                       # the layer path's own label gradient
    assert y.grad is not None and m.__dict__.get("_dvae_engine") is None


def test_y_grad_on_m2_and_on_the_resident_engine_stays_a_layer_path_feature(monkeypatch):
    from packages.models import models as M
    _env(monkeypatch, "1")
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "1")
    x, y0, e, _ = tensors((1, 16, (128, 128)), 17)
    y = y0.clone().requires_grad_()
    ref = M.DeepGenerativeModel_v3([513, 1, 16, [128, 128]]).cuda()
    assert mp.engine_kind(ref, "M2_DEC") == "resident"
    assert mp.engine_for(ref, "M2_DEC", x, y) is None and mp.engine_for(ref, "M2_DEC", x, y0).kind == "resident"
    m2 = M.DeepGenerativeModel([513, 1, 32, [256, 64]], None).cuda()
    assert mp.engine_kind(m2, "M2") == "generic" and mp.engine_for(m2, "M2", x, y) is None


def test_switch_unset_leaves_another_size_on_the_bits_of_the_layer_path(monkeypatch):
    case, B = (1, 5, (48, 200)), 50
    x, y, e, up = tensors(case, B)
    _env(monkeypatch, None)
    unset = _v3(case)
    assert mp.engine_kind(unset, "M2_DEC") is None
    a = _call(unset, x, y, e)
    assert unset.__dict__.get("_dvae_engine") is None and type(a[0].grad_fn).__name__ != "VaeFunctionBackward"
    monkeypatch.setenv("DVAE_MODULE_PATH", "layers")
    b = _call(_v3(case), x, y, e)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # and DVAE_MODULE_GENERIC does not reach this body
    _env(monkeypatch, None)
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "force")
    c = _call(_v3(case), x, y, e)
    assert all(torch.equal(u, v) for u, v in zip(a, c))


# ---- 5: the reference loop bodies ------------------------------------------------------------------------------------------------

LOOP_DIMS = [dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64)), dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))]
BODIES = [("truth", "bce"), ("classifier", "entropy")]        # the main script; the pretrain script
GRAD_BAR, LOSS_BAR = 1e-4, 1e-4                             # the project's fp32 bar (tests/train_generic_cases.py)


def _v5_loop(dims, mode, body, x, y, e, iters=3):
    """the first enc_loss.backward() and then `iters` iterations of the loop body on a fresh seeded _v5 -> (engine_kind of the body, the
    kind of the engine it built, the 26 gradients after that backward, [losses per iteration])"""
    from packages.models import models as M
    synth = importlib.import_module("disentangled-vae_amd.synth")
    torch.manual_seed(3)
    m = synth.build_model("M2_info", dims).cuda()
    mp.set_info_body(m, mode)
    kind = mp.engine_kind(m.enc_dec_clf, "M2_DEC")
    opt_body = torch.optim.Adam(m.enc_dec_clf.parameters(), lr=1e-3, betas=(0.9, 0.999))
    opt_aux = torch.optim.Adam(m.auxiliary.parameters(), lr=1e-3, betas=(0.9, 0.999))
    kw = dict(decoder_label=body[0], aux_enc=body[1], alpha=1.0, beta=10.0, gamma=10.0 if body[0] == "classifier" else 1.0)
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        one_function = type(m(x, y)[1].grad_fn).__name__ == "VaeFunctionBackward"        # z comes out of the body's one Function
        assert one_function == (kind is not None), (kind, one_function)
        L = loops.info_losses(m, x, y, **kw)
        L["enc_loss"].backward()
        grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
        for p in m.parameters():
            p.grad = None
        losses = [loops.info_step(m, opt_body, opt_aux, x, y, **kw) for _ in range(iters)]
    finally:
        M.Stochastic.epsilon_fn = None
    has_engine = m.enc_dec_clf.__dict__.get("_dvae_engine")
    return kind, (None if has_engine is None else has_engine.kind), grads, [{k: float(v) for k, v in l.items()} for l in losses]


@pytest.mark.parametrize("body", BODIES, ids=["main", "pretrain"])
@pytest.mark.parametrize("dims", LOOP_DIMS, ids=["z32_h256x64_y1", "z16_h128x128_y513"])
def test_reference_loop_bodies_on_v5_switch_on_against_off(dims, body, monkeypatch):
    _env(monkeypatch, None)
    synth = importlib.import_module("disentangled-vae_amd.synth")
    x, y, e = synth.device_batches(dims, 50, 1, 7, "cuda")[0]
    kind_off, eng_off, g_off, l_off = _v5_loop(dims, "off", body, x, y, e)
    kind_on, eng_on, g_on, l_on = _v5_loop(dims, "on", body, x, y, e)
    assert kind_off is None and eng_off is None and kind_on == "generic" and eng_on == "generic"
    assert len(g_on) == 26 == len(g_off)
    worst = {}
    for k in g_off:
        top = float(g_off[k].abs().max())
        worst[k] = float((g_on[k] - g_off[k]).abs().max()) / (top + 1e-30)
    name = max(worst, key=worst.get)
    print(f"[{body}] largest gradient difference over the tensor's maximum: {worst[name]:.2e} on {name}")
    if body[0] == "classifier":                              # through g_y and nothing else (alpha BCE is the same on both sides)
        assert all(float(g_on[k].abs().max()) > 0 for k in g_on if k.startswith("enc_dec_clf.classifier."))
    assert worst[name] <= GRAD_BAR, worst
    for a, b in zip(l_on, l_off):
        for k in a:
            rel = abs(a[k] - b[k]) / (abs(b[k]) + 1e-30)
            print(f"[{body}] {k}: {a[k]:.6f} against {b[k]:.6f} ({rel:.1e})")
            assert rel <= LOSS_BAR, (k, a[k], b[k])
    for side, l in (("on", l_on), ("off", l_off)):
        assert all(np.isfinite(v) for it in l for v in it.values()) and l[2]["enc_loss"] < l[0]["enc_loss"], (side, [it["enc_loss"] for it in l])

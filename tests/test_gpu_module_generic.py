"""The whole-model module path at any covered size -- module_path.GenericModuleEngine on dvae_module_generic_forward /
dvae_module_generic_backward, the generic rows kernel in its module-forward and module-backward modes -- against the float64 oracle
(tests/module_generic_cases.py: truth, float32 restatement in two orders, statistics, bound, inputs, cases;
tests/test_module_generic_cpu.py pins the truth against torch.float64 autograd and shows that the statistics see seeded faults).

The engine is driven as tests/test_gpu_module_oracle.py drives the resident one: module_path.engine_for(module, model, x, y), all four
outputs from module_path.run(eng, x, y, eps), gradients from torch.autograd.grad(outputs, eng.params, grad_outputs) -- an output that is
left out reaches the kernel as a null pointer.

Checks: (1) r (on log r), mu, log_var, z against float64 by the rule, and z = mu + exp(log_var / 2) eps on the kernel's own outputs;
(2) every parameter gradient per input column, the reconstruction layer also per output row, a gradient whose truth is identically zero
exactly 0.0; (3) padded leading dimensions of x, y and g_r at odd storage offsets and a stride-0 g_mu: the bits of the contiguous call;
(4) the C ABI on the engine's own plan; (5) autograd behaviour; (6) the switch; (7) three iterations of the script loop with a KL weight.

Measured on the MI355X: 46 cases, 6.3 s of wall time with the CPU references (the slowest: the 4149-frame reference, 1.0 s).  Worst
statistic / bound over all cases -- a device that errs exactly as the larger restatement draw does reaches 0.25:
  outputs        log r 0.33   mu 0.35   log_var 0.30   z 0.38   (r and z: (3, 17, (129, 127)) at ONE frame; mu, log_var: the reference geometry under force)
  gradients      encoder 0.54 ((0, 1, (1, 1)) at 50 frames)   decoder hidden layers 0.42 ((3, 17, (129, 127)), one frame)
                 reconstruction layer 0.47 ((1, 5, (48, 200)) at 50 frames); the 4149-frame batch of the tile loop 0.25
                 each upstream gradient alone and g_mu + g_lv at 17 frames: 0.26 ... 0.30
  z identity     0.64 of what is allowed; 1.89 float32 roundings of |mu| + |std eps| at worst (4149 frames)
  accumulate = 1 exactly one float32 addition per element (1.00 of one rounding) in all three cases
  KL-weighted script loop, first iteration: loss 0.02 of its bound (6e-8 relative), gradients 0.31
No gradient whose truth is identically zero came back as anything but 0.0; every bit-for-bit check holds.  The first device run failed one
check through the test's own expectation: accumulate 1 was held to prefill + gradient in the alignment gaps between the tensors as well,
where the reduce kernel writes zeros in either mode (include/dvae_train.h); the test now holds the gaps to exactly 0.0.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import module_generic_cases as mg
import train_generic_cases as gc
from impl_modules import build_model
from test_gpu_layers_scale import SENT, TAIL, owned, sent, untouched

pytestmark = pytest.mark.gpu

mp = importlib.import_module("disentangled-vae_amd.module_path")
native = importlib.import_module("disentangled-vae_amd.native")
TG = importlib.import_module("disentangled-vae_amd.trainer_generic")
P = native.ptr
U24 = 2.0 ** -24

LOOPS_B = gc.loops_batch(lambda b: TG.make_plan(gc.model_of(mg.LOOPS_CASE), gc.dims_of(mg.LOOPS_CASE), b))[0]
FORWARD = mg.forward_cases(LOOPS_B)
BACKWARD = mg.backward_cases(LOOPS_B)

_ENGINES = {}


def _load(case):
    m = build_model(gc.model_of(case), gc.dims_of(case))
    params = gc.inputs(case, 1)[0]
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return m.cuda()


def engine(case, monkeypatch):
    """The generic engine of one module per geometry, built once (the reference geometry under `force`)."""
    monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "force" if mg.forced(case) else "1")
    if case not in _ENGINES:
        m = _load(case)
        x, y, e, _ = tensors(case, 17)
        model = gc.model_of(case)
        assert mp.engine_kind(m, model) == "generic"
        eng = mp.engine_for(m, model, x, y)
        assert eng is not None and eng.kind == "generic" and eng.precision == "fp32" and eng.z_dim == case[1]
        assert [tuple(p.shape) for p in eng.params] == [v.shape for v in gc.inputs(case, 1)[0].values()]
        _ENGINES[case] = (m, eng)
    return _ENGINES[case][1]


@functools.lru_cache(maxsize=None)
def tensors(case, B):
    """x, y, eps and the upstream gradients of a case on the device"""
    _, x, y, e = gc.inputs(case, B)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    return t(x), t(y), t(e), {k: t(v) for k, v in mg.make_upstream(B, case[1]).items()}


def forward(eng, x, y, e):
    r, z, mu, lv = mp.run(eng, x, y, e)
    return dict(r=r, z=z, mu=mu, lv=lv)


def gradients(eng, out, up, key, params=None):
    names = mg.UPSTREAMS[key]
    return torch.autograd.grad([out[k] for k in names], eng.params if params is None else params, [up[k] for k in names])


def host(ts, names):
    return {k: t.detach().cpu().numpy() for k, t in zip(names, ts)}


# ---- 1: outputs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,B", FORWARD, ids=[mg.case_id(*c) for c in FORWARD])
def test_forward_outputs_against_float64(case, B, monkeypatch):
    ref = mg.reference(case, B)
    eng = engine(case, monkeypatch)
    x, y, e, _ = tensors(case, B)
    out = forward(eng, x, y, e)
    Z = case[1]
    assert out["r"].shape == (B, 513) and all(out[k].shape == (B, Z) for k in ("z", "mu", "lv"))
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(v).all() for v in got.values()) and (got["r"] > 0).all()
    label = f"[{mg.case_id(case, B)}]"
    fails, top, ratios = ref.check_outputs(got, label)
    # z from the kernel's own mu and log_var, as tests/test_gpu_module_oracle.py counts the roundings: two float32 roundings (of exp's result
    # and of the sum) of |mu| + |std eps|, and one more rounding of |std eps| for an exp accurate to one ulp where a correctly rounded
    # one errs by half of one.  The argument of exp is the float32 product fl(0.5 lv) (exact: a power of two), so the expectation is exp
    # of that float32 number in float64.
    mu, lv, z, eps = [got[k].astype(np.float64) for k in ("mu", "lv", "z")] + [ref.e.astype(np.float64)]
    arg = np.float32(0.5) * got["lv"]
    assert arg.dtype == np.float32
    se = np.exp(arg.astype(np.float64)) * eps
    err = np.abs(z - (mu + se))
    plain = float((err / (U24 * (np.abs(mu) + np.abs(se)) + 1e-300)).max())
    allowed = U24 * (2.0 * (np.abs(mu) + np.abs(se)) + np.abs(se))
    used = float((err / (allowed + 1e-300)).max())
    print(f"{label} z against mu + exp(fl(0.5 lv)) eps of the outputs: {used:.2f} of what is allowed; in float32 roundings of |mu| + |std eps|: {plain:.2f}")
    print(f"{label} worst ratio to the bound: {top:.3f}   " + "   ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert not fails, fails
    assert bool((err <= allowed).all()), (used, plain)


# ---- 2: gradients ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,B,key", BACKWARD, ids=[mg.case_id(*c) for c in BACKWARD])
def test_parameter_gradients_against_float64(case, B, key, monkeypatch):
    ref = mg.reference(case, B)
    eng = engine(case, monkeypatch)
    x, y, e, up = tensors(case, B)
    g = host(gradients(eng, forward(eng, x, y, e), up, key), ref.params)
    label = f"[{mg.case_id(case, B, key)}]"
    fails, top, ratios = ref.check_grads(g, key, label)
    fam = {f: max((v for k, v in ratios.items() if k.startswith(f)), default=0.0) for f in ("encoder.", "decoder.hidden", "decoder.reconstruction")}
    print(f"{label} worst ratio to the bound: {top:.3f}   " + "   ".join(f"{f} {v:.3f}" for f, v in fam.items()))
    for k, G in ref.truth[key].items():
        if not G.any():
            assert not g[k].any(), f"{k}: the float64 gradient is identically zero, the kernel's is not"
    assert not fails, fails


# ---- 3: strided inputs -----------------------------------------------------------------------------------------------------------

def _odd(a, ld, c0, offset):
    """a [B, n] as columns c0 .. c0 + n of a [B, ld] matrix that starts `offset` floats into its storage; the rest holds the sentinel"""
    B, n = a.shape
    buf = sent(B * ld + offset + 1)
    v = buf[offset:offset + B * ld].view(B, ld)[:, c0:c0 + n]
    v.copy_(a)
    assert v.storage_offset() % 2 == 1 and v.stride() == (ld, 1)
    return v, buf


STRIDED = [(mg.EDGE_CASE, 17), (mg.EDGE_CASE, 50), ((513, 64, (16, 16)), 50), ((0, 32, (256, 64)), 50), (mg.LOOPS_CASE, LOOPS_B)]


@pytest.mark.parametrize("case,B", STRIDED, ids=[mg.case_id(*c) for c in STRIDED])
def test_padded_rows_at_odd_offsets_give_the_bits_of_the_contiguous_call(case, B, monkeypatch):
    """x = wide[:, 3:516], y = wide_y[:, 1:1 + y_dim], g_r = wide_g[:, 2:515], each at an odd storage offset (no row starts on a 16-byte
    boundary), and g_mu expanded from one row (stride 0) through torch.autograd.grad's grad_outputs."""
    eng = engine(case, monkeypatch)
    x, y, e, up = tensors(case, B)
    Z = case[1]
    up = dict(up, mu=up["mu"][:1].expand(B, Z).contiguous())
    base = forward(eng, x, y, e)
    gbase = gradients(eng, base, up, "all")
    xs, xbuf = _odd(x, 521, 3, 2)
    ys, ybuf = (None, None) if y is None else _odd(y, case[0] + 4, 1, 2)
    gs_r, gbuf = _odd(up["r"], 519, 2, 1)
    ups = dict(up, r=gs_r, mu=up["mu"][:1].expand(B, Z))
    assert ups["mu"].stride() == (0, 1)
    out = forward(eng, xs, ys, e)
    for k in out:
        assert torch.equal(out[k], base[k]), f"{k} differs under padded x / y"
    for gs, gb, name in zip(gradients(eng, out, ups, "all"), gbase, gc.inputs(case, 1)[0]):
        assert torch.equal(gs, gb), f"gradient of {name} differs under padded x / y / g_r and an expanded g_mu"
    assert int((xbuf == SENT).sum()) == xbuf.numel() - x.numel(), "the padding around x was written"
    assert int((gbuf == SENT).sum()) == gbuf.numel() - up["r"].numel(), "the padding around g_r was written"
    if y is not None:
        assert int((ybuf == SENT).sum()) == ybuf.numel() - y.numel(), "the padding around y was written"


# ---- 4: the C ABI ----------------------------------------------------------------------------------------------------------------

ABI = [(mg.EDGE_CASE, 17), ((0, 32, (256, 64)), 50), (mg.LOOPS_CASE, LOOPS_B)]


def _abi(case, B, monkeypatch):
    eng = engine(case, monkeypatch)
    x, y, e, up = tensors(case, B)
    forward(eng, x, y, e)                                    # parameters aliased, packed copies current
    plan, ws = eng._ready(B)
    head = (ctypes.byref(plan), P(eng.flat), P(ws), P(x), 513, P(y), case[0], P(e))
    return eng, native.load(), head, up


@pytest.mark.parametrize("case,B", ABI, ids=[mg.case_id(*c) for c in ABI])
def test_c_abi_forward_padded_ld_r_and_null_out_z(case, B, monkeypatch):
    eng, lib, head, _ = _abi(case, B, monkeypatch)
    Z = case[1]

    def fwd(ld_r, with_z=True):
        bufs = dict(r=sent(B * ld_r + TAIL), mu=sent(B * Z + TAIL), lv=sent(B * Z + TAIL), z=sent(B * Z + TAIL))
        native.check(lib.dvae_module_generic_forward(*head, P(bufs["r"]), ld_r, P(bufs["mu"]), P(bufs["lv"]), P(bufs["z"]) if with_z else None, 1,
                                                     native.stream()), "dvae_module_generic_forward")
        torch.cuda.synchronize()
        return bufs

    tight, wide, noz = fwd(513), fwd(520), fwd(520, with_z=False)
    want = {k: owned(tight[k], B, 513 if k == "r" else Z) for k in tight}
    for run, what in ((wide, "ld_r 520"), (noz, "ld_r 520, out_z NULL")):
        for k in ("r", "mu", "lv") + (("z",) if run is wide else ()):
            assert torch.equal(owned(run[k], B, 513 if k == "r" else Z, 520 if k == "r" else None), want[k]), f"{what}: {k} differs from the ld_r 513 call"
    untouched(noz["z"])
    kept = sent(B * 513 + TAIL)
    rc = lib.dvae_module_generic_forward(*head, P(kept), 512, P(noz["z"]), P(noz["z"]), None, 1, native.stream())
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="ld_r"):
        native.check(rc, "dvae_module_generic_forward")
    untouched(kept)
    untouched(noz["z"])


@pytest.mark.parametrize("case,B", ABI, ids=[mg.case_id(*c) for c in ABI])
def test_c_abi_backward_accumulate_and_refused_ld_gr(case, B, monkeypatch):
    eng, lib, head, up = _abi(case, B, monkeypatch)
    n = eng.n_params

    def bwd(dst, accumulate, ld_gr=513):
        rc = lib.dvae_module_generic_backward(*head, P(up["r"]), ld_gr, P(up["mu"]), P(up["lv"]), P(up["z"]), P(dst), accumulate, native.stream())
        torch.cuda.synchronize()
        return rc

    first = sent(n + TAIL)
    native.check(bwd(first, 0), "dvae_module_generic_backward")
    g0 = owned(first, 1, n)
    # accumulate 0 on another prefill: the same bits, i.e. nothing of either prefill is left
    other = sent(n + TAIL)
    other[:n] = 0.75
    native.check(bwd(other, 0), "dvae_module_generic_backward")
    assert torch.equal(owned(other, 1, n), g0), "accumulate 0 left some of the prefill in place"
    # the views autograd hands out hold the same numbers
    via = gradients(eng, forward(eng, *tensors(case, B)[:3]), up, "all")
    for g, (o, cnt) in zip(via, eng.spans):
        assert torch.equal(g.reshape(-1), g0[0, o:o + cnt])
    # accumulate 1: prefill + gradient, one float32 addition per element
    pre = torch.from_numpy((np.random.default_rng(17).standard_normal(n) * 1e-3).astype(np.float32)).cuda()
    acc = sent(n + TAIL)
    acc[:n] = pre
    native.check(bwd(acc, 1), "dvae_module_generic_backward")
    # (the alignment gaps between the tensors belong to no parameter: the reduce kernel leaves zeros there in either mode)
    inside = torch.zeros(n, dtype=torch.bool, device="cuda")
    for o, cnt in eng.spans:
        inside[o:o + cnt] = True
    want = torch.where(inside, pre.double() + g0[0].double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    assert not bool(g0[0][~inside].any()), "accumulate 0 left something in an alignment gap"
    err = (owned(acc, 1, n)[0].double() - want).abs()
    over = float((err / (U24 * want.abs() + 1e-300)).max())
    print(f"accumulate 1 against prefill + gradient: {over:.2f} float32 roundings of the sum (1 allowed)")
    assert bool((err <= U24 * want.abs()).all()), over
    # a g_r whose rows are shorter than 513: refused, named, nothing written
    kept = sent(n + TAIL)
    with pytest.raises(RuntimeError, match="ld_gr"):
        native.check(bwd(kept, 0, ld_gr=512), "dvae_module_generic_backward")
    untouched(kept)


# ---- 5: autograd behaviour -------------------------------------------------------------------------------------------------------

def test_frozen_parameters_get_no_gradient_and_the_others_keep_their_bits(monkeypatch):
    case, B = mg.EDGE_CASE, 17
    eng = engine(case, monkeypatch)
    names = list(gc.inputs(case, 1)[0])
    x, y, e, up = tensors(case, B)
    full = dict(zip(names, gradients(eng, forward(eng, x, y, e), up, "all")))
    frozen = ("decoder.reconstruction.bias", "encoder.hidden.0.weight")
    by_name = dict(zip(names, eng.params))
    try:
        for k in frozen:
            by_name[k].requires_grad = False
        out = forward(eng, x, y, e)
        torch.autograd.backward([out[k] for k in mg.UPSTREAMS["all"]], [up[k] for k in mg.UPSTREAMS["all"]])
        for k, p in by_name.items():
            if k in frozen:
                assert p.grad is None, k
            else:
                assert p.grad is not None and torch.equal(p.grad, full[k]), k
    finally:
        for p in eng.params:
            p.requires_grad = True
            p.grad = None


def test_a_parameter_changed_between_forward_and_backward_raises(monkeypatch):
    case, B = mg.EDGE_CASE, 17
    eng = engine(case, monkeypatch)
    x, y, e, up = tensors(case, B)
    out = forward(eng, x, y, e)
    p = eng.params[3]
    with torch.no_grad():
        p.add_(0.0)                                          # the bits stay, the version moves
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        gradients(eng, out, up, "all")
    # a replaced storage raises as well, and the engine takes the parameter back into its flat buffer at the next forward
    out = forward(eng, x, y, e)
    keep = p.data
    try:
        p.data = keep.clone()
        with pytest.raises(RuntimeError, match="storage was replaced"):
            gradients(eng, out, up, "all")
    finally:
        p.data = keep
    again = forward(eng, x, y, e)
    gradients(eng, again, up, "all")


def test_two_runs_give_the_same_bits(monkeypatch):
    for case, B in ((mg.EDGE_CASE, 50), (mg.LOOPS_CASE, LOOPS_B)):
        eng = engine(case, monkeypatch)
        x, y, e, up = tensors(case, B)
        a = forward(eng, x, y, e)
        ga = gradients(eng, a, up, "all")
        b = forward(eng, x, y, e)
        gb = gradients(eng, b, up, "all")
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert all(torch.equal(u, v) for u, v in zip(ga, gb))


# ---- 6: the switch ---------------------------------------------------------------------------------------------------------------

def _loop_step(m, model, x, y, e, kl_weight=1.0):
    """one iteration of the script's loop body without the optimizer: (loss, recon, kl), (r, mu, lv), gradients by name"""
    from packages.models import models as M
    from packages.models.utils import elbo
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        r, mu, lv = m(x) if model == "M1" else m(x, y)
    finally:
        M.Stochastic.epsilon_fn = None
    _, recon, kl = elbo(x, r, mu, lv, 1e-8)
    loss = recon + kl_weight * kl
    for p in m.parameters():
        p.grad = None
    loss.backward()
    return (loss, recon, kl), (r, mu, lv), {k: p.grad for k, p in m.named_parameters()}


def test_switch_unset_leaves_a_non_reference_module_on_the_bits_of_the_layer_path(monkeypatch):
    case, B = (1, 5, (48, 200)), 50
    model = gc.model_of(case)
    x, y, e, _ = tensors(case, B)
    monkeypatch.delenv("DVAE_MODULE_GENERIC", raising=False)
    monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
    unset = _load(case)
    assert mp.engine_kind(unset, model) is None
    a = _loop_step(unset, model, x, y, e)
    assert unset.__dict__.get("_dvae_engine") is None
    monkeypatch.setenv("DVAE_MODULE_PATH", "layers")
    b = _loop_step(_load(case), model, x, y, e)
    assert all(torch.equal(u, v) for u, v in zip(a[0] + a[1], b[0] + b[1]))
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_switch_on_takes_the_generic_engine_as_one_function(monkeypatch):
    case, B = (1, 5, (48, 200)), 50
    model = gc.model_of(case)
    x, y, e, _ = tensors(case, B)
    monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "1")
    m = _load(case)
    assert mp.engine_kind(m, model) == "generic"
    from packages.models import models as M
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        r, mu, lv = m(x, y)
    finally:
        M.Stochastic.epsilon_fn = None
    eng = m.__dict__.get("_dvae_engine")
    assert eng is not None and eng.kind == "generic"
    assert r.grad_fn is mu.grad_fn is lv.grad_fn and type(r.grad_fn).__name__ == "VaeFunctionBackward"
    # inference stays on the per-layer kernels, and set_generic(module, "off") takes this module back to them
    with torch.no_grad():
        assert mp.engine_for(m, model, x, y) is None
    mp.set_generic(m, "off")
    assert mp.engine_kind(m, model) is None and mp.engine_for(m, model, x, y) is None
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        r2 = m(x, y)[0]
    finally:
        M.Stochastic.epsilon_fn = None
    assert type(r2.grad_fn).__name__ != "VaeFunctionBackward"
    assert float((r2.detach() / r.detach() - 1).abs().max()) < 1e-4


# ---- 7: a loss the fused step lacks ----------------------------------------------------------------------------------------------

def _elbo_upstreams(out, x, B, W, dtype):
    """(g_r, g_z, g_mu, g_lv) of recon + W KL (packages/models/utils.py: elbo's two terms) at the outputs `out`, in `dtype` arithmetic"""
    r, mu, lv, x = (np.asarray(a).astype(dtype) for a in (out["r"], out["mu"], out["lv"], x))
    one, inv = dtype(1), dtype(1) / dtype(B)
    return (one / r - x / (r * r)) * inv, None, dtype(W) * mu * inv, dtype(W) * dtype(-0.5) * (one - np.exp(lv)) * inv


def test_script_loop_with_a_kl_weight_runs_on_the_generic_engine(monkeypatch):
    """Three iterations of the script loop -- module forward, elbo terms in torch with the KL term weighted by 0.25, loss.backward(), stock
    torch.optim.Adam -- at z 32 / h (256, 64) / M1 on the generic engine.  The first iteration's loss and gradients against the float64
    truth of recon + 0.25 KL (the float64 oracle's loss and the composed backward from the loss's own upstream gradients) by the rule."""
    case, B, W = (0, 32, (256, 64)), 50, 0.25
    model = gc.model_of(case)
    ref = mg.reference(case, B)
    x, y, e, _ = tensors(case, B)
    monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "1")
    m = _load(case)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    # float64: loss = mean_b sum_k (x / r - log(x + eps) + log r - 1) + W mean_b sum_j -0.5 (lv - mu^2 - exp lv); its upstream gradients
    x64, o = ref.x.astype(np.float64), ref.out
    recon = float(np.sum(x64 / o["r"] - np.log(x64 + 1e-8) + o["a"] - 1.0) / B)
    kl = float(np.sum(-0.5 * (o["lv"] - o["mu"] ** 2 - np.exp(o["lv"]))) / B)
    runs = {}
    for name, dtype, hook in (("truth", np.float64, None), ("numpy", np.float32, None), ("k-steps", np.float32, mg.gg.StepOrderF32(ref.slice_frames, case[1]))):
        args = (case, ref.params, ref.x, ref.y, ref.e)
        ups = _elbo_upstreams(mg.run(*args, {}, dtype, hook)[0], ref.x, B, W, dtype)        # of this run's own outputs, in its own arithmetic
        runs[name] = mg.run(*args, {"kl": ups}, dtype, hook)[1]["kl"]
    truth = runs["truth"]
    fig32 = mg.mc.merge(mg.mc.grad_figures(runs["numpy"], truth), mg.mc.grad_figures(runs["k-steps"], truth))
    losses = []
    for it in range(3):
        (loss, rec_t, kl_t), _, grads = _loop_step(m, model, x, y, e, W)
        if it == 0:
            eng = m.__dict__.get("_dvae_engine")
            assert eng is not None and eng.kind == "generic" and type(loss.grad_fn).__name__ != "VaeFunctionBackward"
            g = {k: v.detach().cpu().numpy() for k, v in grads.items()}
            got = (float(rec_t), float(kl_t), float(loss))
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
    # the loss: a float32 mean of B * 513 positive terms, each within the rule's bound on log r of its own size -- the bound of log r
    # (relative to max(1, max |a|)) on every term plus one float32 rounding per term and for the sum
    out_b = mg.mc.gc.bound(ref.out_fig["r"])[0] * max(1.0, float(np.abs(o["a"]).max()))
    terms = np.abs(x64 / o["r"]) * out_b + out_b + U24 * (np.abs(x64 / o["r"]) + np.abs(np.log(x64 + 1e-8)) + np.abs(o["a"]) + 1.0)
    loss_bound = 4.0 * (float(terms.sum()) / B + U24 * abs(recon)) + 4.0 * W * 4.0 * U24 * float(np.sum(np.abs(o["lv"]) + o["mu"] ** 2 + np.exp(o["lv"]))) / B
    want = recon + W * kl
    print(f"[kl-weighted loop] loss {got[2]:.6f} against {want:.6f}: {abs(got[2] - want) / loss_bound:.2f} of its bound {loss_bound:.2e}; "
          f"losses of the three iterations {losses}")
    assert abs(got[2] - want) <= loss_bound, (got, want, loss_bound)
    figs = mg.mc.grad_figures(g, truth)
    fails, top, _ = mg.mc.check(figs, g, truth, fig32, None, "[kl-weighted loop]")
    print(f"[kl-weighted loop] worst ratio to the bound: {top:.3f}")
    assert not fails, fails

"""The whole-model module path -- dvae_module_forward / dvae_module_backward, the 8-wave rows kernel in its forward-only mode and in its
backward-from-upstream-gradients mode -- against the float64 oracle (tests/module_cases.py: truth, restatements, statistics, bound and
inputs; tests/test_module_oracle_cpu.py pins the truth against torch.float64 autograd and shows that the statistics see the seeded faults).

The engine is driven directly: module_path.engine_for(module, model, x, y), all four outputs from module_path.run(eng, x, y, eps),
gradients from torch.autograd.grad(outputs, eng.params, grad_outputs) -- an output that is left out reaches the kernel as a null pointer.

Cases.  M1; M2 y 1; M2 y 513; M2_DEC y 1 -- at 1, 31, 32, 33 frames (one tile of 32, short, full, one frame over), 8192 (256 full tiles:
the whole grid, no loop), 8193 (tile 257 holds one live frame: the persistent loop and the forward-only restart of the weight stream)
and 16417 (three rounds, ragged) under bf16x3 with all four upstream gradients; at 33 and 8193 also each upstream gradient alone and
g_mu + g_lv without g_r; DVAE_MODULE_PRECISION=bf16 for M1 and M2 y 513 at 33 and 8193 with every upstream combination.
Checks: (1) r (on log r), mu, log_var, z against float64 by the rule, and z = mu + exp(0.5 log_var) eps on the kernel's own outputs;
(2) every parameter gradient per input column, the reconstruction layer also per output row (bin 512), a gradient whose truth is
identically zero exactly 0.0; (3) padded leading dimensions of x, y and g_r at odd storage offsets and a stride-0 g_mu: the bits of the
contiguous call; (4) the C ABI on the engine's own plan: ld_r 520 into sentinel-filled buffers, out_z NULL, accumulate 0 / 1, ld_gr 512
refused by name; (5) needs_input_grad.

Measured on the MI355X: 139 cases, 56 s of wall time with the CPU references (the first test of an 8193- or 16417-frame case makes its
reference: 4 ... 7 s; every other test under 2.3 s).  Worst statistic / bound over all cases -- a device that errs exactly as the larger
restatement draw does reaches 0.25:
  outputs, bf16x3     log r 0.23   mu 0.27   log_var 0.27   z 0.29          bf16: 0.25 each (the device rounds as the restatement does)
  gradients, bf16x3   encoder 0.36 (M2 y 513, 33 frames, g_r alone)   decoder hidden layers 0.32 (M2 y 513, 32 frames)
                      reconstruction layer 0.73 (M1, ONE frame: weight column 31, a decoder unit 250 times quieter than the median one); 0.39 elsewhere
  gradients, bf16     0.31 under the rule; under the stated bar encoder layer 1's weight reaches 0.299 of its maximum (bar 0.3, cosine
                      0.9953) with g_mu alone at 8193 frames of M1 and 0.258 with g_lv alone -- the figures of the bf16 restatement itself
  z identity          0.69 of what is allowed; 2.02 float32 roundings of |mu| + |std eps| at worst (two of 32 cases above 2.0: M2 y 1 at
                      16417 frames 2.02, M2 y 513 bf16 at 8193 frames 2.01), 2.66 against exp(0.5 log_var) without the rounded argument
  accumulate = 1      exactly one float32 addition per element (1.00 of one rounding)
No gradient whose truth is identically zero came back as anything but 0.0; every bit-for-bit check holds.
The first device run was made with the float32 restatement's two orders and the grad_columns policy draw alone and read 2.50 (M1, one
frame, reconstruction weight column 31), 2.24 and 1.55 (M2 y 1 at 31 and 8193 frames, ONE element of the reconstruction bias per row)
on three figures -- every other figure under 1.0.  None was a fault of the kernel: the absolute errors of those elements were 0.3 and
2.4 times the median element's, their truths sums that cancel to 1e-6 of their terms.  What was added to the restatements for them,
each from the code and none from a device figure, is written out in tests/module_cases.py: the policies' exp and tanh in the float32
draw, the three-product float32-accumulated draw of bf16x3, and the operand-format term of the per-row bias statistic.  The margin of 4
did not move.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import module_cases as mc
from impl_modules import build_model
from test_gpu_layers_scale import SENT, TAIL, owned, sent, untouched

pytestmark = pytest.mark.gpu

mp = importlib.import_module("disentangled-vae_amd.module_path")
native = importlib.import_module("disentangled-vae_amd.native")
P = native.ptr

FRAMES = [1, 31, 32, 33, 8192, 8193, 16417]
BF16_MODELS = [("M1", 0), ("M2", 513)]
U24 = 2.0 ** -24

FORWARD = [(m, y, B, "bf16x3") for m, y in mc.MODELS for B in FRAMES] + [(m, y, B, "bf16") for m, y in BF16_MODELS for B in mc.FULL_CROSS_AT]
BACKWARD = [(m, y, B, p, key) for m, y, B, p in FORWARD for key in (mc.UPSTREAMS if B in mc.FULL_CROSS_AT else ("all",))]


def _id(c):
    return "{}-y{}-B{}-{}".format(*c[:4]) + ("-" + c[4] if len(c) > 4 else "")


_ENGINES = {}


def engine(model, y_dim, precision, monkeypatch):
    """The engine of one module per (model, y_dim, precision), built once: the precision is read when the engine is built."""
    key = (model, y_dim, precision)
    if key not in _ENGINES:
        monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
        monkeypatch.setenv("DVAE_MODULE_PRECISION", precision)
        params = mc.params_of(model, y_dim)
        m = build_model("M2_info" if model == "M2_DEC" else model, mc.gc.dims_of(y_dim))
        body = m.enc_dec_clf if model == "M2_DEC" else m
        body.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=model != "M2_DEC")
        m.cuda()
        x, y, e, _ = tensors(model, y_dim, 33)
        eng = mp.engine_for(body, model, x, y)
        assert eng is not None and eng.precision == precision and eng.model == model
        assert [tuple(p.shape) for p in eng.params] == [v.shape for v in params.values()]
        _ENGINES[key] = (m, eng)
    return _ENGINES[key][1]


@functools.lru_cache(maxsize=None)
def tensors(model, y_dim, B):
    """x, y, eps and the upstream gradients of a case on the device"""
    r = mc.reference(model, y_dim, B)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    return t(r.x), t(r.y), t(r.e), {k: t(v) for k, v in r.up.items()}


def forward(eng, x, y, e):
    r, z, mu, lv = mp.run(eng, x, y, e)
    return dict(r=r, z=z, mu=mu, lv=lv)


def gradients(eng, out, up, key, params=None):
    """the 14 parameter gradients for the upstream gradients of `key`; the other outputs are not given to autograd at all"""
    names = mc.UPSTREAMS[key]
    return torch.autograd.grad([out[k] for k in names], eng.params if params is None else params, [up[k] for k in names])


def host(ts, names):
    return {k: t.detach().cpu().numpy() for k, t in zip(names, ts)}


@pytest.mark.parametrize("model,y_dim,B,precision", FORWARD, ids=[_id(c) for c in FORWARD])
def test_forward_outputs_against_float64(model, y_dim, B, precision, monkeypatch):
    ref = mc.reference(model, y_dim, B)
    eng = engine(model, y_dim, precision, monkeypatch)
    x, y, e, _ = tensors(model, y_dim, B)
    out = forward(eng, x, y, e)
    assert out["r"].shape == (B, 513) and all(out[k].shape == (B, 16) for k in ("z", "mu", "lv"))
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    assert all(np.isfinite(v).all() for v in got.values()) and (got["r"] > 0).all()
    label = f"[{_id((model, y_dim, B, precision))}]"
    fails, top, _ = ref.check_outputs(got, precision, label)
    # z from the kernel's own mu and log_var, within two float32 roundings (of exp's result and of the sum) of |mu| + |std eps|, plus two
    # terms from the code (csrc/fused_tiles.hpp, PolBF16::exp_ = v_exp_f32(v * log2 e)): the argument is rounded to float32, which moves
    # the result by up to 0.5 |lv| roundings -- so the expectation takes exp2 AT that rounded argument -- and v_exp_f32 is accurate to one
    # ulp where a correctly rounded exp errs by half of one: one more rounding of |std eps| alone.
    mu, lv, z, eps = [got[k].astype(np.float64) for k in ("mu", "lv", "z")] + [ref.e.astype(np.float64)]
    arg = (np.float32(0.5) * got["lv"]) * mc.PolicyElementwiseF32.LOG2E
    assert arg.dtype == np.float32
    se = np.exp2(arg.astype(np.float64)) * eps
    err = np.abs(z - (mu + se))
    plain = float((err / (U24 * (np.abs(mu) + np.abs(se)) + 1e-300)).max())
    allowed = U24 * (2.0 * (np.abs(mu) + np.abs(se)) + np.abs(se))
    used = float((err / (allowed + 1e-300)).max())
    natural = float((np.abs(z - (mu + np.exp(0.5 * lv) * eps)) / (U24 * (np.abs(mu) + np.abs(np.exp(0.5 * lv) * eps)) + 1e-300)).max())
    print(f"{label} z against mu + exp2(fl(0.5 lv log2 e)) eps of the outputs: {used:.2f} of what is allowed; in float32 roundings of "
          f"|mu| + |std eps|: {plain:.2f}, against exp(0.5 lv) itself: {natural:.2f}")
    print(f"{label} worst ratio to the bound: {top:.3f}")
    assert not fails, fails
    assert bool((err <= allowed).all()), (used, plain)


@pytest.mark.parametrize("model,y_dim,B,precision,key", BACKWARD, ids=[_id(c) for c in BACKWARD])
def test_parameter_gradients_against_float64(model, y_dim, B, precision, key, monkeypatch):
    ref = mc.reference(model, y_dim, B)
    eng = engine(model, y_dim, precision, monkeypatch)
    x, y, e, up = tensors(model, y_dim, B)
    g = host(gradients(eng, forward(eng, x, y, e), up, key), ref.params)
    label = f"[{_id((model, y_dim, B, precision, key))}]"
    fails, top, ratios = ref.check_grads(g, key, precision, label)
    fam = {f: max((v for k, v in ratios.items() if k.startswith(f)), default=0.0) for f in ("encoder.", "decoder.hidden", "decoder.reconstruction")}
    print(f"{label} worst ratio to the bound: {top:.3f}   " + "   ".join(f"{f} {v:.3f}" for f, v in fam.items()))
    for k, G in ref.truth[key].items():
        if not G.any():
            assert not g[k].any(), f"{k}: the float64 gradient is identically zero, the kernel's is not"
    assert not fails, fails


def _odd(a, ld, c0, offset):
    """a [B, n] as columns c0 .. c0 + n of a [B, ld] matrix that starts `offset` floats into its storage; the rest holds the sentinel"""
    B, n = a.shape
    buf = sent(B * ld + offset + 1)
    v = buf[offset:offset + B * ld].view(B, ld)[:, c0:c0 + n]
    v.copy_(a)
    assert v.storage_offset() % 2 == 1 and v.stride() == (ld, 1)
    return v, buf


STRIDED = [(m, y, 33) for m, y in mc.MODELS] + [("M2", 513, 8193), ("M2", 1, 8193)]


@pytest.mark.parametrize("model,y_dim,B", STRIDED, ids=["{}-y{}-B{}".format(*c) for c in STRIDED])
def test_padded_rows_at_odd_offsets_give_the_bits_of_the_contiguous_call(model, y_dim, B, monkeypatch):
    """x = wide[:, 3:516], y = wide_y[:, 1:2] / [:, 1:514], g_r = wide_g[:, 2:515], each at an odd storage offset (no row starts on a
    16-byte boundary), and g_mu expanded from one row (stride 0) through torch.autograd.grad's grad_outputs."""
    eng = engine(model, y_dim, "bf16x3", monkeypatch)
    x, y, e, up = tensors(model, y_dim, B)
    up = dict(up, mu=up["mu"][:1].expand(B, 16).contiguous())
    base = forward(eng, x, y, e)
    gbase = gradients(eng, base, up, "all")
    xs, xbuf = _odd(x, 521, 3, 2)
    ys = None if y is None else _odd(y, y_dim + 4, 1, 2)[0]
    ups = dict(up, r=_odd(up["r"], 519, 2, 1)[0], mu=up["mu"][:1].expand(B, 16))
    assert ups["mu"].stride() == (0, 1)
    out = forward(eng, xs, ys, e)
    for k in out:
        assert torch.equal(out[k], base[k]), f"{k} differs under padded x / y"
    for gs, gb, name in zip(gradients(eng, out, ups, "all"), gbase, mc.reference(model, y_dim, B).params):
        assert torch.equal(gs, gb), f"gradient of {name} differs under padded x / y / g_r and an expanded g_mu"
    assert int((xbuf == SENT).sum()) == xbuf.numel() - x.numel(), "the padding around x was written"


ABI = [("M2", 513, 33), ("M2", 513, 8193), ("M1", 0, 33), ("M2_DEC", 1, 8193)]


def _abi(model, y_dim, B, monkeypatch):
    eng = engine(model, y_dim, "bf16x3", monkeypatch)
    x, y, e, up = tensors(model, y_dim, B)
    forward(eng, x, y, e)                                    # parameters aliased, weight copies current
    plan, ws = eng._ready(B)
    head = (ctypes.byref(plan), P(eng.flat), P(ws), P(x), 513, P(y), y_dim, P(e))
    return eng, native.load(), head, up


@pytest.mark.parametrize("model,y_dim,B", ABI, ids=["{}-y{}-B{}".format(*c) for c in ABI])
def test_c_abi_forward_padded_ld_r_and_null_out_z(model, y_dim, B, monkeypatch):
    eng, lib, head, _ = _abi(model, y_dim, B, monkeypatch)

    def fwd(ld_r, with_z=True):
        bufs = dict(r=sent(B * ld_r + TAIL), mu=sent(B * 16 + TAIL), lv=sent(B * 16 + TAIL), z=sent(B * 16 + TAIL))
        native.check(lib.dvae_module_forward(*head, P(bufs["r"]), ld_r, P(bufs["mu"]), P(bufs["lv"]), P(bufs["z"]) if with_z else None, 1,
                                             native.stream()), "dvae_module_forward")
        torch.cuda.synchronize()
        return bufs

    tight, wide, noz = fwd(513), fwd(520), fwd(520, with_z=False)
    want = {k: owned(tight[k], B, 513 if k == "r" else 16) for k in tight}
    for run, what in ((wide, "ld_r 520"), (noz, "ld_r 520, out_z NULL")):
        for k in ("r", "mu", "lv") + (("z",) if run is wide else ()):
            assert torch.equal(owned(run[k], B, 513 if k == "r" else 16, 520 if k == "r" else None), want[k]), f"{what}: {k} differs from the ld_r 513 call"
    untouched(noz["z"])


@pytest.mark.parametrize("model,y_dim,B", ABI, ids=["{}-y{}-B{}".format(*c) for c in ABI])
def test_c_abi_backward_accumulate_and_refused_ld_gr(model, y_dim, B, monkeypatch):
    eng, lib, head, up = _abi(model, y_dim, B, monkeypatch)
    n = eng.n_params

    def bwd(dst, accumulate, ld_gr=513):
        rc = lib.dvae_module_backward(*head, P(up["r"]), ld_gr, P(up["mu"]), P(up["lv"]), P(up["z"]), P(dst), accumulate, native.stream())
        torch.cuda.synchronize()
        return rc

    first = sent(n + TAIL)
    native.check(bwd(first, 0), "dvae_module_backward")
    g0 = owned(first, 1, n)
    # accumulate 0 on another prefill: the same bits, i.e. nothing of either prefill is left
    other = sent(n + TAIL)
    other[:n] = 0.75
    native.check(bwd(other, 0), "dvae_module_backward")
    assert torch.equal(owned(other, 1, n), g0), "accumulate 0 left some of the prefill in place"
    # the views autograd hands out hold the same numbers
    via = gradients(eng, forward(eng, *tensors(model, y_dim, B)[:3]), up, "all")
    for g, (o, cnt) in zip(via, eng.spans):
        assert torch.equal(g.reshape(-1), g0[0, o:o + cnt])
    # accumulate 1: prefill + gradient, one float32 addition per element
    pre = torch.from_numpy((np.random.default_rng(17).standard_normal(n) * 1e-3).astype(np.float32)).cuda()
    acc = sent(n + TAIL)
    acc[:n] = pre
    native.check(bwd(acc, 1), "dvae_module_backward")
    want = pre.double() + g0[0].double()
    err = (owned(acc, 1, n)[0].double() - want).abs()
    over = float((err / (U24 * want.abs() + 1e-300)).max())
    print(f"accumulate 1 against prefill + gradient: {over:.2f} float32 roundings of the sum (1 allowed)")
    assert bool((err <= U24 * want.abs()).all()), over
    # a g_r whose rows are shorter than 513: refused, named, nothing written
    kept = sent(n + TAIL)
    with pytest.raises(RuntimeError, match="ld_gr"):
        native.check(bwd(kept, 0, ld_gr=512), "dvae_module_backward")
    untouched(kept)


def test_frozen_parameters_get_no_gradient_and_the_others_keep_their_bits(monkeypatch):
    model, y_dim, B = "M2", 513, 33
    eng = engine(model, y_dim, "bf16x3", monkeypatch)
    names = list(mc.reference(model, y_dim, B).params)
    x, y, e, up = tensors(model, y_dim, B)
    full = dict(zip(names, gradients(eng, forward(eng, x, y, e), up, "all")))
    frozen = ("decoder.reconstruction.bias", "encoder.hidden.0.weight")
    by_name = dict(zip(names, eng.params))
    try:
        for k in frozen:
            by_name[k].requires_grad = False
        out = forward(eng, x, y, e)
        torch.autograd.backward([out[k] for k in mc.UPSTREAMS["all"]], [up[k] for k in mc.UPSTREAMS["all"]])
        for k, p in by_name.items():
            if k in frozen:
                assert p.grad is None, k
            else:
                assert p.grad is not None and torch.equal(p.grad, full[k]), k
    finally:
        for p in eng.params:
            p.requires_grad = True
            p.grad = None

"""tests/module_cases.py on the CPU: the composed backward from upstream gradients against torch.float64 autograd of the reference modules,
the restatements inside their own rule, and seeded faults -- what the rows kernel's forward-only and upstream-gradient modes could get
wrong -- each at least 10 x over the rule's bound in one of the statistics."""
import numpy as np
import pytest
import torch

import grad_columns as gc
import module_cases as mc
from impl_modules import build_model

B = 33
IDS = ["{}-y{}".format(*m) for m in mc.MODELS]


def _autograd(model, y_dim, key):
    """(outputs, gradients) of the reference modules in torch.float64 on the CPU for the loss sum(r g_r) + sum(z g_z) + sum(mu g_mu) +
    sum(lv g_lv) over the upstream gradients of `key`."""
    from packages.models import models as M
    r = mc.reference(model, y_dim, B)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
    m = build_model("M2_info" if model == "M2_DEC" else model, r.dims).double()
    body = m.enc_dec_clf if model == "M2_DEC" else m
    body.load_state_dict({k: t(v) for k, v in r.params.items()}, strict=model != "M2_DEC")
    x, y, e = t(r.x), t(r.y), t(r.e)
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        if model == "M1":
            z, mu, lv = m.encoder(x)
            rec = m.decoder(z)
        elif model == "M2":
            z, mu, lv = M._encode_xy(m.encoder, x, y)
            rec = M._decode_zy(m.decoder, z, y)
        else:
            rec, z, mu, lv = m(x, y)
    finally:
        M.Stochastic.epsilon_fn = None
    outs = dict(r=rec, z=z, mu=mu, lv=lv)
    loss = sum((outs[k] * t(r.up[k])).sum() for k in mc.UPSTREAMS[key])
    named = dict(body.named_parameters())
    got = torch.autograd.grad(loss, [named[k] for k in r.params], allow_unused=True)
    grads = {k: np.zeros(r.params[k].shape) if g is None else g.numpy() for k, g in zip(r.params, got)}
    return {k: v.detach().numpy() for k, v in outs.items()}, grads


@pytest.mark.parametrize("key", list(mc.UPSTREAMS))
@pytest.mark.parametrize("model,y_dim", mc.MODELS, ids=IDS)
def test_composed_backward_is_autograd_of_the_reference_modules(model, y_dim, key):
    r = mc.reference(model, y_dim, B)
    outs, grads = _autograd(model, y_dim, key)
    for k in mc.OUTPUTS:
        assert np.abs(outs[k] - r.out[k]).max() <= 1e-12 * max(1.0, np.abs(r.out[k]).max()), k
    for k, G in r.truth[key].items():
        assert G.shape == grads[k].shape and np.abs(grads[k] - G).max() <= 1e-12 * max(1.0, np.abs(G).max()), (k, np.abs(grads[k] - G).max())
    if "r" not in mc.UPSTREAMS[key]:                     # nothing reaches the decoder: g_z enters below it, g_mu and g_lv below z
        for k, G in r.truth[key].items():
            assert k.startswith("encoder.") or not G.any(), k
        assert grads["encoder.hidden.0.weight"].any() and grads["encoder.hidden.1.bias"].any()


@pytest.mark.parametrize("model,y_dim", mc.MODELS, ids=IDS)
def test_restatements_stay_inside_their_own_rule(model, y_dim):
    """Trivially true figure by figure; it runs every restatement through check_outputs / check_grads as a device result would be."""
    r = mc.reference(model, y_dim, B)
    assert r.keys == tuple(mc.UPSTREAMS)
    for precision in ("bf16x3", "bf16"):
        for dtype, hook in ((np.float32, None), (np.float32, gc.KStepOrderF32()), (np.float64, gc.POLICIES[precision]())):
            out, grads = r.run(dtype=dtype, hook=hook)
            fails, top, _ = r.check_outputs(out, precision)
            cap = 0.25 + 1e-12 if precision == "bf16x3" else 1.0          # (bf16: some tensors stand under the fixed bar instead)
            assert not fails and top <= cap, (fails, top)
            for key in r.keys:
                fails, top, _ = r.check_grads(grads[key], key, precision, label=key)
                assert not fails and top <= cap, (key, fails, top)
    top = max(f["worst"] for f in r.grad_fig["bf16x3"]["all"].values())
    print(f"bf16x3 restatement, worst column of any gradient: {top:.2e}")


def _ratios(r, key, grads=None, outs=None, precision="bf16x3"):
    """every statistic / its bound, of a faulty result"""
    got = {}
    if grads is not None:
        got.update(r.check_grads(grads, key, precision)[2])
    if outs is not None:
        got.update(r.check_outputs(outs, precision)[2])
    return got


class _LoPlaneDropped(gc.OperandPolicy):
    """bf16x3 with dpre of ONE layer's data gradient (dpre @ W) left at one bf16"""

    def __init__(self, layer):
        super().__init__(2, True)
        self.layer = layer

    def bwd(self, name, dpre, W):
        if name == self.layer:
            return gc.round_bf16(dpre) @ self.op(W)
        return super().bwd(name, dpre, W)


FAULTS = ["bin 512 of g_r ignored", "last frame's da counted twice", "g_mu and g_lv swapped", "g_z dropped",
          "out_r[:, 512] of every frame from the last frame", "lo plane of dpre dropped in decoder layer 2's data gradient"]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("model,y_dim", mc.MODELS, ids=IDS)
def test_a_seeded_fault_exceeds_the_rule_tenfold(model, y_dim, fault):
    """Each fault on the float32 restatement (the last one on the bf16x3 restatement, whose operand it is): at least one statistic of the
    result is 10 x over the bound that a device result is held to."""
    r = mc.reference(model, y_dim, B)
    g_r, g_z, g_mu, g_lv = mc.select(r.up, "all")
    f32run = lambda ups, **kw: mc.run(r.model, r.params, kw.get("x", r.x), kw.get("y", r.y), kw.get("e", r.e), {"all": ups}, np.float32)
    outs = None
    if fault == FAULTS[0]:
        g = g_r.copy()
        g[:, mc.XD - 1] = 0
        grads = f32run((g, g_z, g_mu, g_lv))[1]["all"]
    elif fault == FAULTS[1]:                             # a padding frame (the kernel reads it as frame B - 1) treated as live in da
        again = lambda a: None if a is None else np.concatenate([a, a[-1:]])
        quiet = lambda a: np.concatenate([a, np.zeros_like(a[-1:])])
        grads = f32run((again(g_r), quiet(g_z), quiet(g_mu), quiet(g_lv)), x=again(r.x), y=again(r.y), e=again(r.e))[1]["all"]
    elif fault == FAULTS[2]:
        grads = f32run((g_r, g_z, g_lv, g_mu))[1]["all"]
    elif fault == FAULTS[3]:
        grads = f32run((g_r, None, g_mu, g_lv))[1]["all"]
    elif fault == FAULTS[4]:
        outs, grads = f32run((g_r, g_z, g_mu, g_lv))
        grads = None
        outs["r"] = outs["r"].copy()
        outs["r"][:, mc.XD - 1] = outs["r"][-1, mc.XD - 1]
    else:
        grads = r.run(hook=_LoPlaneDropped("decoder.hidden.1"), keys=("all",))[1]["all"]
    ratios = _ratios(r, "all", grads, outs)
    worst = max(ratios, key=ratios.get)
    print(f"{fault}: {ratios[worst]:.1f} x the bound on {worst}")
    assert ratios[worst] >= 10.0, ratios
    if fault == FAULTS[0]:                               # seen by the per-row figures of the reconstruction layer, at row 512
        assert ratios[mc.REC_B + " rows"] >= 10.0 and ratios[mc.REC_W + " rows"] >= 10.0
    if fault == FAULTS[4]:
        assert set(ratios) == set(mc.OUTPUTS) and all(v <= 0.25 + 1e-12 for k, v in ratios.items() if k != "r")


def test_the_elementwise_hook_at_its_default_changes_no_bit():
    """No hook (the default) and a hook that calls np.tanh / np.exp: the same bits in every output and gradient, in both dtypes; the
    policies' forms differ from them, by float32 roundings only."""
    from oracle import vae_oracle as vo

    class Plain:
        tanh, exp = staticmethod(np.tanh), staticmethod(np.exp)

    r = mc.reference("M2", 1, B)
    assert vo._ELEMENTWISE_HOOK is None
    for dtype in (np.float32, np.float64):
        o0, g0 = r.run(dtype=dtype, keys=("all",))
        o1, g1 = r.run(dtype=dtype, keys=("all",), elementwise=Plain)
        assert vo._ELEMENTWISE_HOOK is None
        assert all(np.array_equal(o0[k], o1[k]) for k in o0) and all(np.array_equal(g0["all"][k], g1["all"][k]) for k in g0["all"])
    o2, _ = r.run(dtype=np.float32, keys=("all",), elementwise=mc.PolicyElementwiseF32)
    d = np.abs(o2["mu"] - o0["mu"]).max()
    assert 0 < d <= 1e-5 * np.abs(o0["mu"]).max()
    v = np.linspace(-12, 12, 4001, dtype=np.float32)
    assert np.abs(mc.PolicyElementwiseF32.tanh(v) - np.tanh(v.astype(np.float64))).max() <= 4 * 2.0 ** -24
    assert np.abs(mc.PolicyElementwiseF32.exp(v) / np.exp(v.astype(np.float64)) - 1).max() <= (2 + 2 * 12) * 2.0 ** -24      # result, product and the float32 log2 e


def test_a_zero_gradient_must_be_exactly_zero():
    r = mc.reference("M2", 1, B)
    g = {k: v.copy() for k, v in r.truth["mu"].items()}
    assert not r.check_grads(g, "mu", "bf16x3")[0]
    g["decoder.hidden.0.bias"][3] = 1e-30
    fails = r.check_grads(g, "mu", "bf16x3")[0]
    assert [k for k, _ in fails] == ["decoder.hidden.0.bias"] and "identically zero" in fails[0][1]

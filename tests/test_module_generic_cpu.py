"""tests/module_generic_cases.py on the CPU, and the host logic of the generic module engine's switch (disentangled-vae_amd/module_path.py):
the composed backward for any z_dim against torch.float64 autograd of the drop-in modules, the restatements inside their own rule,
seeded faults -- what the generic rows kernel's module modes could get wrong -- each at least 10 x over the bound in one statistic,
the frame slices against the library's plans, and engine_kind / set_generic / the default without a device."""
import importlib

import numpy as np
import pytest
import torch

import module_generic_cases as mg
import train_generic_cases as gc
from impl_modules import build_model

mp = importlib.import_module("disentangled-vae_amd.module_path")
TG = importlib.import_module("disentangled-vae_amd.trainer_generic")

B = mg.FULL_CROSS_AT
TWO = [mg.EDGE_CASE, (0, 32, (256, 64))]
IDS = [gc.case_id(c) for c in TWO]


def _module(case, dtype=torch.float32):
    m = build_model(gc.model_of(case), gc.dims_of(case))
    return m.double() if dtype == torch.float64 else m


def _autograd(case, key):
    """(outputs, gradients) of the drop-in module in torch.float64 on the CPU for the loss sum(r g_r) + sum(z g_z) + sum(mu g_mu) +
    sum(lv g_lv) over the upstream gradients of `key`."""
    from packages.models import models as M
    r = mg.reference(case, B)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
    m = _module(case, torch.float64)
    m.load_state_dict({k: t(v) for k, v in r.params.items()})
    x, y, e = t(r.x), t(r.y), t(r.e)
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        if gc.model_of(case) == "M1":
            z, mu, lv = m.encoder(x)
            rec = m.decoder(z)
        else:
            z, mu, lv = M._encode_xy(m.encoder, x, y)
            rec = M._decode_zy(m.decoder, z, y)
    finally:
        M.Stochastic.epsilon_fn = None
    outs = dict(r=rec, z=z, mu=mu, lv=lv)
    loss = sum((outs[k] * t(r.up[k])).sum() for k in mg.UPSTREAMS[key])
    named = dict(m.named_parameters())
    got = torch.autograd.grad(loss, [named[k] for k in r.params], allow_unused=True)
    grads = {k: np.zeros(r.params[k].shape) if g is None else g.numpy() for k, g in zip(r.params, got)}
    return {k: v.detach().numpy() for k, v in outs.items()}, grads


@pytest.mark.parametrize("key", list(mg.UPSTREAMS))
@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_composed_backward_is_autograd_of_the_drop_in_modules(case, key):
    r = mg.reference(case, B)
    assert r.keys == tuple(mg.UPSTREAMS) and r.up["z"].shape == (B, case[1])
    outs, grads = _autograd(case, key)
    for k in ("r", "mu", "lv", "z"):
        assert np.abs(outs[k] - r.out[k]).max() <= 1e-12 * max(1.0, np.abs(r.out[k]).max()), k
    for k, G in r.truth[key].items():
        assert G.shape == grads[k].shape and np.abs(grads[k] - G).max() <= 1e-12 * max(1.0, np.abs(G).max()), (k, np.abs(grads[k] - G).max())
    if "r" not in mg.UPSTREAMS[key]:                     # nothing reaches the decoder
        for k, G in r.truth[key].items():
            assert k.startswith("encoder.") or not G.any(), k


@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_restatements_stay_inside_their_own_rule(case):
    r = mg.reference(case, B)
    for dtype, hook in ((np.float32, None), (np.float32, mg.gg.StepOrderF32(r.slice_frames, case[1]))):
        out, grads = r.run(dtype, hook)
        fails, top, _ = r.check_outputs(out)
        assert not fails and top <= 0.25 + 1e-12, (fails, top)
        for key in r.keys:
            fails, top, _ = r.check_grads(grads[key], key, label=key)
            assert not fails and top <= 0.25 + 1e-12, (key, fails, top)


def _g_z_not_added(p, enc, dec, z, g_r, g_z, g_mu, g_lv):
    return mg.backward(p, enc, dec, z, g_r, None, g_mu, g_lv)


def _latent_width_16(p, enc, dec, z, g_r, g_z, g_mu, g_lv):
    """the resident path's dd[:, :16] on another z: the columns past 16 (or the label columns below 16) are wrong"""
    w = min(16, z)
    pad = lambda a: None if a is None else np.concatenate([a[:, :w], np.zeros_like(a[:, w:])], axis=1)
    grads = {}
    da = g_r * dec["r"]
    dd = mg.vo.decoder_bwd(p, grads, "decoder.", dec, da)
    dz = pad(dd[:, :z]) + g_z
    mg.vo.encoder_bwd(p, grads, "encoder.", enc, dz, g_mu, g_lv)
    return grads


FAULTS = ["one column of g_r dropped", "g_z not added", "bin 512 of g_r ignored", "g_mu and g_lv swapped", "a frame past B counted in da",
          "dz cut at 16 latent columns", "out_r[:, 512] of every frame from the last frame", "1 / B applied to the upstream gradients"]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_a_seeded_fault_exceeds_the_rule_tenfold(case, fault):
    """Each fault on the float32 restatement: at least one statistic of the result is 10 x over the bound a device result is held to."""
    r = mg.reference(case, B)
    g_r, g_z, g_mu, g_lv = mg.select(r.up, "all")
    f32run = lambda ups, back=mg.backward, **kw: mg.run(case, r.params, kw.get("x", r.x), kw.get("y", r.y), kw.get("e", r.e), {"all": ups},
                                                        np.float32, None, back)
    outs, grads = None, None
    if fault == FAULTS[0]:
        g = g_r.copy()
        g[:, 257] = 0
        grads = f32run((g, g_z, g_mu, g_lv))[1]["all"]
    elif fault == FAULTS[1]:
        grads = f32run((g_r, g_z, g_mu, g_lv), _g_z_not_added)[1]["all"]
    elif fault == FAULTS[2]:
        g = g_r.copy()
        g[:, mg.XD - 1] = 0
        grads = f32run((g, g_z, g_mu, g_lv))[1]["all"]
    elif fault == FAULTS[3]:
        grads = f32run((g_r, g_z, g_lv, g_mu))[1]["all"]
    elif fault == FAULTS[4]:
        again = lambda a: None if a is None else np.concatenate([a, a[-1:]])
        quiet = lambda a: np.concatenate([a, np.zeros_like(a[-1:])])
        grads = f32run((again(g_r), quiet(g_z), quiet(g_mu), quiet(g_lv)), x=again(r.x), y=again(r.y), e=again(r.e))[1]["all"]
    elif fault == FAULTS[5]:
        assert case[1] > 16
        grads = f32run((g_r, g_z, g_mu, g_lv), _latent_width_16)[1]["all"]
    elif fault == FAULTS[6]:
        outs = f32run((g_r, g_z, g_mu, g_lv))[0]
        outs["r"] = outs["r"].copy()
        outs["r"][:, mg.XD - 1] = outs["r"][-1, mg.XD - 1]
    else:
        s = np.float32(1.0 / B)
        grads = f32run((g_r * s, g_z * s, g_mu * s, g_lv * s))[1]["all"]
    ratios = {}
    if grads is not None:
        ratios.update(r.check_grads(grads, "all")[2])
    if outs is not None:
        ratios.update(r.check_outputs(outs)[2])
    worst = max(ratios, key=ratios.get)
    print(f"{fault}: {ratios[worst]:.1f} x the bound on {worst}")
    assert ratios[worst] >= 10.0, ratios
    if fault in (FAULTS[0], FAULTS[2]):                  # seen by the per-row figures of the reconstruction layer, at that row
        assert ratios[mg.mc.REC_B + " rows"] >= 10.0 and ratios[mg.mc.REC_W + " rows"] >= 10.0


def test_slice_plan_restates_the_librarys_plans():
    for case in mg.GEOMETRIES:
        for Bn in (1, 17, 50, 127, 128, 500, 4149, 8192):
            p = TG.make_plan(gc.model_of(case), gc.dims_of(case), Bn)
            assert mg.slice_plan(case, Bn) == (p.slice_frames, p.ksplit), (case, Bn)
    Bn, p = gc.loops_batch(lambda b: TG.make_plan(gc.model_of(mg.LOOPS_CASE), gc.dims_of(mg.LOOPS_CASE), b))
    assert -(-Bn // 16) > p.rows_grid == mg.ROWS_GRID and mg.slice_plan(mg.LOOPS_CASE, Bn)[1] >= 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch (host logic: no device)
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def clean_env(monkeypatch):
    for k in ("DVAE_MODULE_PATH", "DVAE_MODULE_GENERIC"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _m(model, y, z, h):
    from packages.models import models as M
    if model == "M1":
        return M.VariationalAutoencoder([513, z, list(h)])
    if model == "M2":
        return M.DeepGenerativeModel([513, y, z, list(h)], None)
    return M.DeepGenerativeModel_v3([513, y, z, list(h)])


def test_default_leaves_a_non_reference_module_on_the_layer_path(clean_env):
    m = _m("M2", 1, 32, (256, 64))
    assert mp.generic_mode(m) == "off" and mp.engine_kind(m, "M2") is None
    assert mp.engine_kind(_m("M2", 1, 16, (128, 128)), "M2") == "resident"
    assert mp.engine_kind(_m("M1", 0, 16, (128, 128)), "M1") == "resident"
    clean_env.setenv("DVAE_MODULE_GENERIC", "0")
    assert mp.engine_kind(m, "M2") is None


def test_engine_kind_for_covered_resident_and_refused_dims(clean_env):
    clean_env.setenv("DVAE_MODULE_GENERIC", "1")
    for case in mg.GEOMETRIES:
        y, z, h = case
        model = gc.model_of(case)
        want = "resident" if mg.forced(case) else "generic"
        assert mp.engine_kind(_m(model, y, z, h), model) == want, case
        assert mp.generic_dims(_m(model, y, z, h), model) == gc.dims_of(case)
    # outside trainer_generic.covered: z 129, a width of 513, three hidden layers, another x_dim, the M2_info body, a flow
    assert mp.engine_kind(_m("M1", 0, 129, (128, 128)), "M1") is None
    assert mp.engine_kind(_m("M2", 1, 16, (513, 128)), "M2") is None
    assert mp.engine_kind(_m("M1", 0, 16, (128, 128, 128)), "M1") is None
    from packages.models import models as M
    assert mp.engine_kind(M.VariationalAutoencoder([512, 16, [128, 128]]), "M1") is None
    assert mp.engine_kind(_m("M2_DEC", 1, 32, (256, 64)), "M2_DEC") is None
    assert mp.engine_kind(_m("M2_DEC", 1, 16, (128, 128)), "M2_DEC") == "resident"
    flowed = _m("M1", 0, 32, (256, 64))
    flowed.add_flow(torch.nn.Identity())
    assert mp.engine_kind(flowed, "M1") is None
    # force: the reference geometry through the generic engine; the M2_info body has none and stays resident
    clean_env.setenv("DVAE_MODULE_GENERIC", "force")
    assert mp.engine_kind(_m("M2", 1, 16, (128, 128)), "M2") == "generic"
    assert mp.engine_kind(_m("M2_DEC", 1, 16, (128, 128)), "M2_DEC") == "resident"
    # DVAE_MODULE_PATH=layers wins
    clean_env.setenv("DVAE_MODULE_PATH", "layers")
    assert mp.engine_kind(_m("M2", 1, 32, (256, 64)), "M2") is None and mp.engine_kind(_m("M2", 1, 16, (128, 128)), "M2") is None


def test_set_generic_overrides_the_environment_per_module(clean_env):
    a, b = _m("M2", 1, 32, (256, 64)), _m("M2", 1, 32, (256, 64))
    mp.set_generic(a, "on")
    assert mp.engine_kind(a, "M2") == "generic" and mp.engine_kind(b, "M2") is None
    clean_env.setenv("DVAE_MODULE_GENERIC", "1")
    mp.set_generic(a, 0)
    assert mp.engine_kind(a, "M2") is None and mp.engine_kind(b, "M2") == "generic"
    mp.set_generic(a, None)
    assert mp.engine_kind(a, "M2") == "generic"
    ref = _m("M1", 0, 16, (128, 128))
    mp.set_generic(ref, "force")
    assert mp.engine_kind(ref, "M1") == "generic"
    with pytest.raises(ValueError, match="set_generic"):
        mp.set_generic(a, "sometimes")
    clean_env.setenv("DVAE_MODULE_GENERIC", "maybe")
    with pytest.raises(ValueError, match="DVAE_MODULE_GENERIC"):
        mp.engine_kind(b, "M2")
    import copy
    assert copy.deepcopy(a).__dict__.get("_dvae_engine") is None


def test_c_abi_refuses_by_name_before_a_device_is_needed():
    """ld_r / ld_gr below 513, a std_norm plan, overlapping rows of x: DVAE_E_BADARG with the argument named (host checks: they come before
    anything is launched, so they answer without a GPU)."""
    import ctypes
    native = importlib.import_module("disentangled-vae_amd.native")
    lib = native.load()
    dims = gc.dims_of((1, 5, (48, 200)))
    plan = TG.make_plan("M2", dims, 17)
    one = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused on the host
    p = ctypes.byref(plan)
    stream = ctypes.c_void_p(0)

    def refused(rc, word):
        msg = lib.dvae_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
    refused(lib.dvae_module_generic_forward(p, one, one, one, 513, one, 1, one, one, 512, one, one, None, 1, stream), "ld_r")
    refused(lib.dvae_module_generic_backward(p, one, one, one, 513, one, 1, one, one, 512, None, None, None, one, 0, stream), "ld_gr")
    refused(lib.dvae_module_generic_forward(p, one, one, one, 512, one, 1, one, one, 513, one, one, None, 1, stream), "leading dimension of x")
    refused(lib.dvae_module_generic_backward(p, one, one, one, 513, one, 0, one, one, 513, None, None, None, one, 0, stream), "leading dimension of y")
    refused(lib.dvae_module_generic_backward(p, one, one, one, 513, one, 1, one, one, 513, None, None, None, one, 2, stream), "accumulate")
    normed = TG.make_plan("M2", dims, 17, std_norm=True)
    refused(lib.dvae_module_generic_forward(ctypes.byref(normed), one, one, one, 513, one, 1, one, one, 513, one, one, None, 1, stream), "std_norm")
    refused(lib.dvae_module_generic_backward(ctypes.byref(normed), one, one, one, 513, one, 1, one, one, 513, None, None, None, one, 0, stream), "std_norm")

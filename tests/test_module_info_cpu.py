"""tests/module_info_cases.py on the CPU, and the host logic of the M2_info body on the generic module engine
(disentangled-vae_amd/module_path.py; include/dvae_train.h: dvae_module_generic_plan, dvae_module_generic_backward_y): the truth, the label
gradient included, against torch.float64 autograd of the drop-in DeepGenerativeModel_v3 with y.requires_grad_(); seeded faults -- what the
DEC variant of the rows kernel could get wrong -- each at least 10 x over the bound in one statistic; the library's M2_DEC plans against the
restated slice_plan, against the M2 plans of the same dims and against dvae_train_generic_plan; the refusals by name without a device; and
engine_kind / set_info_body under every combination of the two switches."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest
import torch

import module_info_cases as mi
import train_generic_cases as gc

mp = importlib.import_module("disentangled-vae_amd.module_path")
TG = importlib.import_module("disentangled-vae_amd.trainer_generic")
native = importlib.import_module("disentangled-vae_amd.native")
MODEL_CODE = importlib.import_module("disentangled-vae_amd.trainer").MODEL_CODE

B = mi.FULL_CROSS_AT
TWO = [mi.EDGE_CASE, (513, 16, (128, 128))]
IDS = [gc.case_id(c) for c in TWO]


def _v3(y, z, h, dtype=torch.float32):
    from packages.models import models as M
    m = M.DeepGenerativeModel_v3([513, y, z, list(h)])
    return m.double() if dtype == torch.float64 else m


def _v5(y, z, h):
    from packages.models import models as M
    return M.DeepGenerativeModel_v5([513, y, z, list(h)])


def _autograd(case, key):
    """(outputs, the 14 gradients and g_y) of the drop-in _v3 in torch.float64 on the CPU for the loss sum(r g_r) + sum(z g_z) + sum(mu g_mu) +
    sum(lv g_lv) over the upstream gradients of `key`, the label input a leaf that requires a gradient."""
    from packages.models import models as M
    r = mi.reference(case, B)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    m = _v3(*case, dtype=torch.float64)
    missing = m.load_state_dict({k: t(v) for k, v in r.params.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("classifier.") for k in missing.missing_keys)
    x, y, e = t(r.x), t(r.y).requires_grad_(), t(r.e)
    M.Stochastic.epsilon_fn = lambda mu: e
    try:
        rec, z, mu, lv = m._forward_z(x, y)
    finally:
        M.Stochastic.epsilon_fn = None
    outs = dict(r=rec, z=z, mu=mu, lv=lv)
    loss = sum((outs[k] * t(r.up[k])).sum() for k in mi.UPSTREAMS[key])
    named = dict(m.named_parameters())
    got = torch.autograd.grad(loss, [named[k] for k in r.params] + [y], allow_unused=True)
    names = list(r.params) + [mi.GY]
    shapes = [r.params[k].shape for k in r.params] + [r.y.shape]
    grads = {k: np.zeros(s) if g is None else g.numpy() for k, g, s in zip(names, got, shapes)}
    return {k: v.detach().numpy() for k, v in outs.items()}, grads


@pytest.mark.parametrize("key", list(mi.UPSTREAMS))
@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_truth_with_the_label_gradient_is_autograd_of_the_drop_in_v3(case, key):
    r = mi.reference(case, B)
    assert r.keys == tuple(mi.UPSTREAMS) and r.truth[key][mi.GY].shape == (B, case[0])
    assert r.params["encoder.hidden.0.weight"].shape == (case[2][0], 513) and r.params["decoder.hidden.0.weight"].shape == (case[2][1], case[1] + case[0])
    outs, grads = _autograd(case, key)
    for k in ("r", "mu", "lv", "z"):
        assert np.abs(outs[k] - r.out[k]).max() <= 1e-12 * max(1.0, np.abs(r.out[k]).max()), k
    assert set(grads) == set(r.truth[key])
    for k, G in r.truth[key].items():
        assert G.shape == grads[k].shape and np.abs(grads[k] - G).max() <= 1e-12 * max(1.0, np.abs(G).max()), (k, np.abs(grads[k] - G).max())
    if "r" not in mi.UPSTREAMS[key]:                     # nothing reaches the decoder, and so nothing reaches y
        assert not r.truth[key][mi.GY].any()
    else:
        assert r.truth[key][mi.GY].any()


@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_restatements_stay_inside_their_own_rule(case):
    r = mi.reference(case, B)
    for dtype, hook in ((np.float32, None), (np.float32, mi.gg.StepOrderF32(r.slice_frames, case[1]))):
        out, grads = r.run(dtype, hook)
        fails, top, _ = r.check_outputs(out)
        assert not fails and top <= 0.25 + 1e-12, (fails, top)
        for key in r.keys:
            fails, top, ratios = r.check_grads(grads[key], key, label=key)
            assert not fails and top <= 0.25 + 1e-12, (key, fails, top)
            assert mi.GY in ratios and mi.GY_TENSOR in ratios
            without = {k: v for k, v in grads[key].items() if k != mi.GY}
            assert mi.GY not in r.check_grads(without, key)[2]


def _no_g_y(p, enc, dec, z, *ups):
    g = mi.backward(p, enc, dec, z, *ups)
    g[mi.GY] = np.zeros_like(g[mi.GY])
    return g


def _label_column_shifted(p, enc, dec, z, *ups):
    """label column c stored where c + 1 belongs (the last one wraps to the first)"""
    g = mi.backward(p, enc, dec, z, *ups)
    g[mi.GY] = np.roll(g[mi.GY], 1, axis=1)
    return g


def _encoder_given_y(p, x, y, e):
    """encoder layer 1 on [x | y], as in M2: the label block of its product not left out (weights of the scale of the layer's own)"""
    W = p["encoder.hidden.0.weight"]
    rng = np.random.default_rng(5)
    Wy = (rng.standard_normal((W.shape[0], y.shape[1])) * np.sqrt(2.0 / (W.shape[0] + W.shape[1]))).astype(W.dtype)
    q = dict(p, **{"encoder.hidden.0.weight": np.concatenate([W, Wy], axis=1)})
    enc = mi.vo.encoder_fwd(q, "encoder.", np.concatenate([x, y], axis=1), e)
    enc["inp"] = x                                       # the backward of the true composition: the weight gradient keeps its 513 columns
    dec = mi.vo.decoder_fwd(p, "decoder.", np.concatenate([enc["z"], y], axis=1))
    return enc, dec


FAULTS = ["the g_y term dropped", "the encoder given y", "one label column shifted"]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("case", TWO, ids=IDS)
def test_a_seeded_fault_exceeds_the_rule_tenfold(case, fault):
    """Each fault on the float32 restatement: at least one statistic of the result is 10 x over the bound a device result is held to."""
    r = mi.reference(case, B)
    ups = {"all": mi.mg.select(r.up, "all")}
    f32run = lambda **kw: mi.run(case, r.params, r.x, r.y, r.e, ups, np.float32, None, **kw)
    if fault == FAULTS[0]:
        out, grads = f32run(back=_no_g_y)
    elif fault == FAULTS[1]:
        out, grads = f32run(fwd=_encoder_given_y)
    else:
        out, grads = f32run(back=_label_column_shifted)
    ratios = dict(r.check_grads(grads["all"], "all")[2])
    ratios.update(r.check_outputs(out)[2])
    worst = max(ratios, key=ratios.get)
    print(f"{fault}: {ratios[worst]:.1f} x the bound on {worst}")
    assert ratios[worst] >= 10.0, ratios
    if fault in (FAULTS[0], FAULTS[2]):                  # seen by the label gradient's own figures, and by nothing else
        assert ratios[mi.GY] >= 10.0 and ratios[mi.GY_TENSOR] >= 10.0
        assert max(v for k, v in ratios.items() if k not in (mi.GY, mi.GY_TENSOR)) <= 0.25 + 1e-12
    else:                                                # the encoder's outputs move
        assert ratios["mu"] >= 10.0 and ratios["z"] >= 10.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the plans (host only)
# ---------------------------------------------------------------------------------------------------------------------------------

def _plan(model, case, Bn, ksplit=0):
    y, z, (h1, h2) = case
    plan = TG.GenericPlan()
    rc = native.load().dvae_module_generic_plan(MODEL_CODE[model], 0 if model == "M1" else y, z, h1, h2, Bn, ksplit, ctypes.byref(plan))
    return rc, plan


def _bytes(plan):
    return bytes(memoryview(plan).cast("B"))


def test_slice_plan_restates_the_librarys_m2_dec_plans():
    for case in mi.GEOMETRIES:
        for Bn in (1, 17, 50, 127, 128, 500, 4149, 8192):
            rc, p = _plan("M2_DEC", case, Bn)
            assert rc == 0 and mi.slice_plan(case, Bn) == (p.slice_frames, p.ksplit), (case, Bn)
    Bn, p = gc.loops_batch(lambda b: _plan("M2_DEC", mi.LOOPS_CASE, b)[1])
    assert -(-Bn // 16) > p.rows_grid == mi.mg.ROWS_GRID and mi.slice_plan(mi.LOOPS_CASE, Bn)[1] >= 2


def test_m1_and_m2_plans_of_the_new_entry_point_are_the_train_plans_byte_for_byte():
    for case in [(0, 32, (256, 64)), (0, 1, (1, 1))] + mi.GEOMETRIES:
        for Bn, ks in ((1, 0), (50, 0), (8192, 0), (500, 3)):
            model = gc.model_of(case)
            rc, p = _plan(model, case, Bn, ks)
            want = TG.make_plan(model, gc.dims_of(case), Bn, ksplit=ks)
            assert rc == 0 and _bytes(p) == _bytes(want), (case, Bn, ks)


def test_m2_dec_plan_differs_from_the_m2_plan_exactly_as_documented():
    al64 = lambda v: -(-v // 64) * 64
    up16 = lambda v: -(-v // 16) * 16
    for case in mi.GEOMETRIES:
        y, z, (h1, h2) = case
        for Bn in (17, 50, 8192):
            rc, d = _plan("M2_DEC", case, Bn, 2)
            m = TG.make_plan("M2", gc.dims_of(case), Bn, ksplit=2)
            assert rc == 0 and d.model == MODEL_CODE["M2_DEC"] and m.model == MODEL_CODE["M2"]
            for f in ("y_dim", "z_dim", "h1", "h2", "precision", "n_tensors", "B", "Bp", "rows_grid", "lds_bytes", "std_norm", "ksplit", "slice_frames"):
                assert getattr(d, f) == getattr(m, f), (case, Bn, f)
            rows = [d.tensor_rows[t] for t in range(14)]
            cols = [d.tensor_cols[t] for t in range(14)]
            assert rows == [m.tensor_rows[t] for t in range(14)]
            assert cols[0] == 513 and m.tensor_cols[0] == 513 + y and cols[8] == z + y == m.tensor_cols[8]
            assert cols[1:] == [m.tensor_cols[t] for t in range(1, 14)]
            # tensor 0 lost its label columns: every later tensor moves down by the same (256-byte aligned) amount
            shift = al64(h1 * (513 + y)) - al64(h1 * 513)
            assert d.tensor_offset[0] == m.tensor_offset[0] == 0
            assert all(m.tensor_offset[t] - d.tensor_offset[t] == shift for t in range(1, 14)) and m.n_params - d.n_params == shift
            # the workspace: W1y ([h1p][yp]) is empty, D1yT ([yp][h2p]) is appended behind the last packed copy; the stash is the same; the
            # slabs hold n_params floats each.  The item table differs where matrix 0 lost its label blocks (not compared byte for byte)
            packed = 4 * (al64(up16(y) * up16(h2)) - al64(up16(h1) * up16(y)))
            al256 = lambda v: -(-v // 256) * 256
            items = al256(16 * d.wgrad_items) - al256(16 * m.wgrad_items)
            assert d.grad_offset_bytes - m.grad_offset_bytes == packed + items, (case, Bn)
            assert (d.workspace_bytes - d.grad_offset_bytes) - (m.workspace_bytes - m.grad_offset_bytes) == al256(d.ksplit * d.n_params * 4) - al256(m.ksplit * m.n_params * 4)
            assert d.wgrad_items <= m.wgrad_items


def test_plan_refusals_name_the_limits():
    lib = native.load()
    for case, word in (((0, 16, (128, 128)), "y_dim 1..513"), ((514, 16, (128, 128)), "y_dim 1..513"), ((1, 129, (128, 128)), "z_dim 1..128"),
                       ((1, 16, (513, 128)), "hidden widths 1..512"), ((1, 16, (128, 0)), "hidden widths 1..512")):
        rc, _ = _plan("M2_DEC", case, 50)
        msg = lib.dvae_last_error().decode()
        assert rc == 1001 and "M2_DEC" in msg and word in msg, (case, rc, msg)
    assert _plan("M2_DEC", mi.EDGE_CASE, 0)[0] == 1001 and "frames" in lib.dvae_last_error().decode()
    assert _plan("M2_DEC", mi.EDGE_CASE, 50, 17)[0] == 1001 and "frame slices" in lib.dvae_last_error().decode()
    rc, _ = _plan("M2_info", mi.EDGE_CASE, 50)
    assert rc == 1003 and "M2_info" in lib.dvae_last_error().decode()
    # the two pinned refusals of the train planner stand
    with pytest.raises(NotImplementedError, match="reference geometry only"):
        TG.make_plan("M2_DEC", gc.dims_of(mi.EDGE_CASE), 50)
    # a plan whose precision field was changed to a 16-bit policy is no plan of the library's
    rc, p = _plan("M2_DEC", mi.EDGE_CASE, 17)
    p.precision = 2
    one, stream = ctypes.c_void_p(256), ctypes.c_void_p(0)
    assert lib.dvae_train_generic_init(ctypes.byref(p), one, one, stream) == 1001 and "not a plan" in lib.dvae_last_error().decode()


def test_c_abi_refuses_by_name_before_a_device_is_needed():
    """Host checks: they come before anything is launched, so they answer without a GPU."""
    lib = native.load()
    rc, plan = _plan("M2_DEC", (3, 5, (48, 200)), 17)
    assert rc == 0
    one = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused on the host
    p, stream = ctypes.byref(plan), ctypes.c_void_p(0)

    def refused(rc, *words):
        msg = lib.dvae_last_error().decode()
        assert rc == 1001 and all(w in msg for w in words), (rc, msg)
    bwd = lambda pl, ld_gr, gy, ld_gy, acc=0, ldy=3: lib.dvae_module_generic_backward_y(pl, one, one, one, 513, one, ldy, one, one, ld_gr, None, None, None,
                                                                                        one, acc, gy, ld_gy, stream)
    refused(bwd(p, 513, one, 2), "ld_gy", "module_generic_backward_y")
    refused(bwd(p, 512, one, 3), "ld_gr")
    refused(bwd(p, 512, None, 0), "ld_gr")
    refused(bwd(p, 513, one, 3, acc=2), "accumulate")
    refused(bwd(p, 513, one, 3, ldy=2), "leading dimension of y")
    m2 = TG.make_plan("M2", gc.dims_of((3, 5, (48, 200))), 17)
    refused(bwd(ctypes.byref(m2), 513, one, 3), "g_y", "M2_DEC")
    m1 = TG.make_plan("M1", gc.dims_of((0, 5, (48, 200))), 17)
    refused(lib.dvae_module_generic_backward_y(ctypes.byref(m1), one, one, one, 513, None, 0, one, one, 513, None, None, None, one, 0, one, 1, stream),
            "g_y", "M2_DEC")
    refused(lib.dvae_module_generic_forward(p, one, one, one, 513, one, 3, one, one, 512, one, one, None, 1, stream), "ld_r")
    refused(lib.dvae_module_generic_forward(p, one, one, one, 513, None, 0, one, one, 513, one, one, None, 1, stream), "y must be given")
    # the train step's entry points refuse the plan, the model named
    f3 = (0.0,) * 5
    for name, rc in (("grads", lib.dvae_train_generic_grads(p, one, one, 513, one, 3, one, 1e-8, stream)),
                     ("step", lib.dvae_train_generic_step(p, one, one, one, one, one, 513, one, 3, one, 1e-8, 1, 1e-3, 0.9, 0.999, 1e-8, one, stream)),
                     ("eval", lib.dvae_train_generic_eval(p, one, one, 513, one, 3, one, 1e-8, one, stream)),
                     ("apply", lib.dvae_train_generic_apply(p, one, one, one, one, 1, *f3, one, stream)),
                     ("reduce", lib.dvae_train_generic_reduce(p, one, one, 0, 1.0, one, stream)),
                     ("apply_flat", lib.dvae_train_generic_apply_flat(p, one, one, one, one, one, 1, *f3, stream)),
                     ("apply_flat_clipped", lib.dvae_train_generic_apply_flat_clipped(p, one, one, one, one, one, 1, *f3, 1.0, one, one, one, stream))):
        msg = lib.dvae_last_error().decode()
        assert rc == 1001 and "M2_DEC" in msg and "train_generic_" in msg, (name, rc, msg)


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch (host logic: no device)
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def clean_env(monkeypatch):
    for k in ("DVAE_MODULE_PATH", "DVAE_MODULE_GENERIC", "DVAE_MODULE_INFO_BODY"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_the_switch_on_sends_an_edited_geometry_to_the_generic_engine(clean_env):
    """fails on the parent: the body of another size had no engine, and the library no dvae_module_generic_plan"""
    clean_env.setenv("DVAE_MODULE_INFO_BODY", "1")
    assert mp.engine_kind(_v3(1, 32, (256, 64)), "M2_DEC") == "generic"
    assert hasattr(native.load(), "dvae_module_generic_plan") and hasattr(native.load(), "dvae_module_generic_backward_y")


def test_engine_kind_under_every_combination_of_the_two_switches(clean_env):
    edited, ibm, ref = _v3(1, 32, (256, 64)), _v3(513, 16, (128, 128)), _v3(1, 16, (128, 128))
    m2 = importlib.import_module("packages.models.models").DeepGenerativeModel([513, 1, 32, [256, 64]], None)
    want = {"off": (None, None, "resident"), "on": ("generic", "generic", "resident"), "force": ("generic", "generic", "generic")}
    settings = {"off": (None, "0", "off"), "on": ("1", "on"), "force": ("force",)}
    for body, generic in itertools.product(("off", "on", "force"), repeat=2):
        for bv, gv in itertools.product(settings[body], settings[generic]):
            for k, v in (("DVAE_MODULE_INFO_BODY", bv), ("DVAE_MODULE_GENERIC", gv)):
                clean_env.delenv(k, raising=False) if v is None else clean_env.setenv(k, v)
            got = tuple(mp.engine_kind(m, "M2_DEC") for m in (edited, ibm, ref))
            assert got == want[body], (bv, gv, got)
            assert mp.info_body_mode(edited) == body and mp.generic_mode(edited) == generic
            # and this switch says nothing about M2
            assert mp.engine_kind(m2, "M2") == (None if generic == "off" else "generic"), (bv, gv)
            clean_env.setenv("DVAE_MODULE_PATH", "layers")
            assert all(mp.engine_kind(m, "M2_DEC") is None for m in (edited, ibm, ref))
            clean_env.delenv("DVAE_MODULE_PATH")


def test_covered_and_refused_dims(clean_env):
    clean_env.setenv("DVAE_MODULE_INFO_BODY", "1")
    for case in mi.GEOMETRIES:
        y, z, h = case
        assert mp.engine_kind(_v3(y, z, h), "M2_DEC") == ("resident" if mi.forced(case) else "generic"), case
        assert mp.generic_dims(_v3(y, z, h), "M2_DEC") == gc.dims_of(case)
    assert mp.engine_kind(_v3(1, 129, (128, 128)), "M2_DEC") is None
    assert mp.engine_kind(_v3(1, 16, (513, 128)), "M2_DEC") is None
    assert mp.engine_kind(_v3(514, 16, (128, 128)), "M2_DEC") is None
    assert mp.engine_kind(_v3(1, 16, (128, 128, 128)), "M2_DEC") is None
    from packages.models import models as M
    assert mp.engine_kind(M.DeepGenerativeModel_v3([512, 1, 16, [128, 128]]), "M2_DEC") is None
    flowed = _v3(1, 32, (256, 64))
    flowed.flow = torch.nn.Identity()
    assert mp.engine_kind(flowed, "M2_DEC") is None
    nobias = _v3(1, 32, (256, 64))
    nobias.decoder.hidden[1].bias = None
    assert mp.engine_kind(nobias, "M2_DEC") is None
    clean_env.setenv("DVAE_MODULE_INFO_BODY", "force")
    assert mp.engine_kind(_v3(1, 16, (128, 128)), "M2_DEC") == "generic"
    assert mp.engine_kind(_v3(1, 129, (128, 128)), "M2_DEC") is None


def test_set_info_body_on_a_v3_and_on_a_v5_and_the_value_errors(clean_env):
    a, b = _v3(1, 32, (256, 64)), _v3(1, 32, (256, 64))
    mp.set_info_body(a, "on")
    assert mp.engine_kind(a, "M2_DEC") == "generic" and mp.engine_kind(b, "M2_DEC") is None
    clean_env.setenv("DVAE_MODULE_INFO_BODY", "1")
    mp.set_info_body(a, 0)
    assert mp.engine_kind(a, "M2_DEC") is None and mp.engine_kind(b, "M2_DEC") == "generic"
    mp.set_info_body(a, None)
    assert mp.engine_kind(a, "M2_DEC") == "generic"
    clean_env.delenv("DVAE_MODULE_INFO_BODY")
    v5 = _v5(513, 16, (128, 128))
    assert mp.engine_kind(v5.enc_dec_clf, "M2_DEC") is None
    mp.set_info_body(v5, "on")
    assert mp.engine_kind(v5.enc_dec_clf, "M2_DEC") == "generic" and "_dvae_info_body" not in v5.__dict__
    mp.set_info_body(v5, None)
    assert mp.engine_kind(v5.enc_dec_clf, "M2_DEC") is None
    ref = _v5(1, 16, (128, 128))
    mp.set_info_body(ref, True)
    assert mp.engine_kind(ref.enc_dec_clf, "M2_DEC") == "resident"
    mp.set_info_body(ref, "force")
    assert mp.engine_kind(ref.enc_dec_clf, "M2_DEC") == "generic"
    with pytest.raises(ValueError, match="set_info_body"):
        mp.set_info_body(a, "sometimes")
    clean_env.setenv("DVAE_MODULE_INFO_BODY", "maybe")
    with pytest.raises(ValueError, match="DVAE_MODULE_INFO_BODY"):
        mp.engine_kind(b, "M2_DEC")
    import copy
    assert copy.deepcopy(a).__dict__.get("_dvae_engine") is None

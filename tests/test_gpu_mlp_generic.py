"""The generic encoder / classifier kernel on the MI355X (csrc/mlp_generic.hip: dvae_encode_generic_batch, dvae_classify_generic_batch;
the packs of encode.py / classify.py made with generic=True, pack_encoder / pack_classifier): every geometry case of
tests/mlp_generic_cases.py within the bars of tests/encode_ref.py / tests/classify_ref.py, bit identity over sources, tile edges (16-frame
tiles), batches and runs with untouched rows and columns, the reference's geometry on both kernels, the column output and the fused
MCEM start with an encoder pack, reconstruct_batch with an encoder pack, a generic classifier's labels into MCEM and f1_batch, refusals
through the C ABI, and the enhancement example at --z-dim 32 --h-dim 256 64 with --fused-start and --labels classifier.

Bars: mu and log_var within 8 c u M of the float64 network, z within the z bar of encode_ref.bars; logits within 8 c u M, soft within
bar / 4 + 4 u, hard equal outside |logit64| <= 2 bar + 4 u with at most 0.1 % of a case excluded.  c = max(c_ref, C_FLOOR): c_ref per
head / logit measured on the reference's own float32 CPU run and recorded in the fixture, C_FLOOR the smallest c_ref of the committed
encode / classify fixtures (mlp_generic_cases.py).  Every test prints its worst error in units of the bars before it asserts.

Measured on an MI355X (worst error in bars over complex frames, power rows, power rows at a leading dimension of 520 and both label
strides), mu / log_var / z per encoder case (y_dim, z, (h1, h2)):
  (0, 32, (256, 64))      0.133 / 0.092 / 0.083        (1, 32, (256, 64))      0.114 / 0.100 / 0.098
  (1, 5, (48, 200))       0.125 / 0.093 / 0.113        (513, 64, (16, 16))     0.152 / 0.150 / 0.125
  (0, 1, (1, 1))          0.194 / 0.129 / 0.147        (3, 17, (129, 127))     0.122 / 0.188 / 0.099
  (513, 128, (512, 512))  0.139 / 0.154 / 0.112        (1, 16, (128, 128))     0.121 / 0.105 / 0.088
logit / soft per classifier case ((h1, h2), y_dim), no hard label off outside the margin, excluded share at most 1.7e-5:
  ((256, 64), 1)    0.126 / 0.186      ((48, 200), 2)     0.187 / 0.194      ((129, 127), 17)   0.152 / 0.210
  ((1, 1), 1)       0.357 / 0.140      ((512, 512), 513)  0.218 / 0.201      ((128, 128), 513)  0.136 / 0.205
The reference's geometry on the committed fixtures: the generic and the resident kernel gave the same figures (encoders 0.118 / 0.165 /
0.091, 0.184 / 0.164 / 0.172, 0.104 / 0.088 / 0.092; classifiers 0.144 / 0.162 and 0.136 / 0.201).  The fused start's Z on the z 32
models: 0.114 (M2) and 0.133 (M1) bars from float64, bit-equal to the default start's; reconstruct_batch's variance at 0.008 of the
decoder bound.
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_ref as CR
import encode_ref as ER
import mlp_generic_cases as MC
from test_classify_cpu import GOLD as CLF_GOLD, rebuild as rebuild_resident_classifier
from test_encode_cpu import GOLD as ENC_GOLD, labels_of as resident_labels_of, rebuild as rebuild_resident_encoder
from test_gpu_encode import _decode_bound, _decoder64, bits, dev, leave_the_allocator_as_found, spec_of, wide      # noqa: F401 (the fixture is used by name)
from test_mlp_generic_cpu import FRAMES, GOLD, labels_of, rebuild_classifier, rebuild_encoder

pytestmark = pytest.mark.gpu
E = importlib.import_module("disentangled-vae_amd.encode")
C = importlib.import_module("disentangled-vae_amd.classify")
M = importlib.import_module("disentangled-vae_amd.mcem")
N = importlib.import_module("disentangled-vae_amd.native")
from packages.models import models as PM
from packages.models.utils import f1_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
COUNTS = MC.COUNTS
EDGES = [1, 15, 16, 17, 31, 33]
NAN = float("nan")
BADARG = 1001

_enc, _clf = {}, {}


def frozen(module):
    module = module.to(DEV).eval()
    for p in module.parameters():
        p.requires_grad = False
    return module


def enc_case(case):
    """(generic pack, model on the device, encoder weights, [x | y] float32, c mu, c log_var) of an encoder case, made once."""
    if case not in _enc:
        model, w = rebuild_encoder(case)
        model = frozen(model)
        c_mu, c_lv = (MC.c_eff(c) for c in GOLD[MC.enc_id(case) + "/c_ref"])
        pack = E.EncoderPack(model.encoder, case[0], generic=True)
        assert pack.generic and (pack.y_dim, pack.z_dim, pack.h1, pack.h2) == (case[0], case[1], *case[2])
        _enc[case] = (pack, model, w, ER.inputs(ER.power(FRAMES), labels_of(case)), c_mu, c_lv)
    return _enc[case]


def clf_case(case):
    """(generic pack, classifier on the device, weights, c) of a classifier case, made once."""
    if case not in _clf:
        clf, w = rebuild_classifier(case)
        clf = frozen(clf)
        pack = C.ClassifierPack(clf, generic=True)
        assert pack.generic and (pack.h1, pack.h2, pack.y_dim) == (*case[0], case[1])
        _clf[case] = (pack, clf, w, MC.c_eff(GOLD[MC.clf_id(case) + "/c_ref"]))
    return _clf[case]


@pytest.fixture(scope="module", autouse=True)
def drop_the_cases(leave_the_allocator_as_found):
    yield
    _enc.clear()
    _clf.clear()


# ---- 1: every case within the bars -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MC.ENCODER_CASES, ids=MC.enc_id)
def test_encoder_case_within_the_bars(case):
    pack, _, w, V, c_mu, c_lv = enc_case(case)
    k = MC.enc_id(case) + "/"
    z_dim = case[1]
    eps = dev(GOLD[k + "eps"])
    P = dev(ER.power(FRAMES))
    worst = np.zeros(3)
    for source in ("complex", "rows", "rows_ld520"):
        for stride in (("packed", "wide") if case[0] else ("none",)):
            y = dev(labels_of(case))
            if stride == "wide":
                y = wide(y, 2)
            if source == "complex":
                lat = E.encode_batch(pack, spec_of(FRAMES, COUNTS), y, eps=eps)
            else:
                lat = E.encode_batch(pack, wide(P, 7) if source == "rows_ld520" else P, y, COUNTS, eps=eps)
            assert lat.mu.shape == (118, z_dim) and lat.frame_off.tolist() == [0, 33, 98, 118] and lat.view(1, "z").shape == (z_dim, 65)
            mu, lv, z = (t.cpu().numpy() for t in (lat.mu, lat.log_var, lat.z))
            worst = np.maximum(worst, ER.check(f"device {k} {source} labels {stride}", mu, lv, z, V, w, c_mu, c_lv, GOLD[k + "eps"]))
    print(f"{k} worst over sources and strides: mu {worst[0]:.3f} / log_var {worst[1]:.3f} / z {worst[2]:.3f} bars; against the reference's recorded "
          f"float32 mu {np.abs(mu - GOLD[k + 'mu']).max():.2e}")
    assert [a.shape for a in lat.numpy("log_var")] == [(z_dim, c) for c in COUNTS]


@pytest.mark.parametrize("case", MC.CLASSIFIER_CASES, ids=MC.clf_id)
def test_classifier_case_within_the_bars(case):
    pack, _, w, c = clf_case(case)
    k = MC.clf_id(case) + "/"
    P = CR.power(FRAMES)
    z64, Mass = CR.logits64(P, w), CR.mass(P, w)
    Pd = dev(P)
    for source in ("complex", "rows", "rows_ld520"):
        src = spec_of(FRAMES, COUNTS) if source == "complex" else wide(Pd, 7) if source == "rows_ld520" else Pd
        lb = C.classify_batch(pack, src, None if source == "complex" else COUNTS, want_logits=True)
        assert lb.y_dim == case[1] and lb.hard.shape == (118, case[1]) and lb.frame_off.tolist() == [0, 33, 98, 118]
        _, _, share = CR.check(f"device {k} {source}", lb.logits.cpu().numpy(), lb.soft.cpu().numpy(), lb.hard.cpu().numpy(), z64, Mass, c)
        assert share <= CR.EXCLUDED_CAP
    without = C.classify_batch(pack, Pd, COUNTS)
    assert without.logits is None and torch.equal(without.soft, lb.soft) and torch.equal(without.hard, lb.hard)
    assert torch.equal(lb.hard, (lb.soft > 0.5).to(torch.float32)), "hard is decided from the stored float32 soft"
    print(f"{k} against the reference's recorded float32 logits {np.abs(lb.logits.cpu().numpy() - GOLD[k + 'logit']).max():.2e}")


# ---- 2: bit identity and tile edges ------------------------------------------------------------------------------------------------------

EDGE_GEOMETRIES = [(0, 32, (256, 64)), (3, 17, (129, 127)), (513, 128, (512, 512))]


@pytest.mark.parametrize("case", EDGE_GEOMETRIES, ids=MC.enc_id)
def test_encoder_sources_tile_edges_batches_and_runs(case):
    pack = enc_case(case)[0]
    y_dim, z_dim, _ = case
    rng = np.random.default_rng(3)
    total, first, tail = sum(EDGES), 5, 23
    rows = first + total + tail
    frames = (rng.standard_normal((rows, 513)) + 1j * rng.standard_normal((rows, 513))).astype(np.complex64) * rng.random((rows, 1)).astype(np.float32) * 0.7
    src = dev(frames)
    y = dev((rng.random((rows, y_dim)) > 0.5).astype(np.float32)) if y_dim else None
    eps = dev(rng.standard_normal((rows, z_dim)).astype(np.float32))
    off = C.frame_table("test", EDGES, rows, first=first)
    cols = np.cumsum([3] + [c + 2 for c in EDGES[:-1]])                        # two free columns between the utterances, three in front
    ntot = int(cols[-1]) + EDGES[-1] + 4

    def run(src, y, eps, off, cols=None, ntot=0):
        outs = [torch.full((src.shape[0], z_dim), NAN, device=DEV) for _ in range(3)]
        Z = torch.full((z_dim, ntot), NAN, device=DEV) if cols is not None else None
        E.encode_rows(pack, src, off, y, eps, *outs, Z=Z, cols=cols)
        return [o.cpu().numpy() for o in outs] + ([Z.cpu().numpy()] if Z is not None else [])

    batch, again = run(src, y, eps, off, cols, ntot), run(src, y, eps, off, cols, ntot)
    for a, b in zip(batch, again):
        assert np.array_equal(bits(a), bits(b)), "two runs differ"
    # all sources give the same bits: the power formed in the kernel is numpy's float32 power
    P = dev(ER.power(frames))
    for name, other in (("power rows", run(P, y, eps, off)), ("power rows at ld 520, labels at a wider stride", run(wide(P, 7), None if y is None else wide(y, 2), eps, off))):
        for a, b in zip(batch[:3], other):
            assert np.array_equal(bits(a), bits(b)), name
    inside = np.zeros(rows, bool)
    inside[first:first + total] = True
    for nm, o in zip(("mu", "log_var", "z"), batch):
        assert np.all(np.isnan(o[~inside])), f"{nm}: rows outside the utterances were written"
        assert np.all(np.isfinite(o[inside])), f"{nm}: rows inside the utterances were left out"
    assert np.std(batch[0][inside]) > 0.01
    real = np.zeros(ntot, bool)
    for c0, c in zip(cols, EDGES):
        real[c0:c0 + c] = True
    assert np.all(np.isnan(batch[3][:, ~real])), "columns outside the utterances were written"
    assert np.array_equal(bits(batch[3][:, real]), bits(batch[0][inside].T)), "the column output is not mu transposed"
    for u, c in enumerate(EDGES):
        a, b = int(off[u]), int(off[u + 1])
        alone = run(src[a:b].contiguous(), None if y is None else y[a:b].contiguous(), eps[a:b].contiguous(), np.array([0, c], np.int64))
        for nm, o, full in zip(("mu", "log_var", "z"), alone, batch):
            assert np.array_equal(bits(o), bits(full[a:b])), f"utterance {u} ({c} frames): {nm} differs alone and in the batch"
    print(f"{MC.enc_id(case)}: {len(EDGES)} utterances of {EDGES} frames from row {first}: bit-identical over sources, alone, in the batch and twice; "
          f"{first} + {tail} outer rows and {int((~real).sum())} outer columns keep their NaNs")


def test_classifier_tile_edges_batches_and_runs():
    case = ((129, 127), 17)
    pack = clf_case(case)[0]
    rng = np.random.default_rng(4)
    total, first, tail = sum(EDGES), 5, 23
    rows = first + total + tail
    frames = (rng.standard_normal((rows, 513)) + 1j * rng.standard_normal((rows, 513))).astype(np.complex64) * rng.random((rows, 1)).astype(np.float32) * 0.7
    src = dev(frames)
    off = C.frame_table("test", EDGES, rows, first=first)

    def run(src, off):
        outs = [torch.full((src.shape[0], case[1]), NAN, device=DEV) for _ in range(3)]
        C.classify_rows(pack, src, off, *outs)
        return [o.cpu().numpy() for o in outs]

    batch, again, rows_src = run(src, off), run(src, off), run(wide(dev(CR.power(frames)), 7), off)
    for a, b, c in zip(batch, again, rows_src):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    inside = np.zeros(rows, bool)
    inside[first:first + total] = True
    for o in batch:
        assert np.all(np.isnan(o[~inside])) and np.all(np.isfinite(o[inside]))
    for u, c in enumerate(EDGES):
        a, b = int(off[u]), int(off[u + 1])
        for o, full in zip(run(src[a:b].contiguous(), np.array([0, c], np.int64)), batch):
            assert np.array_equal(bits(o), bits(full[a:b])), f"utterance {u} ({c} frames) differs alone and in the batch"


# ---- 3: the reference's geometry on both kernels ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_reference_encoder_on_both_kernels(name):
    model, w = rebuild_resident_encoder(name)
    model = frozen(model)
    y_dim = ER.CASES[name]
    V = ER.inputs(ER.power(FRAMES), resident_labels_of(name))
    c_mu, c_lv = (float(c) for c in ENC_GOLD[name + "/c_ref"])
    y, eps = dev(resident_labels_of(name)), dev(ENC_GOLD[name + "/eps"])
    assert E.encoder_kind(model.encoder, y_dim) == "resident" and not E.pack_encoder(model.encoder, y_dim).generic
    mus = []
    for generic in (False, True):
        pack = E.EncoderPack(model.encoder, y_dim, generic=generic)
        assert pack.generic == generic and (pack.z_dim, pack.h1, pack.h2) == (16, 128, 128)
        lat = E.encode_batch(pack, spec_of(FRAMES, COUNTS), y, eps=eps)
        mus.append(lat.mu)
        ER.check(f"{name} generic={generic}", lat.mu.cpu().numpy(), lat.log_var.cpu().numpy(), lat.z.cpu().numpy(), V, w, c_mu, c_lv, ENC_GOLD[name + "/eps"])
    print(f"{name}: mu of the two kernels bit-equal: {torch.equal(*mus)} (not required: two and four products per MFMA step)")
    # repack() after training: the pack follows the parameters
    with torch.no_grad():
        model.encoder.sample.mu.bias.add_(1.0)
    pack.repack(model.encoder)
    assert torch.allclose(E.encode_batch(pack, spec_of(FRAMES, COUNTS), y).mu, lat.mu + 1.0, atol=1e-5)
    with torch.no_grad():
        model.encoder.sample.mu.bias.sub_(1.0)


@pytest.mark.parametrize("y_dim", [1, 513])
def test_reference_classifier_on_both_kernels(y_dim):
    clf, w = rebuild_resident_classifier(CLF_GOLD, y_dim)
    clf = frozen(clf)
    P = CR.power(FRAMES)
    z64, Mass = CR.logits64(P, w), CR.mass(P, w)
    assert C.classifier_kind(clf) == "resident" and not C.pack_classifier(clf).generic
    for generic in (False, True):
        pack = C.ClassifierPack(clf, generic=generic)
        assert pack.generic == generic and (pack.h1, pack.h2, pack.y_dim) == (128, 128, y_dim)
        lb = C.classify_batch(pack, spec_of(FRAMES, COUNTS), want_logits=True)
        CR.check(f"y_dim {y_dim} generic={generic}", lb.logits.cpu().numpy(), lb.soft.cpu().numpy(), lb.hard.cpu().numpy(), z64, Mass, float(CLF_GOLD[f"y{y_dim}/c_ref"]))


# ---- 4: the column output and the fused start --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["M2", "M1"])
def test_fused_start_with_an_encoder_pack(variant):
    case = (1, 32, (256, 64)) if variant == "M2" else (0, 32, (256, 64))
    pack, vae, w, V, c_mu, c_lv = enc_case(case)
    assert E.encoder_kind(vae.encoder, case[0]) == "generic" and E.pack_encoder(vae.encoder, case[0]).generic
    spec = spec_of(FRAMES, COUNTS)
    Y = None if variant == "M1" else [labels_of(case)[a:b].T for a, b in zip((0, 33, 98), (33, 98, 118))]
    kw = dict(label_in_encoder=variant == "M2", label_in_decoder=variant == "M2")
    mk = lambda: M.McemBatch(vae, niter=2, nsamples_E_step=4, burnin_E_step=3, nsamples_WF=3, burnin_WF=3, reference_m1_counts=False, **kw)
    base, fused = mk(), mk()
    torch.manual_seed(11); base.init_parameters(spec, Y)
    torch.manual_seed(11); fused.init_parameters(spec, Y, fused_start=True, encoder_pack=pack)
    assert np.array_equal(bits(fused.X2), bits(base.X2))
    assert (fused.y is None) == (base.y is None) == (variant == "M1")
    if base.y is not None:
        assert fused.y.shape == base.y.shape and np.array_equal(bits(fused.y), bits(base.y))
    assert fused.Z.shape == base.Z.shape == (32, fused.ntot) and fused.Z.is_contiguous()
    real = np.zeros(fused.ntot, bool)
    for s, c in zip(fused.starts, COUNTS):
        real[s:s + c] = True
    Zf, Zb = fused.Z.cpu().numpy(), base.Z.cpu().numpy()
    assert np.all(Zf[:, ~real] == 0), "pad columns were written"
    lat = E.encode_batch(pack, spec, None if Y is None else dev(labels_of(case)))
    assert np.array_equal(bits(Zf[:, real]), bits(lat.mu.cpu().numpy().T))
    bar_mu = ER.bars(*ER.masses(V, w), c_mu, c_lv)[0]
    mu64 = ER.forward64(V, w)[0]
    wf, wb = ER.worst(Zf[:, real].T, mu64, bar_mu), ER.worst(Zb[:, real].T, mu64, bar_mu)
    between = float(np.max(np.abs(Zf[:, real].astype(np.float64) - Zb[:, real]) / bar_mu.T))
    print(f"{variant}: fused Z at {wf:.3f} bars of float64, the default path's at {wb:.3f}; apart by {between:.3f} bars")
    assert wf <= 1.0 and wb <= 1.0 and between <= 2.0
    cost = fused.run()
    assert fused._pack.generic and fused._pack.z_dim == 32
    assert cost.shape == (2, 3) and np.all(np.isfinite(cost))
    s = (fused.WFs + fused.WFn).cpu().numpy()[:, real]
    np.testing.assert_allclose(s, 1.0, rtol=1e-5)                            # the two gains partition the mixture (tests/test_gpu_mcem.py)
    # a pack that does not fit the model
    other_z = enc_case((1, 5, (48, 200)) if variant == "M2" else (0, 1, (1, 1)))[0]
    with pytest.raises(ValueError, match="z_dim"):
        mk().init_parameters(spec, Y, fused_start=True, encoder_pack=other_z)
    other_y = enc_case((0, 32, (256, 64)) if variant == "M2" else (1, 32, (256, 64)))[0]
    with pytest.raises(ValueError, match="y_dim"):
        mk().init_parameters(spec, Y, fused_start=True, encoder_pack=other_y)
    with pytest.raises(ValueError, match="fused_start"):
        mk().init_parameters(spec, Y, fused_start=True)                      # without a pack the refusal of an uncovered encoder stands


# ---- 5: reconstruct_batch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_eps", [False, True])
def test_reconstruct_batch_with_an_encoder_pack(with_eps):
    case = (1, 32, (256, 64))
    pack, model, *_ = enc_case(case)
    spec, y = spec_of(FRAMES, COUNTS), dev(labels_of(case))
    eps = dev(GOLD[MC.enc_id(case) + "/eps"]) if with_eps else None
    var, lat = E.reconstruct_batch(model, spec, y, eps, encoder_pack=pack)
    assert var.shape == (513, 118) and var.is_contiguous() and lat.counts == COUNTS and lat.mu.shape == (118, 32)
    zrows = lat.z if with_eps else lat.mu
    dpack = M.DecoderPack(model.decoder, 1)
    assert dpack.generic
    assert torch.equal(var, dpack.decode(zrows[:, None, :].contiguous(), y.T.contiguous())[0])
    z64 = zrows.cpu().numpy().astype(np.float64)
    want = _decoder64(model.decoder, np.concatenate([z64, labels_of(case).astype(np.float64)], axis=1)).T
    rtol, atol = _decode_bound()
    got = var.cpu().numpy().astype(np.float64)
    print(f"variance against float64 exp(decoder): worst {float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))):.3f} of the bound (rtol {rtol}, atol {atol})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)
    with pytest.raises(ValueError, match="label columns"):
        E.reconstruct_batch(model, spec, y, eps, encoder_pack=enc_case((0, 32, (256, 64)))[0])
    with pytest.raises(TypeError, match="128->128"):
        E.reconstruct_batch(model, spec, y, eps)                             # without a pack nothing changes: the bare module is refused


# ---- 6: a generic classifier's labels into MCEM and the F1 score -------------------------------------------------------------------------

def test_generic_classifier_labels_into_mcem_and_f1():
    case = ((256, 64), 1)
    pack = clf_case(case)[0]
    assert C.pack_classifier(clf_case(case)[1]).generic
    spec = spec_of(FRAMES, COUNTS)
    lb = C.classify_batch(pack, spec)
    hard = lb.hard.cpu().numpy()
    assert 0.05 < hard.mean() < 0.95
    vae = enc_case((1, 32, (256, 64)))[1]
    ys = []
    for form in (lb, lb.numpy("hard")):
        mb = M.McemBatch(vae, niter=1)
        torch.manual_seed(9)
        mb.init_parameters(spec, form)
        ys.append(mb.y.cpu().numpy())
    assert ys[0].shape == (1, mb.ntot) and np.array_equal(bits(ys[0]), bits(ys[1]))
    assert np.array_equal(np.concatenate([ys[0][:, s:s + c] for s, c in zip(mb.starts, COUNTS)], axis=1), hard.T)
    assert mb.Z.shape == (32, mb.ntot) and mb._pack.generic
    truth = CLF_GOLD["y1/truth"].astype(np.float32)
    got = C.f1_batch(lb, dev(truth), counts=COUNTS).cpu().numpy()
    off = lb.frame_off
    want = np.array([[v.numpy() for v in f1_loss(torch.from_numpy(hard[a:b].reshape(-1)), torch.from_numpy(truth[a:b].reshape(-1)), 1e-8)]
                     for a, b in zip(off[:-1], off[1:])], np.float32)
    print(got, want, sep="\n")
    assert np.array_equal(bits(got), bits(want))


# ---- 7: refusals through the C ABI -------------------------------------------------------------------------------------------------------

def test_bad_arguments_return_an_error_and_launch_nothing():
    lib = N.load()
    pack = enc_case((0, 32, (256, 64)))[0]
    cpack = clf_case(((256, 64), 1))[0]
    n, ntot, S = 40, 64, -7.5
    src = torch.zeros((n, 513), device=DEV)
    eps = torch.zeros((n, 32), device=DEV)
    outs = [torch.full((n, 32), S, device=DEV) for _ in range(3)]
    Z = torch.full((32, ntot), S, device=DEV)
    big = torch.full((n, 514), S, device=DEV)                                 # room for any refused width
    table = lambda *v: np.asarray(v, np.int64)
    good, cols = table(0, 10, 40), table(0, 32)
    tab_dev = dev(np.concatenate([good, cols]))

    def enc(y_dim=0, h1=256, h2=64, z=32, y_p=None, ldy=0, off=good, eps_p=N.ptr(eps), mu=N.ptr(outs[0]), lv=N.ptr(outs[1]), zs=N.ptr(outs[2]), Z_p=None,
            nt=0, col=None, tab=None):
        return lib.dvae_encode_generic_batch(N.ptr(src), 0, 513, y_p, ldy, n, 2, off.ctypes.data, N.ptr(pack.weights), y_dim, h1, h2, z, eps_p, mu, lv, zs,
                                             Z_p, nt, col.ctypes.data if col is not None else None, tab, N.stream())

    def clf(y_dim=1, h1=256, h2=64, off=good):
        return lib.dvae_classify_generic_batch(N.ptr(src), 0, 513, n, 2, off.ctypes.data, N.ptr(cpack.weights), y_dim, h1, h2, N.ptr(big), N.ptr(big), None,
                                               N.stream())

    def refused(rc, *words):
        msg = lib.dvae_last_error().decode()
        print(f"code {rc}: {msg}")
        assert rc == BADARG and all(w in msg for w in words), (rc, msg, words)

    # each limit exceeded by one: the size query answers 0, the call DVAE_E_BADARG with the limits named
    assert lib.dvae_encode_generic_weights_floats(0, 256, 64, 129) == 0
    refused(enc(z=129), "encode_generic_batch", "1..128")
    assert lib.dvae_encode_generic_weights_floats(0, 513, 64, 32) == 0 and lib.dvae_encode_generic_weights_floats(0, 256, 513, 32) == 0
    refused(enc(h1=513), "encode_generic_batch", "1..512")
    refused(enc(h2=513), "encode_generic_batch", "1..512")
    assert lib.dvae_encode_generic_weights_floats(514, 256, 64, 32) == 0
    refused(enc(y_dim=514, y_p=N.ptr(big), ldy=514), "encode_generic_batch", "0..513")
    assert lib.dvae_encode_generic_weights_floats(0, 0, 64, 32) == 0 and lib.dvae_encode_generic_weights_floats(0, 256, 64, 0) == 0
    assert lib.dvae_classify_generic_weights_floats(256, 64, 0) == 0 and lib.dvae_classify_generic_weights_floats(256, 64, 514) == 0
    refused(clf(y_dim=0), "classify_generic_batch", "1..513")
    refused(clf(y_dim=514), "classify_generic_batch", "1..513")
    assert lib.dvae_classify_generic_weights_floats(513, 64, 1) == 0 and lib.dvae_classify_generic_weights_floats(256, 513, 1) == 0
    refused(clf(h1=513), "classify_generic_batch", "1..512")
    w = pack.weights
    assert lib.dvae_encode_generic_pack(0, 256, 64, 129, *([N.ptr(w), 513, N.ptr(w)] * 4), N.ptr(w), N.stream()) == BADARG
    assert lib.dvae_classify_generic_pack(256, 64, 0, *([N.ptr(w), 513, N.ptr(w)] * 3), N.ptr(w), N.stream()) == BADARG
    assert lib.dvae_encode_generic_weights_floats(0, 256, 64, 32) == pack.weights.numel() == 256 * 528 + 64 * 256 + 64 * 64 + 256 + 64 + 64
    assert lib.dvae_classify_generic_weights_floats(256, 64, 1) == cpack.weights.numel() == 256 * 528 + 64 * 256 + 16 * 64 + 256 + 64 + 16
    # the tables
    withZ = dict(Z_p=N.ptr(Z), nt=ntot, col=cols, tab=N.ptr(tab_dev))
    refused(enc(eps_p=None), "z needs eps")
    refused(enc(**{**withZ, "col": table(0, 9)}), "goes back", "utterance 1")
    refused(enc(**{**withZ, "col": table(0, 35)}), "leaves", "utterance 1")
    refused(enc(off=table(0, 30, 20)), "utterance 1")
    refused(clf(off=table(0, 30, 20)), "utterance 1")
    refused(enc(mu=None, lv=None, zs=None), "no output")
    refused(enc(**{**withZ, "tab": None}), "column")
    torch.cuda.synchronize()
    assert all(bool((o == S).all()) for o in outs + [Z, big]), "a refused call wrote"
    assert enc(**withZ) == 0
    torch.cuda.synchronize()
    assert not any(bool((o == S).any()) for o in outs)
    Zh = Z.cpu().numpy()
    assert np.all(Zh[:, 10:32] == S) and np.all(Zh[:, 62:] == S) and not np.any(Zh[:, :10] == S) and not np.any(Zh[:, 32:62] == S)
    # the Python layer
    with pytest.raises(ValueError, match="utterance 2"):
        E.encode_batch(pack, src, counts=[10, 20, 11])
    with pytest.raises(ValueError, match=r"\[40, 32\]"):
        E.encode_rows(pack, src, good, mu=torch.empty((n, 16), device=DEV))


# ---- 8: the enhancement example ----------------------------------------------------------------------------------------------------------

def test_enhance_mcem_example_at_another_size_with_fused_start_and_classifier(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "enhance_mcem.py"), "--synthetic", "3", "--z-dim", "32", "--h-dim", "256", "64",
                        "--fused-start", "--labels", "classifier", "--score", "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr, sep="\n")
    assert r.returncode == 0
    assert len(list(tmp_path.glob("*_s_est.wav"))) == 3
    assert "SI-SDR estimate" in r.stdout and "F1" in r.stdout and "mean" in r.stdout

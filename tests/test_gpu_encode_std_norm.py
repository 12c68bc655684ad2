"""The generic encoder kernel with a standardised input (EncoderPack(..., norm=(mean, std)), pack_encoder(..., norm=);
csrc/mlp_generic.hip: dvae_encode_generic_batch_norm) on the cases of tests/mlp_generic_cases.py with COUNTS = [33, 65, 20], from complex
frames and from power rows:
  * mu, log_var and z within the bars of tests/encode_ref.py on V = [xn32 | y] (tests/test_encode_std_norm_cpu.py shows that the
    float32 CPU module on xn32 keeps them);
  * bit for bit the plain generic pack on rows (x - mean) / div formed by torch on the device: the kernel's subtraction and division
    are the IEEE ones;
  * a frame alone equals the frame inside the batch; the fused MCEM start takes the pack unchanged.
Every test prints its worst error in units of the bars before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import encode_ref as ER
import encode_std_norm_cases as EN
import mlp_generic_cases as MC
from test_gpu_encode import bits, dev, leave_the_allocator_as_found, spec_of, wide      # noqa: F401 (the fixture is used by name)
from test_mlp_generic_cpu import FRAMES, GOLD, labels_of, rebuild_encoder

pytestmark = pytest.mark.gpu
E = importlib.import_module("disentangled-vae_amd.encode")
M = importlib.import_module("disentangled-vae_amd.mcem")

DEV = "cuda"
COUNTS = MC.COUNTS
_enc = {}


def enc_case(case):
    """(pack with norm, plain generic pack, model on the device, weights, V = [xn32 | y], c mu, c log_var), made once."""
    if case not in _enc:
        model, w = rebuild_encoder(case)
        model = model.to(DEV).eval()
        for p in model.parameters():
            p.requires_grad = False
        c_mu, c_lv = (MC.c_eff(c) for c in GOLD[MC.enc_id(case) + "/c_ref"])
        pack = E.pack_encoder(model.encoder, case[0], norm=EN.stats(), norm_eps=EN.NORM_EPS)
        assert pack.generic and pack.norm is not None and (pack.y_dim, pack.z_dim, pack.h1, pack.h2) == (case[0], case[1], *case[2])
        plain = E.EncoderPack(model.encoder, case[0], generic=True)
        assert plain.norm is None
        _enc[case] = (pack, plain, model, w, EN.inputs(labels_of(case)), c_mu, c_lv)
    return _enc[case]


@pytest.fixture(scope="module", autouse=True)
def drop_the_cases(leave_the_allocator_as_found):
    yield
    _enc.clear()


def _normalised_on_the_device(P):
    mean, std = (dev(a) for a in EN.stats())
    return (P - mean) / (std + torch.tensor(EN.NORM_EPS, dtype=torch.float32, device=P.device))


@pytest.mark.parametrize("case", MC.ENCODER_CASES, ids=MC.enc_id)
def test_encoder_case_within_the_bars_and_ieee(case):
    pack, plain, _, w, V, c_mu, c_lv = enc_case(case)
    k = MC.enc_id(case) + "/"
    eps = dev(GOLD[k + "eps"])
    P = dev(ER.power(FRAMES))
    y = dev(labels_of(case))
    worst = np.zeros(3)
    outs = {}
    for source in ("complex", "rows", "rows_ld520"):
        if source == "complex":
            lat = E.encode_batch(pack, spec_of(FRAMES, COUNTS), y, eps=eps)
        else:
            lat = E.encode_batch(pack, wide(P, 7) if source == "rows_ld520" else P, None if y is None else wide(y, 2), COUNTS, eps=eps)
        assert lat.mu.shape == (118, case[1]) and lat.frame_off.tolist() == [0, 33, 98, 118]
        outs[source] = [t.cpu().numpy() for t in (lat.mu, lat.log_var, lat.z)]
        worst = np.maximum(worst, ER.check(f"device std_norm {k} {source}", *outs[source], V, w, c_mu, c_lv, GOLD[k + "eps"]))
    print(f"{k} worst over sources: mu {worst[0]:.3f} / log_var {worst[1]:.3f} / z {worst[2]:.3f} bars")
    # the plain pack on torch's (x - mean) / div: the same bits, so the kernel's subtraction and division are IEEE's
    xn = _normalised_on_the_device(P)
    assert np.array_equal(bits(xn), bits(EN.xn32()))
    ref = E.encode_batch(plain, xn.contiguous(), y, COUNTS, eps=eps)
    for source, o in outs.items():
        for name, a, b in zip(("mu", "log_var", "z"), o, (ref.mu, ref.log_var, ref.z)):
            assert np.array_equal(bits(a), bits(b)), (source, name)
    # and without norm the encoder answers something else
    other = E.encode_batch(plain, P, y, COUNTS).mu.cpu().numpy()
    assert not np.allclose(other, outs["rows"][0], atol=1e-3)


@pytest.mark.parametrize("case", [(0, 32, (256, 64)), (3, 17, (129, 127))], ids=MC.enc_id)
def test_a_frame_alone_equals_the_frame_in_the_batch(case):
    pack = enc_case(case)[0]
    P, y = dev(ER.power(FRAMES)), dev(labels_of(case))
    spec = spec_of(FRAMES, COUNTS)
    full = E.encode_batch(pack, spec, y)
    again = E.encode_batch(pack, spec, y)
    assert np.array_equal(bits(full.mu), bits(again.mu)) and np.array_equal(bits(full.log_var), bits(again.log_var))
    for r in (0, 15, 16, 32, 33, 97, 117):
        one = E.encode_batch(pack, P[r:r + 1].contiguous(), None if y is None else y[r:r + 1].contiguous(), [1])
        assert np.array_equal(bits(one.mu), bits(full.mu[r:r + 1])) and np.array_equal(bits(one.log_var), bits(full.log_var[r:r + 1])), r


@pytest.mark.parametrize("variant", ["M2", "M1"])
def test_fused_start_takes_the_pack(variant):
    case = (1, 32, (256, 64)) if variant == "M2" else (0, 32, (256, 64))
    pack, plain, vae, w, V, c_mu, c_lv = enc_case(case)
    spec = spec_of(FRAMES, COUNTS)
    Y = None if variant == "M1" else [labels_of(case)[a:b].T for a, b in zip((0, 33, 98), (33, 98, 118))]
    kw = dict(label_in_encoder=variant == "M2", label_in_decoder=variant == "M2")
    mc = M.McemBatch(vae, niter=2, nsamples_E_step=4, burnin_E_step=3, nsamples_WF=3, burnin_WF=3, reference_m1_counts=False, **kw)
    torch.manual_seed(11)
    mc.init_parameters(spec, Y, fused_start=True, encoder_pack=pack)
    real = np.zeros(mc.ntot, bool)
    for s, c in zip(mc.starts, COUNTS):
        real[s:s + c] = True
    Z = mc.Z.cpu().numpy()
    assert np.all(Z[:, ~real] == 0), "pad columns were written"
    y = None if Y is None else dev(labels_of(case))
    pre = E.encode_batch(plain, _normalised_on_the_device(dev(ER.power(FRAMES))).contiguous(), y, COUNTS)
    assert np.array_equal(bits(Z[:, real]), bits(pre.mu.cpu().numpy().T))      # the Z of the pre-normalised call
    bar_mu = ER.bars(*ER.masses(V, w), c_mu, c_lv)[0]
    wf = ER.worst(Z[:, real].T, ER.forward64(V, w)[0], bar_mu)
    print(f"{variant}: fused start Z with a standardised encoder input at {wf:.3f} bars of float64")
    assert wf <= 1.0
    cost = mc.run()
    assert cost.shape == (2, 3) and np.all(np.isfinite(cost))


def test_reconstruct_batch_takes_the_pack():
    case = (1, 32, (256, 64))
    pack, plain, model, *_ = enc_case(case)
    spec, y = spec_of(FRAMES, COUNTS), dev(labels_of(case))
    var, lat = E.reconstruct_batch(model, spec, y, None, encoder_pack=pack)
    pre = E.encode_batch(plain, _normalised_on_the_device(dev(ER.power(FRAMES))).contiguous(), y, COUNTS)
    assert var.shape == (513, 118) and bool(torch.isfinite(var).all()) and np.array_equal(bits(lat.mu), bits(pre.mu))

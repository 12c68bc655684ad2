"""CPU (no GPU): the premise of tests/test_gpu_encode_std_norm.py -- this repository's float32 CPU module on the standardised input
xn32 stays within the bars of tests/encode_ref.py with the case's recorded factor through c_eff -- and the host side of
EncoderPack(..., norm=)."""
import importlib

import numpy as np
import pytest
import torch

import encode_ref as ER
import encode_std_norm_cases as EN
import mlp_generic_cases as MC
from test_mlp_generic_cpu import GOLD, labels_of, rebuild_encoder

E = importlib.import_module("disentangled-vae_amd.encode")


def test_the_statistics_and_the_input():
    mean, std = EN.stats()
    xn = EN.xn32()
    assert mean.shape == std.shape == (513,) and np.all(std > 0) and np.all(np.isfinite(xn))
    assert np.abs(xn[:33].mean(0)).max() < 1e-3 and np.abs(xn[33:]).max() > 3.0        # the pool is centred, the rest is not the pool
    t = (torch.from_numpy(ER.power(MC.frames())) - torch.from_numpy(mean)) / (torch.from_numpy(std) + NORM32)
    assert np.array_equal(t.numpy().view(np.uint32), xn.view(np.uint32))               # torch's float32 expression, bit for bit


NORM32 = torch.tensor(EN.NORM_EPS, dtype=torch.float32)


@pytest.mark.parametrize("case", MC.ENCODER_CASES, ids=MC.enc_id)
def test_float32_cpu_module_on_the_standardised_input_is_within_the_bars(case):
    model, w = rebuild_encoder(case)
    k = MC.enc_id(case) + "/"
    c_mu, c_lv = (MC.c_eff(c) for c in GOLD[k + "c_ref"])
    V = EN.inputs(labels_of(case))
    with torch.no_grad():
        h = torch.from_numpy(V)
        for l in model.encoder.hidden:
            h = torch.tanh(l(h))
        mu, lv = model.encoder.sample.mu(h).numpy(), model.encoder.sample.log_var(h).numpy()
    eps = GOLD[k + "eps"]
    z = (mu + np.exp(np.float32(0.5) * lv) * eps).astype(np.float32)
    ER.check(f"float32 CPU module on xn32 {k}", mu, lv, z, V, w, c_mu, c_lv, eps)


def test_pack_refuses_bad_tables_before_the_device():
    model, _ = rebuild_encoder((0, 32, (256, 64)))
    for bad in [(np.zeros(512), np.ones(512)), (np.zeros(513), -np.ones(513)), (np.full(513, np.inf), np.ones(513)), (np.zeros(513),)]:
        with pytest.raises(ValueError, match="norm"):
            E.EncoderPack(model.encoder, 0, norm=bad)
        with pytest.raises(ValueError, match="norm"):
            E.pack_encoder(model.encoder, 0, norm=bad)

"""The MCEM oracle (oracle/mcem_oracle.py) against golden vectors captured from the reference's own
packages/models/mcem.py (tests/golden/make_mcem_golden.py), on the reference's recorded random draws."""
import os

import numpy as np
import pytest

import mcem_cases as mc
import golden_util as gu
from oracle import mcem_oracle as mo
from oracle import vae_oracle as vo

FIX = gu.load_golden("mcem_golden")


def case_fix(name):
    return {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + "/")}


def prefixes(model):
    return ("enc_dec_clf.encoder.", "enc_dec_clf.decoder.") if model == "M2_info" else ("encoder.", "decoder.")


def oracle_inputs(case, fix):
    params = gu.make_params(case["model"], mc.DIMS[case["model"]], case["seed"], case["wscale"])
    X, S, y = mc.make_utterance(case)
    assert abs(mc.checksum(X, S, y) - float(fix["input_checksum"])) < 1e-6 * float(fix["input_checksum"])
    X2 = (np.abs(X) ** 2).astype(np.float32)
    return params, X, X2, y


def encoder_z(case, params, X2, y, eps_noise):
    """init_parameters: Z = encoder(|X|^2 [, y]) (mcem.py:195-205, 358-370; M2v2/M2v3 feed x only)."""
    enc, _ = prefixes(case["model"])
    inp = X2.T if case["model"] != "M2" else np.concatenate([X2, y], axis=0).T
    return vo.encoder_fwd(params, enc, inp.astype(np.float32), eps_noise)["mu"].T   # `_, Z, _ = encoder(..)`: Z is mu


@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_oracle_reproduces_reference_run(case):
    fix = case_fix(case["name"])
    params, X, X2, y = oracle_inputs(case, fix)
    _, dec = prefixes(case["model"])
    Z0 = encoder_z(case, params, X2, y, fix["eps_X"])
    np.testing.assert_allclose(Z0, fix["Z0"], rtol=1e-4, atol=1e-5)
    W, H, g = mo.init_nmf(fix["rand_W"], fix["rand_H"], mc.EPS)
    n_e, b_e, n_wf, b_wf = mc.effective_counts(case)
    draws = [(fix[f"noise{i}"], fix[f"logu{i}"]) for i in range(case["niter"] + 1)]
    yd = None if case["model"] == "M1" else y
    hist = mo.run(params, dec, X2, yd, fix["Z0"], W, H, g, draws, case["niter"], n_e, b_e, n_wf, b_wf)
    for it in range(case["niter"]):
        # accept decisions are discrete: a frame whose chain took a different branch shows up as an O(0.1) jump
        dz = np.abs(hist["Z"][it] - fix["Z"][it]).max(axis=0)
        assert (dz > 1e-3).mean() <= 0.03, (it, dz.max())
        ok = dz <= 1e-3
        np.testing.assert_allclose(hist["g"][it][ok], fix["g"][it][ok], rtol=2e-3)
        np.testing.assert_allclose(hist["H"][it][:, ok], fix["H"][it][:, ok], rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(hist["W"][it], fix["W"][it], rtol=5e-3, atol=1e-6)
        np.testing.assert_allclose(hist["cost"][it], fix["cost"][it], rtol=1e-3)
    np.testing.assert_allclose(hist["Vb"], fix["Vb"], rtol=5e-3, atol=1e-7)
    bad = (np.abs(hist["WFs"] - fix["WFs"]) > 5e-3).mean()
    assert bad < 0.05, bad


@pytest.mark.parametrize("case", mc.CASES[:2], ids=[c["name"] for c in mc.CASES[:2]])
def test_m_step_and_wiener_alone(case):
    """M-step from the reference's state (no sampling involved): tight tolerances."""
    fix = case_fix(case["name"])
    params, X, X2, y = oracle_inputs(case, fix)
    _, dec = prefixes(case["model"])
    yd = None if case["model"] == "M1" else y
    W, H, g = mo.init_nmf(fix["rand_W"], fix["rand_H"], mc.EPS)
    n_e, b_e, _, _ = mc.effective_counts(case)
    Zs = mo.sample_posterior(params, dec, fix["Z0"], yd, g, W @ H, X2, fix["noise0"], fix["logu0"], b_e)
    if np.abs(Zs[:, -1, :].T - fix["Z"][0]).max() > 1e-3:
        pytest.skip("a chain branched differently in the first E-step; covered by the run test")
    Vs = mo.compute_vs(params, dec, Zs, yd)
    W1, H1, g1, Vb1, Vx1, cost = mo.m_step(X2, Vs, W, H, g, W @ H)
    np.testing.assert_allclose(W1, fix["W"][0], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(H1, fix["H"][0], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(g1, fix["g"][0], rtol=2e-4)
    np.testing.assert_allclose(cost, fix["cost"][0], rtol=1e-5)


def test_mcem_batch_runs_the_reference_m1_chain_lengths():
    """McemBatch mirrors MCEM_M1's argument shift (reference mcem.py:207, 297-298, 314-315): nsamples <- burnin, burnin <- 30."""
    import importlib
    dev = importlib.import_module("disentangled-vae_amd.mcem")
    case = dict(model="M1", n_e=10, b_e=30, n_wf=25, b_wf=75)
    mb = dev.McemBatch(None, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75, label_in_encoder=False, label_in_decoder=False)
    assert (mb.n_e, mb.b_e, mb.n_wf, mb.b_wf) == mc.effective_counts(case)
    mb = dev.McemBatch(None, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75, label_in_encoder=False, label_in_decoder=False,
                       reference_m1_counts=False)
    assert (mb.n_e, mb.b_e, mb.n_wf, mb.b_wf) == (10, 30, 25, 75)
    mb = dev.McemBatch(None, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75)          # M2: as written
    assert (mb.n_e, mb.b_e, mb.n_wf, mb.b_wf) == mc.effective_counts(dict(model="M2", n_e=10, b_e=30, n_wf=25, b_wf=75))

"""CPU (no GPU): the premises of tests/test_gpu_train_std_norm.py and tests/test_gpu_frame_stats.py, and the host side of std_norm.

  * the float64 truth of tests/std_norm_cases.py is torch.float64 autograd of the drop-in modules under the scripts' loop body;
  * float32 numpy on the same inputs needs less than a tenth of the bars the GPU test asserts;
  * the numpy restatement of dvae_frame_stats stays inside the bound derived in tests/frame_stats_ref.py;
  * FrameFile.stats(), the plan of dvae_train_generic_plan_norm, check_std_norm, trainer_kind and the refusals."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import fake_h5
import frame_stats_ref as fs
import std_norm_cases as sc
import train_generic_cases as tc

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")
TC = importlib.import_module("disentangled-vae_amd.trainer_classifier")
synth = importlib.import_module("disentangled-vae_amd.synth")


# ---- the truth and the bars ----

@pytest.mark.parametrize("case", [(3, 17, (129, 127)), (0, 32, (256, 64))], ids=tc.case_id)
def test_truth_is_float64_autograd_of_the_modules_under_the_scripts_loop_body(case):
    from packages.models import models as M
    from packages.models import utils as U
    B, model = 50, tc.model_of(case)
    l64, g64, _ = sc.truth(case, B)
    p, xn, x, y, eps = sc.cast_inputs(case, B, np.float64)
    t = lambda a: None if a is None else torch.from_numpy(a)
    m = synth.build_model(model, tc.dims_of(case)).double()
    m.load_state_dict({k: t(v) for k, v in p.items()}, strict=True)
    old = M.Stochastic.epsilon_fn
    M.Stochastic.epsilon_fn = lambda mu: t(eps)
    try:
        x_norm = t(xn)                                       # scripts/training_M2.py:136-144
        r, mu, logvar = m(x_norm) if model == "M1" else m(x_norm, t(y))
        loss, recon, kl = U.elbo(t(x), r, mu, logvar, 1e-8)
        loss.backward()
    finally:
        M.Stochastic.epsilon_fn = old
    got = np.array([loss.item(), recon.item(), kl.item()])
    assert tc.loss_err(got, l64[0]) <= 1e-12
    ge, name = tc.grad_err({k: v.grad.numpy() for k, v in m.named_parameters()}, g64[0])
    print(f"{tc.case_id(case)}: composed truth against float64 autograd, gradients {ge:.2e} ({name})")
    assert ge <= 1e-11


@pytest.mark.parametrize("case", sc.CASES, ids=tc.case_id)
def test_float32_arithmetic_needs_a_small_share_of_the_bars(case):
    for B in sc.BATCHES:
        l64, g64, _ = sc.truth(case, B)
        l32, g32, _ = sc.run(case, B, np.float32)
        le, (ge, name) = tc.loss_err(l32[0], l64[0]), tc.grad_err(g32[0], g64[0])
        print(f"{tc.case_id(case)} B {B}: float32 numpy losses {le:.2e}, gradients {ge:.2e} ({name})")
        assert le <= 0.1 * sc.LOSS_RTOL and ge <= 0.1 * sc.GRAD_TOL


def test_the_pool_is_not_the_batch():
    """|xn| is large in the batch and the plain step is far from the truth: the GPU test can see the feature."""
    case = (3, 17, (129, 127))
    xn = sc.cast_inputs(case, 50, np.float32)[1]
    assert np.max(np.abs(xn)) > 1e2 and np.all(np.isfinite(xn))
    l64 = sc.truth(case, 50)[0][0]
    plain = tc.truth(case, 50)[0][0]
    assert tc.loss_err(plain, l64) > 10 * sc.LOSS_RTOL


def test_trajectory_premises():
    case = sc.LOOPS_CASE
    l64, _, _ = sc.truth(case, sc.B_TRAJ, sc.STEPS_TRAJ, sc.LR_TRAJ)
    l32, _, _ = sc.run(case, sc.B_TRAJ, np.float32, sc.STEPS_TRAJ, sc.LR_TRAJ)
    for s in range(sc.STEPS_TRAJ):
        assert tc.loss_err(l32[s], l64[s]) <= 0.2 * sc.LOSS_RTOL, s


# ---- frame statistics ----

@pytest.mark.parametrize("n", [2, 3, 1000, 8195])
def test_restatement_is_inside_the_derived_bound(n):
    x = fs.make_frames(n, 5 + n)
    assert fs.check_inputs(x)
    mean, std = fs.stats_ref(x)
    M, sig, _, _ = fs.exact(x)
    bm, bs = fs.bound(x)
    rm = np.max(np.abs(mean.astype(np.float64) - np.asarray(M, np.float64)) / bm)
    rs = np.max(np.abs(std.astype(np.float64) - np.asarray(sig, np.float64)) / bs)
    varies = np.ptp(x[:, :513], axis=0) > 0
    print(f"n {n}: restatement error / bound: mean {rm:.3f}, std {rs:.3f}; worst relative bound on the std of a bin that varies "
          f"{np.max(bs[varies] / np.asarray(sig, np.float64)[varies]):.2e}")
    assert rm <= 1.0 and rs <= 1.0
    assert mean[fs.CONST_BIN] == fs.CONST_VALUE and std[fs.CONST_BIN] == 0.0 and mean[fs.ZERO_BIN] == 0.0 and std[fs.ZERO_BIN] == 0.0
    assert np.all(np.isfinite(std)) and std[fs.ODD_CONST_BIN] <= bs[fs.ODD_CONST_BIN]
    # against numpy's own two-pass statistics, which the reference's builder uses
    x64 = x[:, :513].astype(np.float64)
    np.testing.assert_allclose(mean, x64.mean(0), rtol=1e-6)
    np.testing.assert_allclose(std[varies], x64.std(0, ddof=1)[varies], rtol=1e-6)


def test_frame_file_stats(monkeypatch):
    from packages.data_handling import FrameFile
    rng = np.random.default_rng(0)
    mean, std = rng.random((513, 1)).astype(np.float32), rng.random((513, 1)).astype(np.float32)
    X = rng.random((513, 9)).astype(np.float32)
    F = fake_h5.install(monkeypatch, {"X_train": X, "Y_train": X[:1], "X_train_mean": mean, "X_train_std": std, "X_validation": X, "Y_validation": X[:1]})
    got = FrameFile("f.h5", "train").stats()
    assert got[0].shape == (513,) and got[1].shape == (513,) and got[0].dtype == np.float32
    assert np.array_equal(got[0], mean[:, 0]) and np.array_equal(got[1], std[:, 0])
    assert FrameFile("f.h5", "validation").stats() is None
    assert F.opened == 0


# ---- the host side ----

def _plans(case, B, ksplit=0):
    y, z, (h1, h2) = case
    lib, a, b = native.load(), G.GenericPlan(), G.GenericPlan()
    args = (T.MODEL_CODE[tc.model_of(case)], y, z, h1, h2, T.PREC_CODE["fp32"], B, ksplit)
    assert lib.dvae_train_generic_plan(*args, ctypes.byref(a)) == 0
    assert lib.dvae_train_generic_plan_norm(*args, 1, ctypes.byref(b)) == 0
    return a, b


@pytest.mark.parametrize("case", sc.CASES, ids=tc.case_id)
def test_plan_with_std_norm(case):
    """One stash block of 528 floats a padded frame more; LDS, slices, items and the tensor table as without it.  std_norm 0 through
    the new entry point is the old plan, byte for byte."""
    y, z, (h1, h2) = case
    for B in (1, 50, 8192):
        a, b = _plans(case, B)
        assert (a.std_norm, b.std_norm) == (0, 1)
        assert b.workspace_bytes - a.workspace_bytes == pytest.approx(a.Bp * 528 * 4, abs=256)
        for f in ("lds_bytes", "ksplit", "slice_frames", "wgrad_items", "rows_grid", "Bp", "n_params", "n_tensors"):
            assert getattr(a, f) == getattr(b, f), f
        assert b.grad_offset_bytes >= a.grad_offset_bytes
        c = G.GenericPlan()
        assert native.load().dvae_train_generic_plan_norm(T.MODEL_CODE[tc.model_of(case)], y, z, h1, h2, T.PREC_CODE["fp32"], B, 0, 0,
                                                          ctypes.byref(c)) == 0
        assert bytes(a) == bytes(c)
    assert native.load().dvae_train_generic_plan_norm(T.MODEL_CODE[tc.model_of(case)], y, z, h1, h2, T.PREC_CODE["fp32"], 8, 0, 2,
                                                      ctypes.byref(c)) == 1001


def test_check_std_norm():
    mean, std = np.linspace(0, 3, 513), np.linspace(0, 2, 513)
    m, d, s = G.check_std_norm((mean, std), 1e-8)
    assert m.dtype == d.dtype == np.float32 and np.array_equal(d, std.astype(np.float32) + np.float32(1e-8)) and np.array_equal(s, std.astype(np.float32))
    m2, d2, _ = G.check_std_norm((torch.from_numpy(mean).reshape(513, 1), torch.from_numpy(std).reshape(513, 1)))
    assert np.array_equal(m, m2) and np.array_equal(d, d2)
    one = G.check_std_norm((np.zeros(513), np.ones(513)))[1]
    assert np.all(one == 1.0)                                # 1 + 1e-8 rounds to 1: xn == x
    bad = [(mean[:512], std), (mean, -std - 1), (np.where(np.arange(513) == 3, np.nan, mean), std), (mean, np.where(np.arange(513) == 3, np.inf, std)),
           (mean,), "ab", (mean, None), (["a"] * 513, std)]
    for b in bad:
        with pytest.raises(ValueError):
            G.check_std_norm(b)
    with pytest.raises(ValueError, match="zero"):
        G.check_std_norm((mean, std), 0.0)                   # std[0] == 0 and no eps: a division by zero
    with pytest.raises(ValueError):
        G.check_std_norm((mean, std), -1.0)


def test_kinds_and_refusals_before_the_device():
    ref = dict(x_dim=513, z_dim=16, h_dim=(128, 128))
    good = (np.zeros(513), np.ones(513))
    assert T.trainer_kind("M2", dict(ref, y_dim=1)) == "resident" and T.trainer_kind("M2", dict(ref, y_dim=1), std_norm=True) == "generic"
    assert T.trainer_kind("M1", dict(ref, y_dim=0), std_norm=True) == "generic"
    assert T.trainer_kind("M2_info", dict(ref, y_dim=1), std_norm=True) is None
    assert T.trainer_kind("M2", dict(ref, y_dim=514), std_norm=True) is None
    with pytest.raises(ValueError, match="std"):             # a bad table is refused before the device is looked for
        G.GenericTrainer("M2", dict(ref, y_dim=1), batch=8, std_norm=(np.zeros(513), -np.ones(513)))
    with pytest.raises(ValueError):
        T.make_trainer("M2", dict(ref, y_dim=1), batch=8, std_norm=(np.zeros(5), np.ones(5)))
    with pytest.raises(NotImplementedError, match="M1 / M2"):
        T.make_trainer("M2_info", dict(ref, y_dim=1), batch=8, std_norm=good)
    with pytest.raises(NotImplementedError, match="std_norm.*1..512"):
        TI.make_info_trainer(dict(ref, y_dim=1), batch=8, std_norm=good)
    with pytest.raises(NotImplementedError, match="std_norm.*1..512"):
        TI.InfoTrainer(dict(ref, y_dim=1), batch=8, std_norm=good)
    with pytest.raises(NotImplementedError, match="std_norm.*1..512"):
        TC.ClassifierTrainer(dict(x_dim=513, y_dim=1, h_dim=(128, 128)), batch=8, std_norm=good)

"""CPU (no GPU): the host side of the generic fused train step -- dvae_train_generic_plan (include/dvae_train.h), trainer.trainer_kind --
and the premises of tests/test_gpu_train_generic.py: what float32 arithmetic itself needs of the bars that test asserts."""
import ctypes
import importlib

import numpy as np
import pytest

import train_generic_cases as tc

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
synth = importlib.import_module("disentangled-vae_amd.synth")

E_BADARG, E_UNSUPPORTED = 1001, 1003


def _plan(case, B, ksplit=0, model=None, precision="fp32"):
    y, z, (h1, h2) = case
    p = G.GenericPlan()
    rc = native.load().dvae_train_generic_plan(T.MODEL_CODE[model or tc.model_of(case)], y, z, h1, h2, T.PREC_CODE[precision], B, ksplit,
                                               ctypes.byref(p))
    return rc, p


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_plan_is_consistent(case):
    """Offsets 256-byte aligned and apart, rows x cols the drop-in module's state_dict shapes in its order, sizes monotone in B,
    the slices cover the frames, an explicit slice hint is honoured."""
    module = synth.build_model(tc.model_of(case), tc.dims_of(case))
    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    assert [k for k, _ in shapes] == T.TENSOR_NAMES
    prev = None
    for B in (1, 33, 50, 128, 8192, 1 << 20):
        rc, p = _plan(case, B)
        assert rc == 0, native.load().dvae_last_error()
        assert p.B == B and p.Bp % 16 == 0 and B <= p.Bp < B + 16 and p.n_tensors == 14
        end = 0
        for i, (name, shape) in enumerate(shapes):
            o, r, c = p.tensor_offset[i], p.tensor_rows[i], p.tensor_cols[i]
            assert o % 64 == 0 and o >= end, name
            assert (r, c) == (shape if len(shape) == 2 else (shape[0], 1)), name
            end = o + r * c
        assert p.n_params >= end and p.n_params % 64 == 0
        assert 1 <= p.ksplit <= 16 and p.slice_frames % 16 == 0
        assert (p.ksplit - 1) * p.slice_frames < B <= p.ksplit * p.slice_frames
        assert 1 <= p.rows_grid <= p.Bp // 16 and p.wgrad_items % p.ksplit == 0
        assert 0 < p.lds_bytes <= 160 * 1024
        assert p.grad_offset_bytes % 256 == 0 and p.workspace_bytes - p.grad_offset_bytes >= 4 * p.ksplit * p.n_params
        size = (p.workspace_bytes, p.grad_offset_bytes, p.Bp, p.rows_grid)
        assert prev is None or all(a >= b for a, b in zip(size, prev)), (B, size, prev)
        prev = size
    rc, p = _plan(case, 8192, ksplit=5)
    assert rc == 0 and p.ksplit == 5
    rc, p = _plan(case, 50, ksplit=1)
    assert rc == 0 and p.ksplit == 1 and p.slice_frames >= 50


@pytest.mark.parametrize("case,word", [((1, 16, (513, 128)), "hidden"), ((1, 16, (128, 513)), "hidden"), ((1, 129, (128, 128)), "z_dim"),
                                       ((514, 16, (128, 128)), "y_dim"), ((1, 0, (128, 128)), "z_dim"), ((1, 16, (0, 128)), "hidden"),
                                       ((1, 16, (128, 0)), "hidden"), ((-1, 16, (128, 128)), "y_dim")])
def test_limit_violations_are_bad_arguments(case, word):
    rc, _ = _plan(case, 128, model="M2")
    msg = native.load().dvae_last_error().decode()
    assert rc == E_BADARG and word in msg and "1..512" in msg and "1..128" in msg and "1..513" in msg, (rc, msg)


def test_model_and_label_width_must_agree():
    assert _plan((0, 16, (128, 128)), 128, model="M2")[0] == E_BADARG
    assert _plan((1, 16, (128, 128)), 128, model="M1")[0] == E_BADARG
    assert _plan((1, 16, (128, 128)), 0)[0] == E_BADARG


@pytest.mark.parametrize("model,precision", [("M2", "bf16"), ("M2", "bf16x3"), ("M2_info", "fp32"), ("M2_DEC", "fp32")])
def test_other_models_and_policies_are_unsupported(model, precision):
    rc, _ = _plan((1, 16, (128, 128)), 128, model=model, precision=precision)
    assert rc == E_UNSUPPORTED and b"reference geometry only" in native.load().dvae_last_error()
    with pytest.raises(NotImplementedError, match="reference geometry only"):
        G.make_plan(model, tc.dims_of((1, 16, (128, 128))), 128, precision)


def test_trainer_kind():
    ref = dict(x_dim=513, z_dim=16, h_dim=(128, 128))
    assert T.trainer_kind("M1", dict(ref, y_dim=0)) == "resident"
    assert T.trainer_kind("M2", dict(ref, y_dim=1)) == "resident" and T.trainer_kind("M2", dict(ref, y_dim=513)) == "resident"
    assert T.trainer_kind("M2_info", dict(ref, y_dim=1)) == "resident"
    assert T.trainer_kind("M2", dict(ref, y_dim=7)) == "generic"
    for case in tc.CASES:
        want = "resident" if T.supported(tc.model_of(case), tc.dims_of(case)) else "generic"
        assert T.trainer_kind(tc.model_of(case), tc.dims_of(case)) == want, case
    assert T.trainer_kind("M2", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))) == "generic"
    for model, dims in [("M2_info", dict(ref, y_dim=7)), ("M2_info", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))),
                        ("M2", dict(ref, y_dim=514)), ("M2", dict(x_dim=513, y_dim=1, z_dim=129, h_dim=(128, 128))),
                        ("M2", dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(513, 128))), ("M2", dict(x_dim=257, y_dim=1, z_dim=16, h_dim=(128, 128))),
                        ("M2", dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128, 128))), ("M1", dict(ref, y_dim=3)), ("M3", dict(ref, y_dim=1))]:
        assert T.trainer_kind(model, dims) is None, (model, dims)
        with pytest.raises(NotImplementedError, match="1..512"):
            T.make_trainer(model, dims)


# ---- the premises of the GPU test: float32 numpy on its exact inputs against the float64 truth ----

@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_float32_arithmetic_needs_a_small_share_of_the_bars(case):
    """One step at both batch sizes: the float32 numpy restatement stays below a tenth of the bars the GPU test asserts."""
    for B in tc.BATCHES:
        l64, g64, _ = tc.truth(case, B)
        l32, g32, _ = tc.run(case, B, np.float32)
        le, (ge, name) = tc.loss_err(l32[0], l64[0]), tc.grad_err(g32[0], g64[0])
        print(f"{tc.case_id(case)} B {B}: float32 numpy losses {le:.2e}, gradients {ge:.2e} ({name})")
        assert le <= 0.1 * tc.LOSS_RTOL and ge <= 0.1 * tc.GRAD_TOL


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_trajectory_premises(case):
    """Three steps at lr 1e-2: float32 numpy stays within a fifth of the loss bar of the float64 trajectory, and every step moves the
    loss by at least ten bars, so a missed update or a stale packed copy shows."""
    l64, _, _ = tc.truth(case, tc.B_TRAJ, tc.STEPS_TRAJ, tc.LR_TRAJ)
    l32, _, _ = tc.run(case, tc.B_TRAJ, np.float32, tc.STEPS_TRAJ, tc.LR_TRAJ)
    for s in range(tc.STEPS_TRAJ):
        assert tc.loss_err(l32[s], l64[s]) <= 0.2 * tc.LOSS_RTOL, s
    for s in range(1, tc.STEPS_TRAJ):
        move = abs(l64[s][0] - l64[s - 1][0]) / abs(l64[s][0])
        print(f"{tc.case_id(case)} step {s + 1}: the loss moves by {move:.2e}")
        assert move >= 10 * tc.LOSS_RTOL, (s, move)


def test_loops_case_premises():
    """The batch the loops test takes from the plan: more tiles than workgroups, at least two slices, the last shorter; float32 numpy
    at that batch stays below a third of the bars."""
    B, p = tc.loops_batch(lambda B: _plan(tc.LOOPS_CASE, B)[1])
    assert -(-B // 16) > p.rows_grid and p.ksplit >= 2 and 0 < B - (p.ksplit - 1) * p.slice_frames < p.slice_frames
    l64, g64, _ = tc.truth(tc.LOOPS_CASE, B)
    l32, g32, _ = tc.run(tc.LOOPS_CASE, B, np.float32)
    le, (ge, name) = tc.loss_err(l32[0], l64[0]), tc.grad_err(g32[0], g64[0])
    print(f"loops case B {B}: float32 numpy losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= tc.LOSS_RTOL / 3 and ge <= tc.GRAD_TOL / 3

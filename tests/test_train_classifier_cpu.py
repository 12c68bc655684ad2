"""CPU (no GPU): the host side of the classifier's fused train step -- dvae_train_clf_plan (include/dvae_train.h),
trainer_classifier.covered / make_plan -- and the premises of tests/test_gpu_train_classifier.py: the frame selection of
tests/train_classifier_cases.py holds, and float32 arithmetic itself needs less than a third of the bars that test asserts."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import train_classifier_cases as cc

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
classify = importlib.import_module("disentangled-vae_amd.classify")

E_BADARG, E_UNSUPPORTED = 1001, 1003


def _plan(case, B, ksplit=0, precision="fp32"):
    (h1, h2), y = case
    p = C.ClassifierPlan()
    rc = native.load().dvae_train_clf_plan(h1, h2, y, T.PREC_CODE[precision], B, ksplit, ctypes.byref(p))
    return rc, p


def _err():
    return native.load().dvae_last_error().decode()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_plan_is_consistent(case):
    """Offsets 256-byte aligned and apart, rows x cols the shapes of Classifier.state_dict() in its order, sizes monotone in B, the
    slices cover the frames, an explicit slice hint is honoured, the LDS of the rows kernel as the design sizes it."""
    from packages.models.models import Classifier
    shapes = [(k, tuple(v.shape)) for k, v in Classifier(cc.dims_of(case)).state_dict().items()]
    assert [k for k, _ in shapes] == C.NAMES == cc.NAMES
    (h1, h2), y = case
    up = lambda v: -(-v // 16) * 16
    prev = None
    for B in (1, 33, 50, 128, 8192, 1 << 20):
        rc, p = _plan(case, B)
        assert rc == 0, _err()
        assert (p.h1, p.h2, p.y_dim) == (h1, h2, y) and p.B == B and p.Bp % 16 == 0 and B <= p.Bp < B + 16 and p.n_tensors == 6
        end = 0
        for i, (name, shape) in enumerate(shapes):
            o, r, c = p.tensor_offset[i], p.tensor_rows[i], p.tensor_cols[i]
            assert o % 64 == 0 and o >= end, name
            assert (r, c) == (shape if len(shape) == 2 else (shape[0], 1)), name
            end = o + r * c
        assert p.n_params >= end and p.n_params % 64 == 0
        assert 1 <= p.ksplit <= 16 and p.slice_frames % 16 == 0
        assert (p.ksplit - 1) * p.slice_frames < B <= p.ksplit * p.slice_frames
        assert 1 <= p.rows_grid <= min(p.Bp // 16, 256) and p.wgrad_items % p.ksplit == 0
        # x tile [528][16], label tile, two hidden tiles, the frames' rows
        assert p.lds_bytes == 64 * (528 + up(y) + 2 * max(up(h1), up(h2))) + 128
        assert p.grad_offset_bytes % 256 == 0 and p.workspace_bytes - p.grad_offset_bytes >= 4 * p.ksplit * p.n_params
        stash = 4 * p.Bp * (2 * up(h1) + 2 * up(h2) + up(y))            # c1, c2, dpre1, dpre2, dpre_o of every padded frame
        assert p.workspace_bytes >= stash + 4 * p.ksplit * p.n_params
        size = (p.workspace_bytes, p.grad_offset_bytes, p.Bp, p.rows_grid)
        assert prev is None or all(a >= b for a, b in zip(size, prev)), (B, size, prev)
        prev = size
    rc, p = _plan(case, 8192, ksplit=5)
    assert rc == 0 and p.ksplit == 5
    rc, p = _plan(case, 50, ksplit=1)
    assert rc == 0 and p.ksplit == 1 and p.slice_frames >= 50


def test_lds_fits_at_every_limit():
    for h1 in (1, 512):
        for h2 in (1, 512):
            for y in (1, 513):
                rc, p = _plan(((h1, h2), y), 128)
                assert rc == 0 and 0 < p.lds_bytes <= 160 * 1024, ((h1, h2), y, p.lds_bytes)
    assert _plan(((512, 512), 513), 128)[1].lds_bytes == (528 + 528 + 2 * 512) * 64 + 128


@pytest.mark.parametrize("case", [((0, 128), 1), ((513, 128), 1), ((128, 0), 1), ((128, 513), 1), ((128, 128), 0), ((128, 128), 514)])
def test_sizes_outside_the_limits_are_unsupported(case):
    rc, _ = _plan(case, 128)
    msg = _err()
    assert rc == E_UNSUPPORTED and "1..512" in msg and "1..513" in msg and "fp32" in msg, (rc, msg)
    assert not C.covered(cc.dims_of(case))
    with pytest.raises(NotImplementedError, match="1..512"):
        C.make_plan(cc.dims_of(case), 128)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_other_precisions_are_unsupported(precision):
    rc, _ = _plan(((128, 128), 1), 128, precision=precision)
    assert rc == E_UNSUPPORTED and "operand policy" in _err() and "fp32" in _err()
    with pytest.raises(NotImplementedError, match="fp32"):
        C.make_plan([513, [128, 128], 1], 128, precision)
    with pytest.raises(NotImplementedError, match="fp32"):           # the plan refuses before anything touches the device
        C.ClassifierTrainer([513, [128, 128], 1], batch=8, precision=precision)


def test_batch_and_slices_are_bad_arguments():
    assert _plan(((128, 128), 1), 0)[0] == E_BADARG and "frames" in _err()
    assert _plan(((128, 128), 1), -3)[0] == E_BADARG
    assert _plan(((128, 128), 1), 128, ksplit=17)[0] == E_BADARG
    with pytest.raises(ValueError, match="frames"):
        C.make_plan([513, [128, 128], 1], 0)


def test_covered_and_other_shapes():
    from packages.models.models import Classifier
    for case in cc.CASES:
        assert C.covered(cc.dims_of(case)) and C.covered(Classifier(cc.dims_of(case)))
    for dims in ([257, [128, 128], 1], [513, [128], 1], [513, [128, 128, 128], 1], [513, [128, 128], 514], "M2"):
        assert not C.covered(dims)
        with pytest.raises(NotImplementedError, match="1..512"):
            C.make_plan(dims, 128)
    assert not C.covered(Classifier([513, [128, 128], 1], batch_norm=True))
    p = C.make_plan(Classifier([513, [48, 200], 2]), 33)
    assert (p.h1, p.h2, p.y_dim, p.B) == (48, 200, 2, 33)


def test_vae_trainers_keep_their_choice():
    """A spot check of tests/test_train_generic_cpu.py's assertions: the classifier step changes nothing in trainer_kind / make_trainer."""
    ref = dict(x_dim=513, z_dim=16, h_dim=(128, 128))
    assert T.trainer_kind("M2_info", dict(ref, y_dim=1)) == "resident" and T.trainer_kind("M2", dict(ref, y_dim=7)) == "generic"
    assert T.trainer_kind("M2_info", dict(ref, y_dim=7)) is None and T.trainer_kind("Classifier", dict(ref, y_dim=1)) is None
    with pytest.raises(NotImplementedError, match="1..512"):
        T.make_trainer("M2_info", dict(ref, y_dim=7))


# ---- the premises of the GPU test ----

@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_selection_rule_holds(case):
    """The pool suffices for every batch the tests use, the selected frames pass both conditions, and they are the FIRST that do."""
    for B in cc.BATCHES:
        idx, frac = cc.selection(case, B)
        x_pool, y_pool = cc.pool(case, B)
        ok = cc.frame_ok(case, x_pool)
        _, x, y = cc.inputs(case, B)
        print(f"{cc.case_id(case)} B {B}: {100 * frac:.0f} % of the pool passes, the last selected frame is number {idx[-1] + 1}")
        assert frac >= 0.28
        assert np.all(ok[idx]) and np.array_equal(idx, np.flatnonzero(ok)[:B])
        assert np.array_equal(x, x_pool[idx]) and np.array_equal(y, y_pool[idx]) and x.shape == (B, 513) and y.shape == (B, case[1])
        assert np.all(cc.frame_ok(case, x))


def test_selection_reach_at_the_widest_case():
    case = ((512, 512), 513)
    assert cc.selection(case, 50)[0][-1] < 161
    x, _ = cc.pool(case, 200)
    assert np.flatnonzero(cc.frame_ok(case, x))[199] < 713


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_float32_arithmetic_needs_less_than_a_third_of_the_bars(case):
    """One step at both batch sizes: the float32 numpy restatement stays below a third of the bars the GPU test asserts, and its hard
    counts equal the float64 ones."""
    for B in cc.BATCHES:
        l64, g64, c64, _ = cc.truth(case, B)
        l32, g32, c32, _ = cc.run(case, B, np.float32)
        le, (ge, name) = cc.loss_err(l32[0], l64[0]), cc.grad_err(g32[0], g64[0])
        print(f"{cc.case_id(case)} B {B}: float32 numpy loss {le:.2e}, gradients {ge:.2e} ({name})")
        assert le <= cc.LOSS_RTOL / 3 and ge <= cc.GRAD_TOL / 3
        assert np.array_equal(c32[0], c64[0]) and int(c64[0].sum()) == B * case[1]


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_trajectory_premises(case):
    """Three steps at lr 1e-2: float32 numpy stays within a third of the loss bar of the float64 trajectory with the same hard counts
    at every step."""
    l64, _, c64, _ = cc.truth(case, cc.B_TRAJ, cc.STEPS_TRAJ, cc.LR_TRAJ)
    l32, _, c32, _ = cc.run(case, cc.B_TRAJ, np.float32, cc.STEPS_TRAJ, cc.LR_TRAJ)
    errs = [cc.loss_err(l32[s], l64[s]) for s in range(cc.STEPS_TRAJ)]
    print(f"{cc.case_id(case)}: float32 numpy trajectory loss errors {['%.2e' % e for e in errs]}, losses {['%.4f' % v for v in l64]}")
    assert max(errs) <= cc.LOSS_RTOL / 3
    assert all(np.array_equal(a, b) for a, b in zip(c32, c64))


def test_loops_case_premises():
    """The batch the loops test takes from the plan: more tiles than workgroups, at least two slices, the last shorter; the pool
    suffices there and float32 numpy stays below a third of the bars."""
    B, p = cc.loops_batch(lambda B: _plan(cc.LOOPS_CASE, B)[1])
    assert -(-B // 16) > p.rows_grid and p.ksplit >= 2 and 0 < B - (p.ksplit - 1) * p.slice_frames < p.slice_frames
    l64, g64, c64, _ = cc.truth(cc.LOOPS_CASE, B)
    l32, g32, c32, _ = cc.run(cc.LOOPS_CASE, B, np.float32)
    le, (ge, name) = cc.loss_err(l32[0], l64[0]), cc.grad_err(g32[0], g64[0])
    print(f"loops case B {B}: float32 numpy loss {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= cc.LOSS_RTOL / 3 and ge <= cc.GRAD_TOL / 3 and np.array_equal(c32[0], c64[0])


def test_frames_alone_premises():
    """The frames test_a_frame_alone_is_its_term_of_the_batch compares alone with float64: enough of them, and float32 numpy on each
    needs less than a third of the loss bar."""
    case, B = ((48, 200), 2), 50
    idx = cc.alone_frames(case, B)
    p, x, y = cc.inputs(case, B)
    worst = 0.0
    for i in idx:
        l64, _, _, _ = cc.run_on(p, x[i:i + 1], y[i:i + 1], np.float64)
        l32, _, _, _ = cc.run_on(p, x[i:i + 1], y[i:i + 1], np.float32)
        worst = max(worst, cc.loss_err(l32[0], l64[0]))
    print(f"{idx.size} of {B} frames have every logit within {cc.LOGIT_ALONE}; float32 numpy alone: worst loss error {worst:.2e}")
    assert idx.size >= 16 and worst <= cc.LOSS_RTOL / 3


def test_a_zero_truth_demands_zeros():
    """grad_err: a tensor whose truth is all zero (a dead unit: every frame on the flat side of its ReLU) must be all zero.  Shown on
    the (1, 1) case with its unit switched off by a bias the frames cannot overcome."""
    p, x, y = cc.inputs(((1, 1), 1), 50)
    dead = dict(p)
    dead["hidden.1.bias"] = np.array([-1e6], np.float32)
    _, g64, _, _ = cc.run_on(dead, x, y, np.float64)
    _, g32, _, _ = cc.run_on(dead, x, y, np.float32)
    for k in ("hidden.0.weight", "hidden.0.bias", "hidden.1.weight", "hidden.1.bias", "output_layer.weight"):
        assert not np.any(g64[0][k]), k
    assert np.any(g64[0]["output_layer.bias"]) and cc.grad_err(g32[0], g64[0])[0] <= cc.GRAD_TOL / 3
    bad = {k: v.copy() for k, v in g64[0].items()}
    bad["hidden.0.bias"][0] = 1e-30
    assert cc.grad_err(bad, g64[0]) == (float("inf"), "hidden.0.bias")


@pytest.mark.parametrize("case", [((128, 128), 1), ((129, 127), 17)], ids=cc.case_id)
def test_f1_from_counts_is_f1_loss(case):
    """classify.f1_from_counts on the oracle's counts equals packages.models.utils.f1_loss on the same hard labels."""
    from packages.models.utils import f1_loss
    p, x, y = cc.inputs(case, 50)
    _, _, counts, soft = cc.loss_and_grads({k: v.astype(np.float64) for k, v in p.items()}, x.astype(np.float64), y.astype(np.float64))
    hard = torch.from_numpy((soft > 0.5).astype(np.float32).ravel())
    want = torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in f1_loss(hard, torch.from_numpy(y.ravel().copy()))])
    got = classify.f1_from_counts(torch.from_numpy(counts))
    assert torch.equal(got, want), (got, want)

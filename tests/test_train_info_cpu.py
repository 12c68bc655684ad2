"""CPU (no GPU): the host side of the generic M2_info fused train step -- dvae_train_info_plan (include/dvae_train.h),
trainer_info.covered / info_trainer_kind / make_info_trainer -- and the premises of tests/test_gpu_train_info.py: the frame selection
of tests/train_info_cases.py holds, float32 arithmetic itself needs less than half of the bars that test asserts, and the float64
trajectory keeps enough cases whole.  Every test prints its worst figures before it asserts."""
import ctypes
import importlib

import numpy as np
import pytest

import train_info_cases as ic

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
synth = importlib.import_module("disentangled-vae_amd.synth")

E_BADARG = 1001
LDS_MAX = 160 * 1024


def _plan(case, B, ksplit=0):
    y, z, (h1, h2) = case
    p = I.InfoPlan()
    rc = native.load().dvae_train_info_plan(y, z, h1, h2, B, ksplit, ctypes.byref(p))
    return rc, p


def _err():
    return native.load().dvae_last_error().decode()


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_plan_is_consistent(case):
    """26 tensors with the names, order and shapes of DeepGenerativeModel_v5.state_dict(); offsets 256-byte aligned and apart; the
    slices cover the frames; the script's loss weights; the LDS of the rows kernel as the design sizes it, within 160 KB; three launches
    whatever the batch."""
    shapes = [(k, tuple(v.shape)) for k, v in synth.build_model("M2_info", ic.dims_of(case)).state_dict().items()]
    assert [k for k, _ in shapes] == T.INFO_NAMES == list(ic.params_of(case))
    y, z, (h1, h2) = case
    up = lambda v: -(-v // 16) * 16
    prev, launches = None, set()
    for B in (1, 33, 50, 128, 8192, 1 << 20):
        rc, p = _plan(case, B)
        assert rc == 0, _err()
        assert (p.y_dim, p.z_dim, p.h1, p.h2) == (y, z, h1, h2) and p.B == B and p.Bp % 16 == 0 and B <= p.Bp < B + 16 and p.n_tensors == 26
        assert (p.info_alpha, p.info_beta, p.info_gamma) == (0.0, 10.0, 1.0)
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
        # the tiles of the M1 / M2 kernel and no more: x, labels, two hidden tiles, three latent tiles, the frames' rows
        assert p.lds_bytes == 64 * (528 + up(y) + 2 * max(up(h1), up(h2), up(z)) + 3 * up(z)) + 128 <= LDS_MAX
        assert p.grad_offset_bytes % 256 == 0 and p.workspace_bytes - p.grad_offset_bytes >= 4 * p.ksplit * p.n_params
        stash = 4 * p.Bp * (8 * up(h1) + 8 * up(h2) + 3 * up(z) + 528 + 2 * up(y))     # every layer input and pre-activation gradient
        assert p.workspace_bytes >= stash + 4 * p.ksplit * p.n_params
        size = (p.workspace_bytes, p.grad_offset_bytes, p.Bp, p.rows_grid)
        assert prev is None or all(a >= b for a, b in zip(size, prev)), (B, size, prev)
        prev = size
        launches.add(p.launches_per_step)
    print(f"{ic.case_id(case)}: launches per step {sorted(launches)}, LDS {p.lds_bytes} B")
    assert launches == {3}
    rc, p = _plan(case, 8192, ksplit=5)
    assert rc == 0 and p.ksplit == 5
    rc, p = _plan(case, 50, ksplit=1)
    assert rc == 0 and p.ksplit == 1 and p.slice_frames >= 50


def test_lds_fits_at_every_corner():
    worst = 0
    for h1 in (1, 512):
        for h2 in (1, 512):
            rc, p = _plan((513, 128, (h1, h2)), 128)
            assert rc == 0, _err()
            worst = max(worst, p.lds_bytes)
            assert 0 < p.lds_bytes <= LDS_MAX, ((h1, h2), p.lds_bytes)
    print(f"largest LDS plan {worst} B of {LDS_MAX}")
    assert _plan((513, 128, (512, 512)), 128)[1].lds_bytes == (528 + 528 + 2 * 512 + 3 * 128) * 64 + 128


def test_launch_count_does_not_depend_on_the_batch():
    for case in ic.CASES:
        assert _plan(case, 1)[1].launches_per_step == _plan(case, 1 << 20)[1].launches_per_step == 3


@pytest.mark.parametrize("case", [(0, 16, (128, 128)), (514, 16, (128, 128)), (1, 0, (128, 128)), (1, 129, (128, 128)), (1, 16, (0, 128)),
                                  (1, 16, (513, 128)), (1, 16, (128, 0)), (1, 16, (128, 513))], ids=ic.case_id)
def test_sizes_outside_the_limits_are_bad_arguments(case):
    rc, _ = _plan(case, 128)
    msg = _err()
    assert rc == E_BADARG and "1..513" in msg and "1..512" in msg and "1..128" in msg and "fp32" in msg, (rc, msg)
    assert not I.covered(ic.dims_of(case)) and I.info_trainer_kind(ic.dims_of(case)) is None
    with pytest.raises(ValueError, match="1..512"):
        I.make_plan(ic.dims_of(case), 128)
    with pytest.raises(NotImplementedError, match="1..512"):
        I.make_info_trainer(ic.dims_of(case), batch=8)


def test_batch_and_slices_are_bad_arguments():
    assert _plan((1, 16, (128, 128)), 0)[0] == E_BADARG and "frames" in _err()
    assert _plan((1, 16, (128, 128)), -3)[0] == E_BADARG
    assert _plan((1, 16, (128, 128)), 128, ksplit=17)[0] == E_BADARG
    with pytest.raises(ValueError, match="frames"):
        I.make_plan(ic.dims_of((1, 16, (128, 128))), 0)


def test_kinds():
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    assert I.info_trainer_kind(ref) == "resident" and I.covered(ref)
    for case in ic.CASES:
        want = "resident" if case == (1, 16, (128, 128)) else "generic"
        assert I.covered(ic.dims_of(case)) and I.info_trainer_kind(ic.dims_of(case)) == want, case
    assert I.info_trainer_kind(dict(ref, y_dim=513)) == "generic" and I.info_trainer_kind(dict(ref, z_dim=32, h_dim=(256, 64))) == "generic"
    for dims in (dict(ref, x_dim=257), dict(ref, h_dim=(128,)), dict(ref, h_dim=(128, 128, 128)), dict(ref, y_dim=0), dict(ref, z_dim=129), {}):
        assert I.info_trainer_kind(dims) is None and not I.covered(dims), dims
    # refused before anything touches the device, with the limits named
    wide = dict(ref, z_dim=32, h_dim=(256, 64))
    for kw in (dict(precision="bf16"), dict(precision="bf16x3"), dict(world=2)):
        for dims, generic in ((wide, False), (wide, True), (ref, True)):
            with pytest.raises(NotImplementedError, match="fp32, one GPU"):
                I.make_info_trainer(dims, generic=generic, batch=8, **kw)
    with pytest.raises(NotImplementedError, match="1..512"):
        I.make_info_trainer(dict(ref, h_dim=(128,)), generic=True, batch=8)


def test_the_other_trainers_keep_their_refusals():
    """A spot check of what tests/test_train_generic_cpu.py pins: the new step comes in through its own entry points only."""
    ref = dict(x_dim=513, z_dim=16, h_dim=(128, 128))
    G = importlib.import_module("disentangled-vae_amd.trainer_generic")
    assert T.trainer_kind("M2_info", dict(ref, y_dim=1)) == "resident" and T.trainer_kind("M2_info", dict(ref, y_dim=7)) is None
    assert T.trainer_kind("M2_info", dict(ref, y_dim=1, z_dim=32)) is None
    with pytest.raises(NotImplementedError):
        T.make_trainer("M2_info", dict(ref, y_dim=7))
    with pytest.raises(NotImplementedError, match="reference geometry only"):
        G.make_plan("M2_info", dict(ref, y_dim=1), 128)
    p = G.make_plan("M2", dict(ref, y_dim=7), 128)
    assert p.n_tensors == 14


# ---- the premises of the GPU test ----

@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_selection_rule_holds(case):
    """The pool suffices for every batch the tests use, the selected frames pass for both side nets, they are the FIRST that do, and
    they keep their own eps rows."""
    for B in ic.BATCHES:
        idx, n_ok = ic.selection(case, B)
        xp, yp, ep = ic.pool(case, B)
        ok = ic.frames_ok(ic.params_of(case), xp, ep)
        _, x, y, eps = ic.inputs(case, B)
        print(f"{ic.case_id(case)} B {B}: {n_ok} of {xp.shape[0]} pool frames pass, the last selected frame is number {idx[-1] + 1}")
        assert xp.shape[0] == 8 * B + 16 and n_ok >= B
        assert np.all(ok[idx]) and np.array_equal(idx, np.flatnonzero(ok)[:B])
        assert np.array_equal(x, xp[idx]) and np.array_equal(y, yp[idx]) and np.array_equal(eps, ep[idx])
        assert x.shape == (B, 513) and y.shape == (B, case[0]) and eps.shape == (B, case[1])
        assert np.all(ic.frames_ok(ic.params_of(case), x, eps))


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_float32_arithmetic_needs_less_than_half_of_the_bars(case):
    for B in ic.BATCHES:
        l64, g64, _, _ = ic.truth(case, B)
        l32, g32, _, _ = ic.run(case, B, np.float32)
        le, (ge, name) = ic.loss_err(l32[0], l64[0]), ic.grad_err(g32[0], g64[0])
        print(f"{ic.case_id(case)} B {B}: float32 numpy losses {le:.2e}, gradients {ge:.2e} ({name})")
        assert le <= ic.LOSS_RTOL / 2 and ge <= ic.GRAD_TOL / 2


def test_the_dead_unit_of_the_smallest_case_demands_zeros():
    """(1, 1, (1, 1)): the auxiliary net's second unit is off for every selected frame, so the truth of everything below it is all zero
    and grad_err asks for exact zeros there."""
    _, g64, _, _ = ic.truth((1, 1, (1, 1)), 50)
    dead = [k for k, v in g64[0].items() if not np.any(v)]
    print(f"all-zero truths at (1, 1, (1, 1)) B 50: {dead}")
    assert dead and all(k.startswith(ic.AUX) for k in dead)
    bad = {k: v.copy() for k, v in g64[0].items()}
    bad[dead[0]].flat[0] = 1e-30
    assert ic.grad_err(bad, g64[0]) == (float("inf"), dead[0])


def test_trajectory_premises():
    """Three steps at lr 1e-6 in the float64 oracle alone: at most a quarter of the cases drop (keep fewer than three quarters of their
    frames), every frame that is compared passes the selection at every step, the losses move by more than the bar at most cases, and
    float32 numpy stays within half of the loss bar on the compared frames."""
    dropped, worst, moved = [], 0.0, 0
    for case in ic.CASES:
        idx = ic.traj_frames(case)
        p, x, y, eps = ic.traj_inputs(case)
        l64, _, _, starts = ic.traj_truth(case)
        assert x.shape[0] == idx.size >= 1 and all(np.all(ic.frames_ok(s, x, eps)) for s in starts)
        if ic.traj_dropped(case):
            dropped.append(ic.case_id(case))
        l32 = ic.run_on(p, x, y, eps, np.float32, ic.STEPS_TRAJ, ic.LR_TRAJ)[0]
        errs = [ic.loss_err(l32[s], l64[s]) for s in range(ic.STEPS_TRAJ)]
        move = ic.loss_err(l64[-1], l64[0])
        moved += move > ic.LOSS_RTOL
        print(f"{ic.case_id(case)}: {idx.size} of {ic.B_TRAJ} frames, float32 numpy loss errors {['%.2e' % e for e in errs]}, "
              f"the float64 losses move by {move:.1e}")
        worst = max([worst] + errs)
    print(f"dropped cases: {dropped}; worst float32 error {worst:.2e}; {moved} cases move by more than the bar")
    assert len(dropped) <= ic.TRAJ_DROPPED_MAX * len(ic.CASES) and worst <= ic.LOSS_RTOL / 2 and moved >= 6


def test_loops_case_premises():
    B, p = ic.loops_batch(lambda B: _plan(ic.LOOPS_CASE, B)[1])
    assert -(-B // 16) > p.rows_grid and p.ksplit >= 2 and 0 < B - (p.ksplit - 1) * p.slice_frames < p.slice_frames
    l64, g64, _, _ = ic.truth(ic.LOOPS_CASE, B)
    l32, g32, _, _ = ic.run(ic.LOOPS_CASE, B, np.float32)
    le, (ge, name) = ic.loss_err(l32[0], l64[0]), ic.grad_err(g32[0], g64[0])
    print(f"loops case B {B}: float32 numpy losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= ic.LOSS_RTOL / 2 and ge <= ic.GRAD_TOL / 2


def test_weight_edges_in_the_oracle():
    """The loss-weight edges of the GPU test, in float64: alpha 0 leaves the classifier without gradient, gamma = beta the auxiliary net,
    and beta 0 takes the adversarial term out of the encoder."""
    case, B = (3, 17, (129, 127)), 50
    g = ic.truth(case, B, weights=(0.0, 10.0, 1.0))[1][0]
    assert all(not np.any(v) for k, v in g.items() if k.startswith(ic.CLF)) and any(np.any(v) for k, v in g.items() if k.startswith(ic.AUX))
    g = ic.truth(case, B, weights=(0.5, 10.0, 10.0))[1][0]
    assert all(not np.any(v) for k, v in g.items() if k.startswith(ic.AUX)) and any(np.any(v) for k, v in g.items() if k.startswith(ic.CLF))
    g0, g10 = ic.truth(case, B, weights=(0.5, 0.0, 1.0))[1][0], ic.truth(case, B)[1][0]
    assert not np.array_equal(g0[ic.ENC + "hidden.0.weight"], g10[ic.ENC + "hidden.0.weight"])
    assert np.array_equal(g0["enc_dec_clf.decoder.hidden.0.weight"], g10["enc_dec_clf.decoder.hidden.0.weight"])

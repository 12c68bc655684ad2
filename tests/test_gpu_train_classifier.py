"""The classifier's fused train step (csrc/train_classifier.hip; disentangled-vae_amd/trainer_classifier.py: ClassifierTrainer) against
the float64 oracle (oracle/vae_oracle.py: classifier_fwd, binary_cross_entropy, bce_bwd, classifier_bwd, AdamState) on the cases and the
selected frames of tests/train_classifier_cases.py.

Bars (train_classifier_cases.py): loss 1e-4 relative, every gradient tensor within 1e-4 of its maximum, a tensor whose truth is all zero
all zero -- the project's fp32 bar of the fused step.  The confusion counts equal the oracle's exactly.
tests/test_train_classifier_cpu.py shows that float32 numpy on the same inputs needs less than a third of the bars.  The optimizer update
is held per element to tests/adam_bounds.py.  Every test prints its worst figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import golden_util as gu
import train_classifier_cases as cc

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.trainer")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
classify = importlib.import_module("disentangled-vae_amd.classify")

DEV = "cuda:0"
LR = 1e-4


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the shared inputs are read-only)


def _trainer(case, B, **kw):
    params = cc.params_of(case) if "params" not in kw else kw.pop("params")
    return C.ClassifierTrainer(cc.dims_of(case), params=params, batch=B, device=DEV, **kw)


def _batch(case, B):
    _, x, y = cc.inputs(case, B)
    return _dev(x), _dev(y)


def _check_step(case, B, tr, loss, what, step=0, truth=None):
    l64, g64, c64, _ = truth or cc.truth(case, B)
    le = cc.loss_err(loss, l64[step])
    ge, name = cc.grad_err(tr.grads_numpy(), g64[step])
    counts = tr.counts.cpu().numpy()
    print(f"{what} {cc.case_id(case)} B {B}: loss {le:.2e}, gradients {ge:.2e} ({name}), counts {counts.tolist()}")
    assert le <= cc.LOSS_RTOL and ge <= cc.GRAD_TOL, (le, ge, name)
    assert np.array_equal(counts, c64[step]), (counts, c64[step])


@pytest.mark.parametrize("B", cc.BATCHES)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_one_step_against_float64(case, B):
    tr = _trainer(case, B, lr=LR)
    p0 = tr.state_dict_numpy()
    out = tr.step(*_batch(case, B))
    assert tuple(out.shape) == (1,) and out.device.type == "cuda"
    _check_step(case, B, tr, out.cpu().numpy()[0], "one step")
    p1 = tr.state_dict_numpy()
    for k in p0:
        assert np.all(np.isfinite(p1[k])) and np.max(np.abs(p1[k].astype(np.float64) - p0[k])) <= 1.05 * LR, k


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_adam_per_element(case):
    """From zero moments: p', m', v' equal the float64 update of the trainer's own gradient within the per-element bound."""
    B = 50
    tr = _trainer(case, B, lr=LR)
    p0 = tr.state_dict_numpy()
    tr.step(*_batch(case, B))
    g, p1 = tr.grads_numpy(), tr.state_dict_numpy()
    hyper = (1, LR, 0.9, 0.999, 1e-8)
    worst = 0.0
    for i, k in enumerate(tr.names):
        o, n = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i]
        z = np.zeros(n, np.float32)
        G32, P0 = g[k].ravel(), p0[k].ravel()
        want = ab.truth(P0, z, z, G32, hyper)
        bound = ab.bounds(P0, z, z, G32, hyper)
        got = (p1[k].ravel(), tr.m[o:o + n].cpu().numpy(), tr.v[o:o + n].cpu().numpy())
        for a, w, b in zip(got, want, bound):
            worst = max(worst, float(np.max(ab.ratios(a, w, b))))
    print(f"adam {cc.case_id(case)}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_three_steps_follow_the_float64_trajectory(case):
    B = cc.B_TRAJ
    l64, _, c64, _ = cc.truth(case, B, cc.STEPS_TRAJ, cc.LR_TRAJ)
    tr = _trainer(case, B, lr=cc.LR_TRAJ)
    batch = _batch(case, B)
    errs, same = [], []
    for s in range(cc.STEPS_TRAJ):
        errs.append(cc.loss_err(tr.step(*batch).cpu().numpy()[0], l64[s]))
        same.append(np.array_equal(tr.counts.cpu().numpy(), c64[s]))
    print(f"trajectory {cc.case_id(case)}: loss errors {['%.2e' % e for e in errs]}, counts equal {same}")
    assert max(errs) <= cc.LOSS_RTOL and all(same)


def test_loops_tiles_beyond_the_grid_and_a_short_last_slice():
    case = cc.LOOPS_CASE
    B, p = cc.loops_batch(lambda B: C.make_plan(cc.dims_of(case), B))
    tr = _trainer(case, B, lr=LR)
    assert tr.plan.rows_grid < -(-B // 16) and tr.plan.ksplit >= 2 and 0 < B - (tr.plan.ksplit - 1) * tr.plan.slice_frames < tr.plan.slice_frames
    batch = _batch(case, B)
    loss = tr.step(*batch).cpu().numpy()[0]
    _check_step(case, B, tr, loss, f"loops ({tr.plan.rows_grid} workgroups, {tr.plan.ksplit} slices of {tr.plan.slice_frames})")
    one = _trainer(case, B, lr=LR, ksplit=1)
    assert one.plan.ksplit == 1
    _check_step(case, B, one, one.step(*batch).cpu().numpy()[0], "loops, one slice")


def _state(tr):
    return [tr.losses.cpu().numpy().copy(), tr.counts.cpu().numpy().copy()] + list(tr.grads_numpy().values()) + list(tr.state_dict_numpy().values())


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


@pytest.mark.parametrize("ksplit", [0, 4])
def test_determinism(ksplit):
    case, B = ((129, 127), 17), 50
    batch = _batch(case, B)
    runs = []
    for _ in range(2):
        tr = _trainer(case, B, lr=cc.LR_TRAJ, ksplit=ksplit)
        rec = []
        for _ in range(2):
            tr.step(*batch)
            rec += _state(tr)
        runs.append(rec + [tr.m.cpu().numpy(), tr.v.cpu().numpy()])
    assert tr.plan.ksplit == (ksplit or 1)
    assert _same(*runs)
    _check_step(case, B, tr, tr.losses.cpu().numpy()[0], f"second step, {tr.plan.ksplit} slices", step=1,
                truth=cc.truth(case, B, 2, cc.LR_TRAJ))


def test_a_frame_alone_is_its_term_of_the_batch():
    """evaluate() exposes no row losses, so: the B = 1 loss of a frame against that frame's float64 term under the loss bar, on the
    frames where one frame alone can be held to it (train_classifier_cases.alone_frames: every logit within 6); and, on all frames, the
    float64 mean of the B = 1 losses against the batch's loss.  The batch rounds one double sum to float32 once, each frame alone
    rounds its own: the two differ by at most 2^-25 of the loss twice over; 4 * 2^-24 is asserted."""
    case, B = ((48, 200), 2), 50
    p, x, y = cc.inputs(case, B)
    alone = set(cc.alone_frames(case, B).tolist())
    one, many = _trainer(case, 1), _trainer(case, B)
    xd, yd = _batch(case, B)
    whole = float(many.evaluate(xd, yd).cpu().numpy()[0])
    terms, worst = [], 0.0
    for i in range(B):
        got = float(one.evaluate(xd[i:i + 1], yd[i:i + 1]).cpu().numpy()[0])
        if i in alone:
            worst = max(worst, cc.loss_err(got, cc.run_on(p, x[i:i + 1], y[i:i + 1], np.float64)[0][0]))
        terms.append(got)
    again = float(one.evaluate(xd[7:8], yd[7:8]).cpu().numpy()[0])
    print(f"{len(alone)} frames alone: worst loss error {worst:.2e}; batch loss {whole:.8g}, mean of the frames' {np.mean(terms):.8g}")
    assert len(alone) >= 16 and worst <= cc.LOSS_RTOL and again == terms[7]
    assert abs(whole - np.mean(terms)) <= 4 * 2.0 ** -24 * abs(whole)


def test_gather():
    case, B, n = ((129, 127), 17), 50, 70
    x, y = cc.pool(case, B)
    big_x, big_y = _dev(x[:100]), _dev(y[:100])
    store_x, store_y = big_x[:n], big_y[:n]                  # a leading slice of a larger allocation: row `n` is mapped memory
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:B].to(DEV)
    a, b = _trainer(case, B), _trainer(case, B)
    a.step(store_x, store_y, rows=perm)
    b.step(store_x[perm].contiguous(), store_y[perm].contiguous())
    assert a.bad_row_count() == 0 and _same(_state(a), _state(b))
    bad, fixed = perm.clone(), perm.clone()
    bad[7], fixed[7] = n, 0
    a, b = _trainer(case, B), _trainer(case, B)
    a.step(store_x, store_y, rows=bad)
    b.step(store_x, store_y, rows=fixed)
    assert a.bad_row_count() == 1 and a.bad_row_count() == 0 and b.bad_row_count() == 0
    assert _same(_state(a), _state(b))
    bad[9] = -1
    a.evaluate(store_x, store_y, rows=bad)
    assert a.bad_row_count() == 2


def test_evaluate_fork_and_running_sums():
    case, B = ((48, 200), 2), 50
    tr = _trainer(case, B, lr=cc.LR_TRAJ)
    batch = _batch(case, B)
    tr.step(*batch)                                          # moments are not zero from here on
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    total = torch.zeros(4, dtype=torch.int64, device=DEV)
    tr.accumulate_losses(acc)
    ev = tr.evaluate(*batch, counts=total)
    ev_counts = tr.counts.clone()
    assert ev.data_ptr() != tr.losses.data_ptr() and tuple(ev.shape) == (1,)
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.m, tr.v)))
    tr.evaluate(*batch, counts=total)
    st = tr.step(*batch).cpu().numpy().copy()
    tr.accumulate_losses(None)
    assert np.array_equal(ev.cpu().numpy().view(np.uint32), st.view(np.uint32)), (ev, st)
    assert torch.equal(ev_counts, tr.counts) and torch.equal(total, 2 * tr.counts) and int(tr.counts.sum()) == B * case[1]
    np.testing.assert_allclose(acc.cpu().numpy()[0], 3.0 * float(st[0]), rtol=1e-12)
    with pytest.raises(ValueError, match="int64"):
        tr.evaluate(*batch, counts=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="float64"):
        tr.accumulate_losses(torch.zeros(8, device=DEV))
    # a fork shares parameters and moments and sees the parent's update
    f = tr.fork(17)
    assert f.params.data_ptr() == tr.params.data_ptr() and f.m.data_ptr() == tr.m.data_ptr() and f.v.data_ptr() == tr.v.data_ptr() and f.B == 17
    small = tuple(t[:17].contiguous() for t in batch)
    l0 = f.evaluate(*small).cpu().numpy()
    tr.step(*batch)
    l1 = f.evaluate(*small).cpu().numpy()
    fresh = _trainer(case, 17, params=tr.state_dict_numpy())
    l2 = fresh.evaluate(*small).cpu().numpy()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and not np.array_equal(l0, l1)
    f.step(*small)                                           # and the parent sees the fork's
    again = _trainer(case, B, params=f.state_dict_numpy())
    assert np.array_equal(tr.evaluate(*batch).cpu().numpy().view(np.uint32), again.evaluate(*batch).cpu().numpy().view(np.uint32))
    assert tr.step_count == 4
    # grads_only leaves parameters and moments alone and gives the step's gradient
    g_tr = _trainer(case, B)
    g_tr.grads_only(*batch)
    ge, name = cc.grad_err(g_tr.grads_numpy(), cc.truth(case, B)[1][0])
    assert ge <= cc.GRAD_TOL and g_tr.step_count == 0 and not torch.any(g_tr.m)


def test_a_dead_unit_gives_exact_zeros():
    """The second hidden unit of (1, 1) switched off by its bias: every gradient below the output bias is exactly zero."""
    case, B = ((1, 1), 1), 50
    p, x, y = cc.inputs(case, B)
    dead = dict(p)
    dead["hidden.1.bias"] = np.array([-1e6], np.float32)
    l64, g64, c64, _ = cc.run_on(dead, x, y, np.float64)
    tr = _trainer(case, B, params=dead)
    loss = tr.step(_dev(x), _dev(y)).cpu().numpy()[0]
    _check_step(case, B, tr, loss, "dead unit", truth=(l64, g64, c64, None))
    g = tr.grads_numpy()
    assert not np.any(g["hidden.0.weight"]) and not np.any(g["hidden.1.weight"]) and np.any(g["output_layer.bias"])


def test_soft_labels_go_through_the_same_formulas():
    case, B = ((129, 127), 17), 50
    p, x, y = cc.inputs(case, B)
    soft = np.random.default_rng(5).random(y.shape).astype(np.float32)
    soft[::7] = y[::7]
    l64, g64, c64, _ = cc.run_on(p, x, soft, np.float64)
    tr = _trainer(case, B)
    loss = tr.step(_dev(x), _dev(soft)).cpu().numpy()[0]
    _check_step(case, B, tr, loss, "soft labels", truth=(l64, g64, c64, None))


def test_surface():
    from packages.models.models import Classifier
    ref_info = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    for case in [((128, 128), 1), ((48, 200), 2)]:
        dims = cc.dims_of(case)
        module = Classifier(dims)
        tr = C.ClassifierTrainer(dims, batch=8, device=DEV, seed=5)
        sd = tr.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
        # the seeded init: the module constructed under the seed, then xavier-normal weights and zero biases in module order -- what every
        # model of packages/models/models.py that owns a Classifier does to it
        torch.manual_seed(5)
        twin = Classifier(dims)
        for m in twin.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_normal_(m.weight.data)
                m.bias.data.zero_()
        assert all(torch.equal(sd[k].cpu(), v) for k, v in twin.state_dict().items())
        assert not torch.any(sd["hidden.0.bias"]) and torch.any(sd["hidden.0.weight"])
        module.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
        tr.load_state_dict(module.state_dict(), strict=True)
        with pytest.raises(KeyError):
            tr.load_state_dict({"hidden.0.bias": sd["hidden.0.bias"]})
        tr.load_state_dict({"hidden.0.bias": sd["hidden.0.bias"] + 1}, strict=False)
        assert torch.equal(tr.state_dict()["hidden.0.bias"], sd["hidden.0.bias"] + 1)
        # the prefix round trip
        psd = tr.state_dict(prefix=C.INFO_PREFIX)
        assert list(psd) == [C.INFO_PREFIX + k for k in C.NAMES]
        other = C.ClassifierTrainer(dims, batch=8, device=DEV, seed=6)
        other.load_state_dict(dict(psd, **{"enc_dec_clf.encoder.hidden.0.bias": torch.zeros(3)}), prefix=C.INFO_PREFIX)
        assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), tr.state_dict().values()))
        with pytest.raises(KeyError):
            other.load_state_dict(psd)
        # a trainer from a module takes its weights
        from_module = C.ClassifierTrainer(module.to(DEV), batch=8, device=DEV)
        assert all(torch.equal(a, b.detach()) for a, b in zip(from_module.state_dict().values(), module.state_dict().values()))
        with pytest.raises(ValueError, match="float32"):
            tr.step(torch.zeros(8, 513, device=DEV, dtype=torch.float64), torch.zeros(8, case[1], device=DEV))
        with pytest.raises(ValueError):
            tr.step(torch.zeros(8, 513, device=DEV), torch.zeros(8, case[1] + 1, device=DEV))
    with pytest.raises(NotImplementedError, match="1..512"):
        C.ClassifierTrainer([513, [513, 128], 1], batch=8, device=DEV)
    # the VAE trainers keep their choice
    assert type(T.make_trainer("M2", ref_info, batch=8, device=DEV)) is T.Trainer
    with pytest.raises(NotImplementedError):
        T.make_trainer("M2_info", ref_info, batch=8, device=DEV, generic=True)


@pytest.mark.parametrize("case", [((128, 128), 1), ((129, 127), 17)], ids=cc.case_id)
def test_to_module_labels_what_the_trainer_counted(case):
    """to_module() through pack_classifier and classify_batch: on the selected frames its hard labels score against y as tr.counts."""
    B = 50
    tr = _trainer(case, B)
    x, y = _batch(case, B)
    tr.evaluate(x, y)                # (the weights the frames were selected for: no logit of theirs lies within rounding of zero)
    assert np.array_equal(tr.counts.cpu().numpy(), cc.truth(case, B)[2][0])
    module = tr.to_module()
    assert isinstance(module, importlib.import_module("packages.models.models").Classifier)
    pack = classify.pack_classifier(module)
    assert pack.generic == (case != ((128, 128), 1))
    labels = classify.classify_batch(pack, x)
    got = classify.label_counts_batch(labels, y, counts=[B])
    print(f"{cc.case_id(case)}: classify_batch counts {got.cpu().numpy().tolist()}, trainer {tr.counts.cpu().numpy().tolist()}")
    assert torch.equal(got[0], tr.counts)
    f1 = classify.f1_from_counts(tr.counts)
    assert tuple(f1.shape) == (4,) and bool(torch.all((f1 >= 0) & (f1 <= 1)))


def test_round_trip_with_the_resident_m2info_trainer():
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    case, B = ((128, 128), 1), 50
    tr = _trainer(case, B, lr=cc.LR_TRAJ)
    tr.step(*_batch(case, B))
    info = T.Trainer("M2_info", dims, gu.make_params("M2_info", dims, 3), batch=8, device=DEV)
    before = info.state_dict()
    info.load_state_dict(tr.state_dict(prefix=C.INFO_PREFIX), strict=False)
    after = info.state_dict()
    mine = tr.state_dict(prefix=C.INFO_PREFIX)
    untouched = [k for k in after if k not in mine]
    assert len(untouched) == 20 and len(mine) == 6
    assert all(torch.equal(after[k], before[k]) for k in untouched) and all(torch.equal(after[k], mine[k]) for k in mine)
    assert any(not torch.equal(before[k], mine[k]) for k in mine)
    back = C.ClassifierTrainer(cc.dims_of(case), batch=8, device=DEV, seed=1)
    back.load_state_dict(info.state_dict(), prefix=C.INFO_PREFIX)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), tr.state_dict().values()))
    x, y, e = (_dev(a) for a in gu.make_batch(dims, 8, 4))
    assert np.all(np.isfinite(info.step(x, y, e).cpu().numpy()))


def test_raw_frames_stay_finite():
    """Raw, unselected make_batch frames at B = 50 include saturated sigmoids (and units within rounding of their ReLU's kink), where
    float32 and float64 disagree through no fault of a kernel (train_classifier_cases.py).  Loss, gradients and parameters after a step
    must be finite; nothing tighter is claimed there."""
    for case in [((128, 128), 1), ((512, 512), 513)]:
        B = 50
        x, y = cc.pool(case, B)
        assert not np.all(cc.frame_ok(case, x[:B]))
        tr = _trainer(case, B)
        loss = tr.step(_dev(x[:B]), _dev(y[:B])).cpu().numpy()
        assert np.all(np.isfinite(loss)) and all(np.all(np.isfinite(v)) for v in tr.grads_numpy().values())
        assert all(np.all(np.isfinite(v)) for v in tr.state_dict_numpy().values()) and int(tr.counts.sum()) == B * case[1]

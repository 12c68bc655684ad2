"""The two options of the generic M2_info fused train step (csrc/train_info.hip; disentangled-vae_amd/trainer_info.py: InfoTrainer,
dec_label / aux_enc) against the float64 truth of tests/train_info_modes_ref.py on the cases and modes of
tests/train_info_modes_cases.py.

Bars (train_info_cases.py): each of the seven losses 1e-4 relative, every gradient tensor 1e-4 of its maximum, an all-zero truth exactly
zero; the label columns of decoder layer 1 and the classifier's three weight matrices also 1e-4 of their own maximum.
tests/test_train_info_modes_cpu.py shows that float32 numpy on the same inputs needs less than half of them.  The optimizer update is
held per element to tests/adam_bounds.py.  Every test prints its worst figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import train_classifier_cases as cc
import train_info_cases as ic
import train_info_modes_cases as mc

pytestmark = pytest.mark.gpu
I = importlib.import_module("disentangled-vae_amd.trainer_info")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")

DEV = "cuda:0"
LR = 1e-4


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the shared inputs are read-only)


def _trainer(case, B, mode, weights=mc.WEIGHTS, **kw):
    params = ic.params_of(case) if "params" not in kw else kw.pop("params")
    a, b, g = weights
    tr = I.make_info_trainer(ic.dims_of(case), params=params, batch=B, device=DEV, alpha=a, beta=b, gamma=g, dec_label=mode[0],
                             aux_enc=mode[1], **kw)
    assert isinstance(tr, I.InfoTrainer) and tr.plan.launches_per_step == 3 and (tr.dec_label, tr.aux_enc) == tuple(mode)
    return tr


def _batch(case, B):
    _, x, y, eps = ic.inputs(case, B)
    return _dev(x), _dev(y), _dev(eps)


def _check_step(case, B, mode, tr, losses, what, weights=mc.WEIGHTS):
    l64, g64, _, _ = mc.truth(case, B, mode, weights=weights)
    le = mc.loss_err(losses, l64[0], mc.by_terms(case, mode, B))
    g = tr.grads_numpy()
    ge, name = ic.grad_err(g, g64[0])
    be, bname = ic.grad_err(mc.block_grads(g, case[1]), mc.block_grads(g64[0], case[1]))
    print(f"{what} {ic.case_id(case)} {mc.mode_id(mode)} B {B}: losses {le:.2e}, gradients {ge:.2e} ({name}), blocks {be:.2e} ({bname})")
    assert le <= ic.LOSS_RTOL and ge <= ic.GRAD_TOL and be <= ic.GRAD_TOL, (le, ge, name, be, bname)


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("mode", mc.MODES, ids=mc.mode_id)
@pytest.mark.parametrize("case", mc.CASES, ids=ic.case_id)
def test_one_step_against_float64(case, mode, B):
    tr = _trainer(case, B, mode, lr=LR)
    p0 = tr.state_dict_numpy()
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    assert losses.shape == (8,) and losses[7] == 0.0
    _check_step(case, B, mode, tr, losses, "one step")
    p1 = tr.state_dict_numpy()
    for k in p0:
        assert np.all(np.isfinite(p1[k])) and np.max(np.abs(p1[k].astype(np.float64) - p0[k])) <= 1.05 * LR, k


@pytest.mark.parametrize("case", [(3, 17, (129, 127)), (513, 128, (512, 512))], ids=ic.case_id)
def test_alpha_0_the_decoder_alone_trains_the_classifier(case):
    """The pretrain script's own setting: with alpha = 0 the label columns of decoder layer 1 are the classifier's only gradient."""
    B, mode, w = 50, mc.PRETRAIN, (0.0, 10.0, 10.0)
    tr = _trainer(case, B, mode, weights=w, lr=LR)
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    g = tr.grads_numpy()
    clf = [k for k in tr.names if k.startswith(ic.CLF)]
    print(f"alpha 0 {ic.case_id(case)}: smallest of the classifier tensors' largest gradients {min(float(np.max(np.abs(g[k]))) for k in clf):.1e}")
    assert len(clf) == 6 and all(np.any(g[k]) for k in clf) and losses[4] == 0.0
    _check_step(case, B, mode, tr, losses, "alpha 0", w)


def test_beta_0_divides_nothing():
    case, B, mode, w = (3, 17, (129, 127)), 50, ("truth", "entropy"), (0.5, 0.0, 1.0)
    tr = _trainer(case, B, mode, weights=w, lr=LR)
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    g = tr.grads_numpy()
    assert np.all(np.isfinite(losses)) and losses[6] == 0.0 and all(np.all(np.isfinite(v)) for v in g.values())
    _check_step(case, B, mode, tr, losses, "beta 0", w)
    # gamma dBCE alone: the auxiliary tensors of the default mode at beta 0
    g64 = ic.truth(case, B, weights=w)[1][0]
    aux = {k: v for k, v in g64.items() if k.startswith(ic.AUX)}
    ge, name = ic.grad_err(g, aux)
    print(f"beta 0: auxiliary gradients against gamma dBCE {ge:.2e} ({name})")
    assert len(aux) == 6 and ge <= ic.GRAD_TOL


@pytest.mark.parametrize("case", mc.CASES, ids=ic.case_id)
def test_adam_per_element(case):
    B, mode = 50, mc.PRETRAIN
    tr = _trainer(case, B, mode, lr=LR)
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
    print(f"adam {ic.case_id(case)}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode", mc.MODES, ids=mc.mode_id)
@pytest.mark.parametrize("case", mc.CASES, ids=ic.case_id)
def test_three_steps_follow_the_float64_trajectory(case, mode):
    _, x, y, eps = mc.traj_inputs(case, mode)
    l64 = mc.traj_truth(case, mode)[0]
    tr = _trainer(case, x.shape[0], mode, lr=mc.LR_TRAJ)
    batch = (_dev(x), _dev(y), _dev(eps))
    errs = [mc.loss_err(tr.step(*batch).cpu().numpy(), l64[s]) for s in range(ic.STEPS_TRAJ)]
    print(f"trajectory {ic.case_id(case)} {mc.mode_id(mode)} on {x.shape[0]} of {ic.B_TRAJ} frames: loss errors {['%.2e' % e for e in errs]}")
    assert max(errs) <= ic.LOSS_RTOL


def test_loops_tiles_beyond_the_grid_and_a_short_last_slice():
    case, mode = ic.LOOPS_CASE, mc.PRETRAIN
    B, p = ic.loops_batch(lambda B: I.make_plan(ic.dims_of(case), B, 0, *mode))
    tr = _trainer(case, B, mode, lr=LR)
    assert tr.plan.rows_grid < -(-B // 16) and tr.plan.ksplit >= 2 and 0 < B - (tr.plan.ksplit - 1) * tr.plan.slice_frames < tr.plan.slice_frames
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    _check_step(case, B, mode, tr, losses, f"loops ({tr.plan.rows_grid} workgroups, {tr.plan.ksplit} slices of {tr.plan.slice_frames})")


def _state(tr):
    return [tr.losses.cpu().numpy().copy()] + list(tr.grads_numpy().values()) + list(tr.state_dict_numpy().values())


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_gather():
    case, B, n, mode = (3, 17, (129, 127)), 50, 70, mc.PRETRAIN
    _, x, y, eps = ic.inputs(case, 100)
    big_x, big_y, eps = _dev(x), _dev(y), _dev(eps[:B])
    store_x, store_y = big_x[:n], big_y[:n]                  # a leading slice of a larger allocation: row `n` is mapped memory
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:B].to(DEV)
    a, b = _trainer(case, B, mode), _trainer(case, B, mode)
    a.step(store_x, store_y, eps, rows=perm)
    b.step(store_x[perm].contiguous(), store_y[perm].contiguous(), eps)
    assert a.bad_row_count() == 0 and _same(_state(a), _state(b))
    # one index past the store: counted once -- though the kernel reads the frame's labels in three phases -- and trained on row 0
    bad, fixed = perm.clone(), perm.clone()
    bad[7], fixed[7] = n, 0
    a, b = _trainer(case, B, mode), _trainer(case, B, mode)
    a.step(store_x, store_y, eps, rows=bad)
    b.step(store_x, store_y, eps, rows=fixed)
    assert a.bad_row_count() == 1 and a.bad_row_count() == 0 and b.bad_row_count() == 0
    assert _same(_state(a), _state(b))
    la = a.evaluate(store_x, store_y, eps, rows=bad).cpu().numpy()
    lb = b.evaluate(store_x, store_y, eps, rows=fixed).cpu().numpy()
    assert a.bad_row_count() == 1 and np.array_equal(la.view(np.uint32), lb.view(np.uint32))


@pytest.mark.parametrize("ksplit", [0, 4])
def test_determinism(ksplit):
    case, B, mode = (3, 17, (129, 127)), 50, mc.PRETRAIN
    batch = _batch(case, B)
    runs = []
    for _ in range(2):
        tr = _trainer(case, B, mode, lr=1e-2, ksplit=ksplit)
        rec = []
        for _ in range(2):
            rec.append(tr.step(*batch).cpu().numpy().copy())
            rec += list(tr.grads_numpy().values())
        runs.append(rec + list(tr.state_dict_numpy().values()))
    assert tr.plan.ksplit == (ksplit or 1)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    split = _trainer(case, B, mode, lr=LR, ksplit=ksplit)
    _check_step(case, B, mode, split, split.step(*batch).cpu().numpy(), f"{split.plan.ksplit} slices")


@pytest.mark.parametrize("mode", [mc.PRETRAIN, ("truth", "uniform")], ids=mc.mode_id)
def test_evaluate_fork_and_accumulate(mode):
    case, B = (1, 5, (48, 200)), 50
    tr = _trainer(case, B, mode, lr=1e-2)
    batch = _batch(case, B)
    ev0 = tr.evaluate(*batch).cpu().numpy()
    le = mc.loss_err(ev0, mc.truth(case, B, mode)[0][0], mc.by_terms(case, mode, B))
    print(f"evaluate {mc.mode_id(mode)}: losses {le:.2e}")
    assert le <= ic.LOSS_RTOL and tr.step_count == 0
    tr.step(*batch)                                          # moments are not zero from here on
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    grads = list(tr.grads_numpy().values())
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    tr.accumulate_losses(acc)
    ev = tr.evaluate(*batch).cpu().numpy()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.m, tr.v))) and _same(grads, list(tr.grads_numpy().values()))
    assert tr.step_count == 1
    st = tr.step(*batch).cpu().numpy().copy()
    tr.accumulate_losses(None)
    assert np.array_equal(ev.view(np.uint32), st.view(np.uint32)), (ev, st)
    got = acc.cpu().numpy()
    print(f"accumulated {got}")
    np.testing.assert_allclose(got[:7], 2.0 * st[:7].astype(np.float64), rtol=1e-12)
    assert got[7] == 0.0 and np.all(st[:7] != 0.0)
    # a fork carries the options, shares parameters and moments and sees the parent's update
    f = tr.fork(17)
    assert f.params.data_ptr() == tr.params.data_ptr() and f.m.data_ptr() == tr.m.data_ptr() and f.B == 17
    assert (f.alpha, f.beta, f.gamma) == mc.WEIGHTS and (f.dec_label, f.aux_enc) == tuple(mode) and f.plan.info_mode == tr.plan.info_mode != 0
    small = tuple(t[:17].contiguous() for t in batch)
    l0 = f.evaluate(*small).cpu().numpy()
    tr.step(*batch)
    l1 = f.evaluate(*small).cpu().numpy()
    fresh = _trainer(case, 17, mode, params=tr.state_dict_numpy())
    l2 = fresh.evaluate(*small).cpu().numpy()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and not np.array_equal(l0, l1)
    f.step(*small)                                           # and the parent sees the fork's
    again = _trainer(case, B, mode, params=f.state_dict_numpy())
    assert np.array_equal(tr.evaluate(*batch).cpu().numpy().view(np.uint32), again.evaluate(*batch).cpu().numpy().view(np.uint32))
    assert tr.step_count == 4


def test_surface():
    case, mode = (7, 16, (128, 128)), mc.PRETRAIN
    dims = ic.dims_of(case)
    tr = I.make_info_trainer(dims, batch=8, device=DEV, seed=5, dec_label=mode[0], aux_enc=mode[1])
    assert isinstance(tr, I.InfoTrainer) and tr.plan.info_mode == 5
    sd = tr.state_dict()
    twin = I.make_info_trainer(dims, batch=8, device=DEV, seed=6, dec_label=mode[0], aux_enc=mode[1])
    twin.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in twin.state_dict().items())
    # a classifier trained alone moves in under the pretrain script's prefix: only its six tensors change
    clf = C.ClassifierTrainer([513, list(case[2]), case[0]], batch=8, device=DEV, seed=9)
    tr.load_state_dict(clf.state_dict(prefix=cc.PREFIX), strict=False)
    now = tr.state_dict()
    moved = [k for k in now if not torch.equal(now[k], sd[k])]
    assert all(torch.equal(now[cc.PREFIX + k], v) for k, v in clf.state_dict().items())
    assert len(clf.state_dict()) == 6 and set(moved) <= {cc.PREFIX + k for k in clf.state_dict()} and len(moved) >= 3
    x, y, eps = (_dev(a[:8]) for a in ic.pool(case, 8))
    a = tr.step(x, y).cpu().numpy().copy()                   # noise drawn on the device from (seed, step)
    twin.load_state_dict(now, strict=True)
    b = twin.step(x, y, tr.noise(1)).cpu().numpy()
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    tr.grads_only(x, y, eps)
    assert all(np.all(np.isfinite(v)) for v in tr.grads_numpy().values())
    # the reference geometry goes to the generic step for a non-default option, and explicit defaults give the bits of no options
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    assert isinstance(I.make_info_trainer(ref, batch=8, device=DEV, aux_enc="uniform"), I.InfoTrainer)
    case, B = (3, 17, (129, 127)), 50
    batch = _batch(case, B)
    runs = []
    for kw in (dict(), dict(dec_label="truth", aux_enc="bce")):
        t = I.make_info_trainer(ic.dims_of(case), generic=True, params=ic.params_of(case), batch=B, device=DEV, **kw)
        assert t.plan.info_mode == 0
        t.step(*batch)
        t.step(*batch)
        runs.append(_state(t))
    assert _same(*runs)

"""The generic M2_info fused train step (csrc/train_info.hip; disentangled-vae_amd/trainer_info.py: InfoTrainer) against the float64
oracle (oracle/vae_oracle.py: m2info_losses_and_grads, train_step_m2info) on the cases of tests/train_info_cases.py.

Bars (train_info_cases.py): each of the seven losses 1e-4 relative, every gradient tensor 1e-4 of its maximum, an all-zero truth exactly
zero -- the project's fp32 bars of the fused step.  tests/test_train_info_cpu.py shows that float32 numpy on the same inputs needs less
than half of them.  The optimizer update is held per element to tests/adam_bounds.py.
Every test prints its worst figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import train_classifier_cases as cc
import train_info_cases as ic

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.trainer")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
synth = importlib.import_module("disentangled-vae_amd.synth")

DEV = "cuda:0"
LR = 1e-4


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the shared inputs are read-only)


def _trainer(case, B, weights=ic.WEIGHTS, **kw):
    params = ic.params_of(case) if "params" not in kw else kw.pop("params")
    a, b, g = weights
    return I.make_info_trainer(ic.dims_of(case), generic=True, params=params, batch=B, device=DEV, alpha=a, beta=b, gamma=g, **kw)


def _batch(case, B):
    _, x, y, eps = ic.inputs(case, B)
    return _dev(x), _dev(y), _dev(eps)


def _check_step(case, B, tr, losses, what, weights=ic.WEIGHTS):
    l64, g64, _, _ = ic.truth(case, B, weights=weights)
    le = ic.loss_err(losses, l64[0])
    ge, name = ic.grad_err(tr.grads_numpy(), g64[0])
    print(f"{what} {ic.case_id(case)} B {B}: losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= ic.LOSS_RTOL and ge <= ic.GRAD_TOL, (le, ge, name)


@pytest.mark.parametrize("B", ic.BATCHES)
@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_one_step_against_float64(case, B):
    tr = _trainer(case, B, lr=LR)
    assert isinstance(tr, I.InfoTrainer) and tr.plan.launches_per_step == 3
    p0 = tr.state_dict_numpy()
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    assert losses.shape == (8,) and losses[7] == 0.0
    _check_step(case, B, tr, losses, "one step")
    p1 = tr.state_dict_numpy()
    for k in p0:
        assert np.all(np.isfinite(p1[k])) and np.max(np.abs(p1[k].astype(np.float64) - p0[k])) <= 1.05 * LR, k


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_adam_per_element(case):
    """From zero moments: p', m', v' of all 26 tensors equal the float64 update of the trainer's own gradient within the per-element
    bound -- one update at the same step count for the auxiliary tensors too."""
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
    print(f"adam {ic.case_id(case)}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_three_steps_follow_the_float64_trajectory(case):
    """On the frames that pass the selection at every step of the float64 trajectory (train_info_cases.py: traj_frames)."""
    _, x, y, eps = ic.traj_inputs(case)
    l64 = ic.traj_truth(case)[0]
    tr = _trainer(case, x.shape[0], lr=ic.LR_TRAJ)
    batch = (_dev(x), _dev(y), _dev(eps))
    errs = [ic.loss_err(tr.step(*batch).cpu().numpy(), l64[s]) for s in range(ic.STEPS_TRAJ)]
    print(f"trajectory {ic.case_id(case)} on {x.shape[0]} of {ic.B_TRAJ} frames: loss errors {['%.2e' % e for e in errs]}")
    assert max(errs) <= ic.LOSS_RTOL


def test_loss_weight_edges():
    case, B = (3, 17, (129, 127)), 50
    batch = _batch(case, B)
    # the script's defaults: no gradient reaches the classifier, and its parameters stay as they are, bit for bit
    w = (0.0, 10.0, 1.0)
    tr = _trainer(case, B, weights=w, lr=LR)
    p0 = tr.state_dict_numpy()
    losses = tr.step(*batch).cpu().numpy()
    g, p1 = tr.grads_numpy(), tr.state_dict_numpy()
    clf = [k for k in tr.names if k.startswith(ic.CLF)]
    print(f"alpha 0: largest classifier gradient {max(float(np.max(np.abs(g[k]))) for k in clf):.1e}, classif_loss {losses[4]}")
    assert len(clf) == 6 and all(not np.any(g[k]) for k in clf) and losses[4] == 0.0
    assert all(np.array_equal(p0[k].view(np.uint32), p1[k].view(np.uint32)) for k in clf)
    _check_step(case, B, tr, losses, "alpha 0", w)
    # no adversarial term: nothing divides by beta, and the encoder's gradients are the oracle's without it
    w = (0.5, 0.0, 1.0)
    tr = _trainer(case, B, weights=w, lr=LR)
    losses = tr.step(*batch).cpu().numpy()
    assert np.all(np.isfinite(losses)) and losses[6] == 0.0
    _check_step(case, B, tr, losses, "beta 0", w)
    g64 = ic.truth(case, B, weights=w)[1][0]
    enc = {k: v for k, v in g64.items() if k.startswith(ic.ENC)}
    ge, name = ic.grad_err(tr.grads_numpy(), enc)
    print(f"beta 0: encoder gradients {ge:.2e} ({name})")
    assert len(enc) == 8 and ge <= ic.GRAD_TOL
    # gamma = beta: the two backward passes cancel in the auxiliary net
    w = (0.5, 10.0, 10.0)
    tr = _trainer(case, B, weights=w, lr=LR)
    losses = tr.step(*batch).cpu().numpy()
    g = tr.grads_numpy()
    aux = [k for k in tr.names if k.startswith(ic.AUX)]
    print(f"gamma = beta: largest auxiliary gradient {max(float(np.max(np.abs(g[k]))) for k in aux):.1e}")
    assert len(aux) == 6 and all(not np.any(g[k]) for k in aux)
    _check_step(case, B, tr, losses, "gamma = beta", w)


def test_loops_tiles_beyond_the_grid_and_a_short_last_slice():
    case = ic.LOOPS_CASE
    B, p = ic.loops_batch(lambda B: I.make_plan(ic.dims_of(case), B))
    tr = _trainer(case, B, lr=LR)
    assert tr.plan.rows_grid < -(-B // 16) and tr.plan.ksplit >= 2 and 0 < B - (tr.plan.ksplit - 1) * tr.plan.slice_frames < tr.plan.slice_frames
    batch = _batch(case, B)
    losses = tr.step(*batch).cpu().numpy()
    _check_step(case, B, tr, losses, f"loops ({tr.plan.rows_grid} workgroups, {tr.plan.ksplit} slices of {tr.plan.slice_frames})")
    one = _trainer(case, B, lr=LR, ksplit=1)
    assert one.plan.ksplit == 1
    _check_step(case, B, one, one.step(*batch).cpu().numpy(), "loops, one slice")


@pytest.mark.parametrize("ksplit", [0, 4])
def test_determinism(ksplit):
    case, B = (3, 17, (129, 127)), 50
    batch = _batch(case, B)
    runs = []
    for _ in range(2):
        tr = _trainer(case, B, lr=1e-2, ksplit=ksplit)
        rec = []
        for _ in range(2):
            rec.append(tr.step(*batch).cpu().numpy().copy())
            rec += list(tr.grads_numpy().values())
        runs.append(rec + list(tr.state_dict_numpy().values()))
    assert tr.plan.ksplit == (ksplit or 1)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    split = _trainer(case, B, lr=LR, ksplit=ksplit)
    _check_step(case, B, split, split.step(*batch).cpu().numpy(), f"{split.plan.ksplit} slices")


def _state(tr):
    return [tr.losses.cpu().numpy().copy()] + list(tr.grads_numpy().values()) + list(tr.state_dict_numpy().values())


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_gather():
    case, B, n = (3, 17, (129, 127)), 50, 70
    _, x, y, eps = ic.inputs(case, 100)
    big_x, big_y, eps = _dev(x), _dev(y), _dev(eps[:B])
    store_x, store_y = big_x[:n], big_y[:n]                  # a leading slice of a larger allocation: row `n` is mapped memory
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:B].to(DEV)
    a, b = _trainer(case, B), _trainer(case, B)
    a.step(store_x, store_y, eps, rows=perm)
    b.step(store_x[perm].contiguous(), store_y[perm].contiguous(), eps)
    assert a.bad_row_count() == 0 and _same(_state(a), _state(b))
    bad, fixed = perm.clone(), perm.clone()
    bad[7], fixed[7] = n, 0
    a, b = _trainer(case, B), _trainer(case, B)
    a.step(store_x, store_y, eps, rows=bad)
    b.step(store_x, store_y, eps, rows=fixed)
    assert a.bad_row_count() == 1 and a.bad_row_count() == 0 and b.bad_row_count() == 0
    assert _same(_state(a), _state(b))
    bad[9], fixed[9] = -1, 0
    la = a.evaluate(store_x, store_y, eps, rows=bad).cpu().numpy()
    lb = b.evaluate(store_x, store_y, eps, rows=fixed).cpu().numpy()
    assert a.bad_row_count() == 2 and np.array_equal(la.view(np.uint32), lb.view(np.uint32))


def test_evaluate_fork_and_accumulate():
    case, B = (1, 5, (48, 200)), 50
    tr = _trainer(case, B, lr=1e-2)
    batch = _batch(case, B)
    tr.step(*batch)                                          # moments are not zero from here on
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    grads = list(tr.grads_numpy().values())
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    tr.accumulate_losses(acc)
    ev = tr.evaluate(*batch).cpu().numpy()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.m, tr.v))) and _same(grads, list(tr.grads_numpy().values()))
    st = tr.step(*batch).cpu().numpy().copy()
    tr.accumulate_losses(None)
    assert np.array_equal(ev.view(np.uint32), st.view(np.uint32)), (ev, st)
    got = acc.cpu().numpy()
    print(f"accumulated {got}")
    np.testing.assert_allclose(got[:7], 2.0 * st[:7].astype(np.float64), rtol=1e-12)
    assert got[7] == 0.0 and np.all(st[:7] != 0.0)
    # a fork shares parameters and moments and sees the parent's update
    f = tr.fork(17)
    assert f.params.data_ptr() == tr.params.data_ptr() and f.m.data_ptr() == tr.m.data_ptr() and f.B == 17
    assert (f.alpha, f.beta, f.gamma) == ic.WEIGHTS
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


def test_surface():
    for case in [(7, 16, (128, 128)), (1, 32, (256, 64))]:
        dims = ic.dims_of(case)
        module = synth.build_model("M2_info", dims)
        tr = I.make_info_trainer(dims, batch=8, device=DEV, seed=5)
        assert isinstance(tr, I.InfoTrainer) and (tr.alpha, tr.beta, tr.gamma) == (0.0, 10.0, 1.0)
        sd = tr.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
        torch.manual_seed(5)                                 # the seeded init is the drop-in module's
        twin = synth.build_model("M2_info", dims)
        assert all(torch.equal(sd[k].cpu(), v) for k, v in twin.state_dict().items())
        module.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
        tr.load_state_dict(module.state_dict(), strict=True)
        with pytest.raises(KeyError):
            tr.load_state_dict({"auxiliary.hidden.0.bias": sd["auxiliary.hidden.0.bias"]})
        tr.load_state_dict({"auxiliary.hidden.0.bias": sd["auxiliary.hidden.0.bias"] + 1}, strict=False)
        assert torch.equal(tr.state_dict()["auxiliary.hidden.0.bias"], sd["auxiliary.hidden.0.bias"] + 1)
        # a classifier trained alone moves in under the pretrain script's prefix
        clf = C.ClassifierTrainer([513, list(case[2]), case[0]], batch=8, device=DEV, seed=9)
        tr.load_state_dict(clf.state_dict(prefix=cc.PREFIX), strict=False)
        now = tr.state_dict()
        assert all(torch.equal(now[cc.PREFIX + k], v) for k, v in clf.state_dict().items())
        assert torch.equal(now["enc_dec_clf.encoder.hidden.0.weight"], sd["enc_dec_clf.encoder.hidden.0.weight"])
        x, y, eps = (_dev(a) for a in synth.make_batch(dims, 8, 1))
        a = tr.step(x, y).cpu().numpy().copy()               # noise drawn on the device from (seed, step)
        assert np.all(np.isfinite(a)) and tuple(tr.noise(1).shape) == (8, case[1]) and torch.equal(tr.noise(1), tr.noise(1))
        assert tr.losses_host().shape == (8,)
        tr.grads_only(x, y, eps)
        assert all(np.all(np.isfinite(v)) for v in tr.grads_numpy().values())
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    assert type(I.make_info_trainer(ref, batch=8, device=DEV)) is T.Trainer
    assert isinstance(I.make_info_trainer(ref, batch=8, device=DEV, generic=True), I.InfoTrainer)
    with pytest.raises(NotImplementedError):
        T.Trainer("M2_info", dict(ref, y_dim=7), batch=8, device=DEV)

"""The generic fused train step (csrc/train_generic.hip; disentangled-vae_amd/trainer_generic.py: GenericTrainer) against the float64
oracle (oracle/vae_oracle.py: vae_loss_and_grads, train_step_vae) on the cases of tests/train_generic_cases.py.

Bars (train_generic_cases.py): losses 1e-4 relative, every gradient tensor 1e-4 of its maximum -- the project's fp32 bar of the fused step
(tests/test_gpu_fused.py: test_fused_step_vs_oracle).  tests/test_train_generic_cpu.py shows that float32 numpy on the same inputs needs less
than a tenth of them (a third at the loops batch).  The optimizer update is held per element to tests/adam_bounds.py.
Every test prints its worst figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import train_generic_cases as tc

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
synth = importlib.import_module("disentangled-vae_amd.synth")

DEV = "cuda:0"
LR = 1e-4


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the shared inputs are read-only)


def _trainer(case, B, **kw):
    params = tc.inputs(case, B)[0] if "params" not in kw else kw.pop("params")
    return T.make_trainer(tc.model_of(case), tc.dims_of(case), generic=True, params=params, batch=B, device=DEV, **kw)


def _batch(case, B):
    _, x, y, eps = tc.inputs(case, B)
    return _dev(x), _dev(y), _dev(eps)


def _check_step(case, B, tr, losses, what):
    l64, g64, _ = tc.truth(case, B)
    le = tc.loss_err(losses, l64[0])
    ge, name = tc.grad_err(tr.grads_numpy(), g64[0])
    print(f"{what} {tc.case_id(case)} B {B}: losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= tc.LOSS_RTOL and ge <= tc.GRAD_TOL, (le, ge, name)


@pytest.mark.parametrize("B", tc.BATCHES)
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_one_step_against_float64(case, B):
    tr = _trainer(case, B, lr=LR)
    assert isinstance(tr, G.GenericTrainer)
    p0 = tr.state_dict_numpy()
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    _check_step(case, B, tr, losses, "one step")
    p1 = tr.state_dict_numpy()
    for k in p0:
        assert np.all(np.isfinite(p1[k])) and np.max(np.abs(p1[k].astype(np.float64) - p0[k])) <= 1.05 * LR, k


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
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
    print(f"adam {tc.case_id(case)}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_three_steps_follow_the_float64_trajectory(case):
    B = tc.B_TRAJ
    l64, _, _ = tc.truth(case, B, tc.STEPS_TRAJ, tc.LR_TRAJ)
    tr = _trainer(case, B, lr=tc.LR_TRAJ)
    batch = _batch(case, B)
    errs = []
    for s in range(tc.STEPS_TRAJ):
        errs.append(tc.loss_err(tr.step(*batch).cpu().numpy(), l64[s]))
    print(f"trajectory {tc.case_id(case)}: loss errors {['%.2e' % e for e in errs]}")
    assert max(errs) <= tc.LOSS_RTOL


def test_loops_tiles_beyond_the_grid_and_a_short_last_slice():
    case = tc.LOOPS_CASE
    B, p = tc.loops_batch(lambda B: G.make_plan(tc.model_of(case), tc.dims_of(case), B))
    tr = _trainer(case, B, lr=LR)
    assert tr.plan.rows_grid < -(-B // 16) and tr.plan.ksplit >= 2 and 0 < B - (tr.plan.ksplit - 1) * tr.plan.slice_frames < tr.plan.slice_frames
    batch = _batch(case, B)
    losses = tr.step(*batch).cpu().numpy()
    _check_step(case, B, tr, losses, f"loops ({tr.plan.rows_grid} workgroups, {tr.plan.ksplit} slices of {tr.plan.slice_frames})")
    one = _trainer(case, B, lr=LR, ksplit=1)
    assert one.plan.ksplit == 1
    _check_step(case, B, one, one.step(*batch).cpu().numpy(), "loops, one slice")


@pytest.mark.parametrize("case,ksplit", [((3, 17, (129, 127)), 4), ((0, 32, (256, 64)), 0)], ids=["y3_ks4", "y0"])
def test_determinism(case, ksplit):
    B = 50
    batch = _batch(case, B)
    runs = []
    for _ in range(2):
        tr = _trainer(case, B, lr=tc.LR_TRAJ, ksplit=ksplit)
        rec = []
        for _ in range(2):
            rec.append(tr.step(*batch).cpu().numpy().copy())
            rec += list(tr.grads_numpy().values())
        runs.append(rec + list(tr.state_dict_numpy().values()))
    assert tr.plan.ksplit == (ksplit or 1)
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    one = _trainer(case, B, lr=LR, ksplit=1)
    _check_step(case, B, one, one.step(*batch).cpu().numpy(), "one slice")
    split = _trainer(case, B, lr=LR, ksplit=ksplit)
    _check_step(case, B, split, split.step(*batch).cpu().numpy(), f"{split.plan.ksplit} slices")


def _state(tr):
    return [tr.losses.cpu().numpy().copy()] + list(tr.grads_numpy().values()) + list(tr.state_dict_numpy().values())


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_gather():
    case, B, n = (3, 17, (129, 127)), 50, 70
    _, x, y, eps = tc.inputs(case, 100)
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
    bad[9] = -1
    a.evaluate(store_x, store_y, eps, rows=bad)
    assert a.bad_row_count() == 2


def test_evaluate_and_fork():
    case, B = (1, 5, (48, 200)), 50
    tr = _trainer(case, B, lr=tc.LR_TRAJ)
    batch = _batch(case, B)
    tr.step(*batch)                                          # moments are not zero from here on
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    tr.accumulate_losses(acc)
    ev = tr.evaluate(*batch).cpu().numpy()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.m, tr.v)))
    st = tr.step(*batch).cpu().numpy().copy()
    tr.accumulate_losses(None)
    assert np.array_equal(ev.view(np.uint32), st.view(np.uint32)), (ev, st)
    np.testing.assert_allclose(acc.cpu().numpy()[:3], 2.0 * st.astype(np.float64), rtol=1e-12)
    # a fork shares parameters and moments and sees the parent's update
    f = tr.fork(17)
    assert f.params.data_ptr() == tr.params.data_ptr() and f.m.data_ptr() == tr.m.data_ptr() and f.B == 17
    small = tuple(None if t is None else t[:17].contiguous() for t in batch)
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
    for case in [(7, 16, (128, 128)), (0, 32, (256, 64))]:
        model, dims = tc.model_of(case), tc.dims_of(case)
        module = synth.build_model(model, dims)
        tr = T.make_trainer(model, dims, batch=8, device=DEV, seed=5)
        assert isinstance(tr, G.GenericTrainer)
        sd = tr.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
        torch.manual_seed(5)                                 # the seeded init is the drop-in module's
        twin = synth.build_model(model, dims)
        assert all(torch.equal(sd[k].cpu(), v) for k, v in twin.state_dict().items())
        module.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
        tr.load_state_dict(module.state_dict(), strict=True)
        with pytest.raises(KeyError):
            tr.load_state_dict({"encoder.hidden.0.bias": sd["encoder.hidden.0.bias"]})
        tr.load_state_dict({"encoder.hidden.0.bias": sd["encoder.hidden.0.bias"] + 1}, strict=False)
        assert torch.equal(tr.state_dict()["encoder.hidden.0.bias"], sd["encoder.hidden.0.bias"] + 1)
        x, y, eps = (_dev(a) for a in synth.make_batch(dims, 8, 1))
        a = tr.step(x, y).cpu().numpy().copy()               # noise drawn on the device from (seed, step)
        assert np.all(np.isfinite(a)) and tuple(tr.noise(1).shape) == (8, case[1]) and torch.equal(tr.noise(1), tr.noise(1))
        assert tr.losses_host().shape == (3,)
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    assert type(T.make_trainer("M2", ref, batch=8, device=DEV)) is T.Trainer
    assert isinstance(T.make_trainer("M2", ref, batch=8, device=DEV, generic=True), G.GenericTrainer)
    with pytest.raises(NotImplementedError):
        T.Trainer("M2", dict(ref, y_dim=7), batch=8, device=DEV)
    with pytest.raises(NotImplementedError, match="reference geometry only"):
        G.GenericTrainer("M2_info", ref, batch=8, device=DEV)
    with pytest.raises(NotImplementedError, match="reference geometry only"):
        G.GenericTrainer("M2", ref, batch=8, device=DEV, precision="bf16")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        G.GenericTrainer("M2", ref, batch=8, device=DEV, world=2)
    with pytest.raises(NotImplementedError):
        T.make_trainer("M2_info", ref, batch=8, device=DEV, generic=True)
    with pytest.raises(NotImplementedError):
        T.make_trainer("M2", dict(ref, y_dim=7), batch=8, device=DEV, precision="bf16x3")

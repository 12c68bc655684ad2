"""The generic fused train step with a standardised encoder input (GenericTrainer(..., std_norm=(mean, std)); csrc/train_generic.hip,
the NORM instantiation of the rows kernel) against the float64 truth of tests/std_norm_cases.py: the scripts' loop body
`model((x - mean) / (std + eps), y)` scored by `elbo(x, r, ...)` against the raw x.

Bars (tests/train_generic_cases.py): losses 1e-4 relative, every gradient tensor 1e-4 of its maximum; tests/test_std_norm_cpu.py shows
that float32 numpy on the same inputs needs less than a tenth of them.  encoder.hidden.0.weight -- the one tensor whose operand is read
from the new stash block -- is also held per input column to the bound of tests/grad_columns.py.  Every test prints its worst figures
before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import grad_columns as gcol
import std_norm_cases as sc
import train_generic_cases as tc

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")
TC = importlib.import_module("disentangled-vae_amd.trainer_classifier")
A = importlib.import_module("disentangled-vae_amd.accumulate")

DEV = "cuda:0"
LR = 1e-4


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _trainer(case, B, std_norm="pool", **kw):
    params = tc.inputs(case, B)[0] if "params" not in kw else kw.pop("params")
    if std_norm == "pool":
        std_norm = sc.stats(case)
    return T.make_trainer(tc.model_of(case), tc.dims_of(case), generic=True, params=params, batch=B, device=DEV, std_norm=std_norm,
                          norm_eps=sc.NORM_EPS, **kw)


def _batch(case, B):
    _, x, y, eps = tc.inputs(case, B)
    return _dev(x), _dev(y), _dev(eps)


def _errs(case, B, tr, losses):
    l64, g64, _ = sc.truth(case, B)
    return tc.loss_err(losses, l64[0]), tc.grad_err(tr.grads_numpy(), g64[0])


def _check_step(case, B, tr, losses, what):
    le, (ge, name) = _errs(case, B, tr, losses)
    print(f"{what} {tc.case_id(case)} B {B}: losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= sc.LOSS_RTOL and ge <= sc.GRAD_TOL, (le, ge, name)


def _state(tr):
    return [tr.losses.cpu().numpy().copy()] + list(tr.grads_numpy().values()) + list(tr.state_dict_numpy().values()) + \
        [tr.m.cpu().numpy(), tr.v.cpu().numpy()]


def _same(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize("B", sc.BATCHES)
@pytest.mark.parametrize("case", sc.CASES, ids=tc.case_id)
def test_one_step_against_float64(case, B):
    tr = _trainer(case, B, lr=LR)
    assert isinstance(tr, G.GenericTrainer) and tr.plan.std_norm == 1
    p0 = tr.state_dict_numpy()
    losses = tr.step(*_batch(case, B)).cpu().numpy()
    _check_step(case, B, tr, losses, "one step")
    p1 = tr.state_dict_numpy()
    for k in p0:
        assert np.all(np.isfinite(p1[k])) and np.max(np.abs(p1[k].astype(np.float64) - p0[k])) <= 1.05 * LR, k
    assert list(tr.state_dict()) == list(T.TENSOR_NAMES)                            # the reference's keys only
    mean, std = tr.std_norm
    assert np.array_equal(mean.cpu().numpy(), sc.stats(case)[0]) and np.array_equal(std.cpu().numpy(), sc.stats(case)[1])


@pytest.mark.parametrize("case", [(3, 17, (129, 127)), (0, 32, (256, 64))], ids=tc.case_id)
def test_the_plain_step_misses_this_truth(case):
    """The same inputs through the trainer without std_norm are off by more than the bar: the test sees the feature."""
    B = 50
    plain = T.make_trainer(tc.model_of(case), tc.dims_of(case), generic=True, params=tc.inputs(case, B)[0], batch=B, device=DEV, lr=LR)
    assert plain.std_norm is None and plain.plan.std_norm == 0
    le, (ge, name) = _errs(case, B, plain, plain.step(*_batch(case, B)).cpu().numpy())
    print(f"plain step against the std_norm truth {tc.case_id(case)}: losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le > sc.LOSS_RTOL and ge > sc.GRAD_TOL


@pytest.mark.parametrize("case", [(1, 5, (48, 200)), (513, 128, (512, 512)), (0, 1, (1, 1))], ids=tc.case_id)
def test_three_steps_follow_the_float64_trajectory(case):
    B = sc.B_TRAJ
    l64, _, _ = sc.truth(case, B, sc.STEPS_TRAJ, sc.LR_TRAJ)
    tr = _trainer(case, B, lr=sc.LR_TRAJ)
    batch = _batch(case, B)
    errs = [tc.loss_err(tr.step(*batch).cpu().numpy(), l64[s]) for s in range(sc.STEPS_TRAJ)]
    print(f"trajectory {tc.case_id(case)}: loss errors {['%.2e' % e for e in errs]}")
    assert max(errs) <= sc.LOSS_RTOL


def test_loops_tiles_beyond_the_grid_and_a_short_last_slice():
    case = sc.LOOPS_CASE
    B, _ = tc.loops_batch(lambda B: G.make_plan(tc.model_of(case), tc.dims_of(case), B, std_norm=True))
    tr = _trainer(case, B, lr=LR)
    assert tr.plan.rows_grid < -(-B // 16) and tr.plan.ksplit >= 2 and 0 < B - (tr.plan.ksplit - 1) * tr.plan.slice_frames < tr.plan.slice_frames
    batch = _batch(case, B)
    _check_step(case, B, tr, tr.step(*batch).cpu().numpy(), f"loops ({tr.plan.rows_grid} workgroups, {tr.plan.ksplit} slices of {tr.plan.slice_frames})")
    one = _trainer(case, B, lr=LR, ksplit=1)
    assert one.plan.ksplit == 1
    _check_step(case, B, one, one.step(*batch).cpu().numpy(), "loops, one slice")


def test_gather_gives_the_bits_of_the_contiguous_call():
    case, B, n = (3, 17, (129, 127)), 50, 70
    _, x, y, eps = tc.inputs(case, 100)
    big_x, big_y, eps = _dev(x), _dev(y), _dev(eps[:B])
    store_x, store_y = big_x[:n], big_y[:n]
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
    assert a.bad_row_count() == 1 and b.bad_row_count() == 0 and _same(_state(a), _state(b))


def test_evaluate_and_fork():
    case, B = (1, 5, (48, 200)), 50
    tr = _trainer(case, B, lr=sc.LR_TRAJ)
    batch = _batch(case, B)
    tr.step(*batch)
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    ev = tr.evaluate(*batch).cpu().numpy()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.m, tr.v)))
    st = tr.step(*batch).cpu().numpy().copy()
    assert np.array_equal(ev.view(np.uint32), st.view(np.uint32)), (ev, st)         # evaluate(): the step's loss bits on the same parameters
    l64 = sc.truth(case, B, 2, sc.LR_TRAJ)[0]
    assert tc.loss_err(st, l64[1]) <= sc.LOSS_RTOL
    f = tr.fork(17)                                                                  # a fork carries the tables
    assert f.plan.std_norm == 1 and f.std_norm[0].data_ptr() == tr.std_norm[0].data_ptr() and f.params.data_ptr() == tr.params.data_ptr()
    small = tuple(None if t is None else t[:17].contiguous() for t in batch)
    l1 = f.evaluate(*small).cpu().numpy()
    fresh = _trainer(case, 17, params=tr.state_dict_numpy())
    l2 = fresh.evaluate(*small).cpu().numpy()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    fs = f.step(*small).cpu().numpy()
    assert np.array_equal(fs.view(np.uint32), l1.view(np.uint32)) and tr.step_count == 3


def test_two_micro_batches_equal_one_step_bit_for_bit():
    """AccumulatedStep over two micro-batches of 48 against one step of 96 with two slices: gradient, parameters and moments."""
    case, BM = (1, 5, (48, 200)), 48
    batch = _batch(case, 2 * BM)
    big = _trainer(case, 2 * BM, ksplit=2, params=tc.inputs(case, 2 * BM)[0])
    assert big.plan.ksplit == 2 and big.plan.slice_frames == BM
    tr = _trainer(case, BM, ksplit=1, params=tc.inputs(case, 2 * BM)[0])
    acc = A.AccumulatedStep(tr, micro_batches=[BM, BM])
    for s in range(2):
        big.step(*batch)
        gb = big.grads_numpy()
        for k in range(2):
            acc.micro(*(None if a is None else a[k * BM:(k + 1) * BM] for a in batch))
        ga = acc.grads_numpy()
        acc.apply()
        for k in gb:
            assert np.array_equal(np.asarray(ga[k], np.float32).view(np.uint32), gb[k].view(np.uint32)), (s, k)
    assert _same(_state(big)[len(gb) + 1:], _state(tr)[len(gb) + 1:])


def test_clipped_step():
    """max_norm: +inf gives the plain step's bits; a small norm scales the update."""
    case, B = (3, 17, (129, 127)), 50
    batch = _batch(case, B)
    a, b = _trainer(case, B), _trainer(case, B)
    a.step(*batch)
    b.step(*batch, max_norm=float("inf"))
    sa, sb = _state(a), _state(b)
    n = len(a.names)
    assert _same(sa[1 + n:], sb[1 + n:]) and np.array_equal(sa[0], sb[0])
    c = _trainer(case, B)
    c.step(*batch, max_norm=1e-3)
    norm, coef = c.grad_norm.cpu().numpy()
    g64 = sc.truth(case, B)[1][0]
    want = np.sqrt(sum(float(np.sum(v * v)) for v in g64.values()))
    print(f"clipped: total norm {norm:.6e} (float64 {want:.6e}), coef {coef:.3e}")
    assert abs(norm - want) <= 1e-4 * want and coef < 1 and c.skipped_step_count() == 0


@pytest.mark.parametrize("case,ksplit", [((3, 17, (129, 127)), 4), ((0, 32, (256, 64)), 0)], ids=["y3_ks4", "y0"])
def test_determinism(case, ksplit):
    B = 50
    batch = _batch(case, B)
    runs = []
    for _ in range(2):
        tr = _trainer(case, B, lr=sc.LR_TRAJ, ksplit=ksplit)
        rec = []
        for _ in range(2):
            tr.step(*batch)
            rec += _state(tr)
        runs.append(rec)
    assert _same(*runs)


@pytest.mark.parametrize("case", [(3, 17, (129, 127)), (0, 32, (256, 64)), (513, 128, (512, 512))], ids=tc.case_id)
def test_identity_statistics_give_the_plain_step(case):
    """mean 0, std 1: div = fl32(1 + 1e-8) = 1 and xn == x, so the forward pass, and with it the losses, are the plain step's bit for
    bit.  The gradients are reported: encoder layer 1's comes from the stash block in the place of x, the same numbers in the same
    order."""
    B = 50
    batch = _batch(case, B)
    plain = T.make_trainer(tc.model_of(case), tc.dims_of(case), generic=True, params=tc.inputs(case, B)[0], batch=B, device=DEV)
    ident = _trainer(case, B, std_norm=(np.zeros(513, np.float32), np.ones(513, np.float32)))
    lp, li = plain.step(*batch).cpu().numpy(), ident.step(*batch).cpu().numpy()
    gp, gi = plain.grads_numpy(), ident.grads_numpy()
    same = [k for k in gp if np.array_equal(gp[k].view(np.uint32), gi[k].view(np.uint32))]
    print(f"identity statistics {tc.case_id(case)}: losses {lp} / {li}; gradient tensors equal bit for bit: {len(same)} of {len(gp)}"
          + ("" if len(same) == len(gp) else f" (not: {[k for k in gp if k not in same]})"))
    assert np.array_equal(lp.view(np.uint32), li.view(np.uint32))
    ev_p, ev_i = plain.evaluate(*batch).cpu().numpy(), ident.evaluate(*batch).cpu().numpy()
    print(f"  after the update: evaluate() {ev_p} / {ev_i}")


def test_adam_per_element():
    case, B = (3, 17, (129, 127)), 50
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


@pytest.mark.parametrize("case,B,ksplit", sc.COLUMN_CASES, ids=lambda v: tc.case_id(v) if isinstance(v, tuple) else str(v))
def test_encoder_layer_1_weight_gradient_per_input_column(case, B, ksplit):
    (bw, bm), G64 = sc.column_bound(case, B, ksplit)
    tr = _trainer(case, B, ksplit=ksplit)
    assert tr.plan.ksplit == ksplit
    x, y, eps = _batch(case, B)
    tr.grads_only(x, y, eps)
    f = gcol.column_figures(tr.grads_numpy()[sc.COLUMN_TENSOR], G64)
    print(f"{sc.COLUMN_TENSOR} {tc.case_id(case)} B {B} ksplit {ksplit}: worst column {f['worst']:.2e} ({f['worst'] / bw:.2f} of bound) at "
          f"{f['arg']}, median {f['median']:.2e} ({f['median'] / bm:.2f}), tensor-level {f['tensor']:.1e}")
    assert f["zero_ok"] and f["worst"] <= bw and f["median"] <= bm, f


def test_refusals_and_kinds():
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    good = (np.zeros(513), np.ones(513))
    assert T.trainer_kind("M2", ref, std_norm=True) == "generic" and T.trainer_kind("M2", ref) == "resident"
    tr = T.make_trainer("M2", ref, batch=8, device=DEV, std_norm=good)               # the reference geometry goes to the generic step
    assert isinstance(tr, G.GenericTrainer) and tr.plan.std_norm == 1
    tr = T.make_trainer("M2", ref, batch=8, device=DEV, std_norm=(torch.zeros(513, device=DEV), torch.ones(513, 1, device=DEV)))
    assert tr.std_norm[1].shape == (513,)
    with pytest.raises(ValueError):
        T.make_trainer("M2", ref, batch=8, device=DEV, std_norm=(np.zeros(513), np.full(513, np.nan)))
    with pytest.raises(NotImplementedError, match="std_norm"):
        TI.make_info_trainer(ref, batch=8, device=DEV, std_norm=good)
    with pytest.raises(NotImplementedError, match="std_norm"):
        TI.InfoTrainer(ref, batch=8, device=DEV, std_norm=good)
    with pytest.raises(NotImplementedError, match="std_norm"):
        TC.ClassifierTrainer(dict(x_dim=513, y_dim=1, h_dim=(128, 128)), batch=8, device=DEV, std_norm=good)
    with pytest.raises(NotImplementedError):
        T.make_trainer("M2_info", ref, batch=8, device=DEV, std_norm=good)

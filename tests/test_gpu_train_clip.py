"""Global-norm clipping on the device in the any-size fused train steps (csrc/train_tables.hip: train_generic_gradnorm_kernel,
train_generic_apply_clipped_kernel; include/dvae_train.h: dvae_train_*_apply_flat_clipped; disentangled-vae_amd/clip.py, accumulate.py).
Truth: tests/clip_ref.py (held against torch in tests/test_train_clip_cpu.py); update bounds: tests/adam_bounds.py.

One geometry per trainer kind at 50 frames (three tiles and a ragged fourth; 35 072, 73 152 and 276 288 floats: 9, 18 and 68 chunks of
the norm launch, the last one ragged) and the M1 (0, 1, (1, 1)) whose 2432 floats are less than one chunk.  On an MI355X: total_norm
and coef within 3.8e-8 of float64, the clipped update within 0.50 of the Adam bounds, every bit-for-bit comparison without a differing
element.
 1. grad_norm = [total_norm, coef] against float64 on the read-back flat gradient: 2^-22 relative -- double accumulation over at most
    2^22 terms costs below 2^-30; what remains is the one rounding to float32 of each output plus slack for sqrt.
 2. the update at max_norm = 0.1 total_norm, per element within adam_bounds.bounds(grad_scale=gscale_eff) of the restatement; the
    packed copies follow: evaluate equals that of a fresh trainer loaded from state_dict.
 3. max_norm = inf and 10 total_norm: bit-identical to a twin's plain apply() / step().
 4. two runs give the same bits; two equal micro-batches + a clipped apply == one step(max_norm=) of twice the frames, bit for bit
    (the power-of-two rule of DESIGN 4a'''': the accumulator is exactly twice the big step's gradient, so s is exactly four times,
    total_norm, coef and the product with the gradient come out equal).
 5. an inf / a NaN in the flat gradient: nothing is written, the step is counted as skipped, the next clipped step updates normally.
 6. two ranks sharing the GPU over gloo, three clipped steps: replicas equal, grad_norm equal, == one trainer of the whole batch.
Every comparison prints its figures before it asserts."""
import functools
import importlib
import math
import os

import numpy as np
import pytest
import torch

import adam_bounds as ab
import clip_ref
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic

pytestmark = pytest.mark.gpu
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")

DEV = "cuda:0"
LR = 1e-4
ADAM = (LR, 0.9, 0.999, 1e-8)            # the trainers' defaults
B = 50
BM = 48                                  # three whole tiles: the micro-batch of the bit-for-bit comparisons
BAR = 2.0 ** -22
CASES = [("generic", (1, 5, (48, 200))), ("generic", (0, 1, (1, 1))), ("clf", ((48, 200), 2)), ("info", (3, 17, (129, 127)))]
KIND_CASES = [CASES[0], CASES[2], CASES[3]]              # one per trainer kind
MODS = {"generic": gc, "clf": cc, "info": ic}


def _id(kc):
    return f"{kc[0]}-{MODS[kc[0]].case_id(kc[1])}"


def _make(mods, kind, case, batch, ksplit, **kw):
    """mods = (G, C, I, gc, cc, ic): the two-rank workers import their own."""
    Gm, Cm, Im, gcm, ccm, icm = mods
    if kind == "generic":
        return Gm.GenericTrainer(gcm.model_of(case), gcm.dims_of(case), gcm.inputs(case, 1)[0], batch=batch, device=DEV, lr=LR, ksplit=ksplit, **kw)
    if kind == "clf":
        return Cm.ClassifierTrainer(ccm.dims_of(case), params=ccm.params_of(case), batch=batch, device=DEV, lr=LR, ksplit=ksplit, **kw)
    a, b, g = icm.WEIGHTS
    return Im.InfoTrainer(icm.dims_of(case), params=icm.params_of(case), batch=batch, device=DEV, lr=LR, alpha=a, beta=b, gamma=g, ksplit=ksplit, **kw)


def _trainer(kind, case, batch=B, ksplit=0):
    return _make((G, C, I, gc, cc, ic), kind, case, batch, ksplit)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _batch(kind, case, n=B):
    """The n frames of the cases module on the device: (x, y[, eps]); never written."""
    return tuple(_dev(a) for a in MODS[kind].inputs(case, n)[1:])


def _rows(batch, lo, hi):
    return tuple(None if a is None else a[lo:hi] for a in batch)


def _tensor_index(tr):
    """The flat indices that belong to a tensor, in tensor order."""
    n = len(tr.names)
    return np.concatenate([np.arange(tr.plan.tensor_offset[i], tr.plan.tensor_offset[i] + tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i])
                           for i in range(n)])


def _pmv(tr):
    return tuple(t.cpu().numpy().copy() for t in (tr.params, tr.m, tr.v))


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_same_pmv(got, want, what):
    for part, g, w in zip("pmv", got, want):
        assert _same(g, w), (what, part, f"{np.count_nonzero(g.view(np.uint32) != w.view(np.uint32))} of {g.size} elements differ")


@functools.lru_cache(maxsize=None)
def _norm_of(kind, case, n=B):
    """float64 norm of the gradient of the mean loss over the n frames, from the read-back flat gradient of one micro-batch."""
    tr = _trainer(kind, case, n)
    acc = A.AccumulatedStep(tr)
    acc.micro(*_batch(kind, case, n))
    return math.sqrt(clip_ref.sum_squares([acc.flat.cpu().numpy()[_tensor_index(tr)]]))


def _evaluate(tr, kind, case):
    return tr.evaluate(*_batch(kind, case)).cpu().numpy().copy()


def _clipped_run(kind, case, factor=0.1):
    """Step 1 plain (moments become non-zero), step 2 clipped at max_norm = factor * total_norm of its own gradient.  Everything a
    test needs of step 2: inputs, outputs, grad_norm, the evaluate after it."""
    tr = _trainer(kind, case)
    acc = A.AccumulatedStep(tr)
    batch = _batch(kind, case)
    acc.micro(*batch)
    acc.apply()
    acc.micro(*batch)
    idx = _tensor_index(tr)
    flat = acc.flat.cpu().numpy().copy()
    before = _pmv(tr)
    gs = acc._grad_scale(acc._pending)
    max_norm = factor * gs * math.sqrt(clip_ref.sum_squares([flat[idx]]))
    acc.apply(max_norm=max_norm)
    assert tr.step_count == 2 and np.array_equal(acc.flat.cpu().numpy(), flat)          # the accumulator is left alone
    return dict(tr=tr, idx=idx, flat=flat, gs=gs, max_norm=max_norm, before=before, after=_pmv(tr), grad_norm=acc.grad_norm.cpu().numpy().copy(),
                skipped=acc.skipped_step_count(), evaluate=_evaluate(tr, kind, case))


_clipped_once = functools.lru_cache(maxsize=None)(_clipped_run)


# ---- 1: norm and coefficient ----
@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_grad_norm_and_coefficient_against_float64(kc):
    r = _clipped_once(*kc)
    info = clip_ref.clip_scale([r["flat"][r["idx"]]], r["gs"], r["max_norm"])
    gn = r["grad_norm"].astype(np.float64)
    en, ec = abs(gn[0] - info["total_norm"]) / info["total_norm"], abs(gn[1] - info["coef"]) / info["coef"]
    chunks = (r["flat"].size + 4095) // 4096
    print(f"{_id(kc)}: {r['flat'].size} floats = {chunks} chunk(s); total_norm {gn[0]:.6e} off by {en:.2e}, coef {gn[1]:.6e} off by {ec:.2e} (bar {BAR:.2e})")
    assert r["flat"].dtype == np.float32 and gn.shape == (2,) and r["skipped"] == 0
    assert (chunks == 1) == (kc[1] == (0, 1, (1, 1))) and (chunks == 1 or r["flat"].size % 4096 != 0)       # the premise: one chunk; many and a ragged last
    assert en <= BAR and ec <= BAR
    assert 0.09 < info["coef"] < 0.11


# ---- 2: the update ----
@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_clipped_update_within_the_adam_bounds_and_copies_follow(kc):
    kind, case = kc
    r = _clipped_once(*kc)
    idx = r["idx"]
    p0, m0, v0 = (a[idx] for a in r["before"])
    Gf = r["flat"][idx]
    hyper = (2,) + ADAM
    info = clip_ref.clip_scale([Gf], r["gs"], r["max_norm"])
    want = clip_ref.clipped_step([p0], [m0], [v0], [Gf], hyper, r["gs"], r["max_norm"])
    bounds = ab.bounds(p0, m0, v0, Gf, hyper, grad_scale=info["gscale_eff"])
    worst = {}
    for part, got, w, b in zip("pmv", r["after"], want[:3], bounds):
        worst[part] = float(np.max(ab.ratios(got[idx], w[0], b)))
    moved = float(np.max(np.abs(r["after"][0][idx].astype(np.float64) - p0)))
    print(f"{_id(kc)}: gscale_eff {info['gscale_eff']:.8e}; worst |error| / bound: p {worst['p']:.3f}, m {worst['m']:.3f}, v {worst['v']:.3f}; "
          f"largest parameter move {moved / LR:.3f} lr")
    assert max(worst.values()) <= 1.0, worst
    assert moved > 0.0
    gaps = np.ones(r["flat"].size, bool)
    gaps[idx] = False
    for a, b in zip(r["after"], r["before"]):                  # floats that belong to no tensor are not touched
        assert _same(a[gaps], b[gaps])
    fresh = _trainer(kind, case)
    fresh.load_state_dict(r["tr"].state_dict())
    assert np.array_equal(_evaluate(fresh, kind, case), r["evaluate"]), (r["evaluate"], "the packed copies do not hold the updated parameters")


# ---- 3: thresholds that clip nothing ----
@pytest.mark.parametrize("path", ["apply", "step"])
@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_thresholds_that_clip_nothing_leave_the_unclipped_bits(kc, path):
    kind, case = kc
    batch = _batch(kind, case)
    big = 10.0 * _norm_of(kind, case)

    def run(max_norm):
        tr = _trainer(kind, case)
        acc = A.AccumulatedStep(tr)
        coefs = []
        for _ in range(2):
            if path == "apply":
                acc.micro(*batch)
                acc.apply() if max_norm is None else acc.apply(max_norm=max_norm)
            else:
                tr.step(*batch) if max_norm is None else tr.step(*batch, max_norm=max_norm)
            if max_norm is not None:
                coefs.append(tr.grad_norm.cpu().numpy().copy())
        return _pmv(tr), tr.losses.cpu().numpy().copy(), coefs
    plain, plain_losses, _ = run(None)
    for max_norm in (math.inf, big):
        got, losses, gn = run(max_norm)
        print(f"{_id(kc)} {path}(max_norm={max_norm:.4g}): [total_norm, coef] of the two steps {[g.tolist() for g in gn]}")
        _assert_same_pmv(got, plain, f"{_id(kc)} {path} max_norm {max_norm}")
        assert np.array_equal(losses, plain_losses)
        assert all(g[1] == 1.0 and 0.0 < g[0] < big for g in gn)


# ---- 4: determinism ----
@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_two_clipped_runs_give_the_same_bits(kc):
    a, b = _clipped_once(*kc), _clipped_run(*kc)
    _assert_same_pmv(b["after"], a["after"], _id(kc))
    assert _same(a["grad_norm"], b["grad_norm"]) and np.array_equal(a["evaluate"], b["evaluate"])


@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_two_micro_batches_and_a_clipped_apply_equal_one_clipped_step_of_twice_the_frames(kc):
    kind, case = kc
    batch = _batch(kind, case, 2 * BM)
    max_norm = 0.1 * _norm_of(kind, case, 2 * BM)
    big = _trainer(kind, case, 2 * BM, 2)
    assert big.plan.ksplit == 2 and big.plan.slice_frames == BM          # the premise: slice k of the big step is micro-batch k
    tr = _trainer(kind, case, BM, 1)
    acc = A.AccumulatedStep(tr, micro_batches=[BM, BM])
    for s in range(2):
        big.step(*batch, max_norm=max_norm)
        for k in range(2):
            acc.micro(*_rows(batch, k * BM, (k + 1) * BM))
        acc.apply(max_norm=max_norm)
        gb, ga = big.grad_norm.cpu().numpy().copy(), acc.grad_norm.cpu().numpy().copy()
        print(f"{_id(kc)} step {s + 1}: [total_norm, coef] one step of {2 * BM} frames {gb.tolist()}, 2 x {BM} frames {ga.tolist()}")
        assert _same(ga, gb) and 0.0 < ga[1] < 0.5
    _assert_same_pmv(_pmv(tr), _pmv(big), _id(kc))
    assert big.skipped_step_count() == 0 and acc.skipped_step_count() == 0


# ---- 5: a gradient that is not finite ----
@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("kc", CASES, ids=_id)
def test_a_gradient_that_is_not_finite_skips_the_step(kc, bad):
    kind, case = kc
    batch = _batch(kind, case)
    max_norm = 0.1 * _norm_of(kind, case)
    tr = _trainer(kind, case)
    acc = A.AccumulatedStep(tr)
    acc.micro(*batch)
    acc.apply(max_norm=max_norm)                               # an ordinary clipped step: the moments are no longer zero
    before, ev = _pmv(tr), _evaluate(tr, kind, case)
    acc.micro(*batch)
    where = int(_tensor_index(tr)[-1])                         # the last float of the last tensor: the last, ragged chunk
    acc.flat[where] = bad
    acc.apply(max_norm=max_norm)
    gn = acc.grad_norm.cpu().numpy().copy()
    print(f"{_id(kc)}: flat[{where}] = {bad}: [total_norm, coef] {gn.tolist()}")
    _assert_same_pmv(_pmv(tr), before, f"{_id(kc)} skipped")
    assert np.array_equal(_evaluate(tr, kind, case), ev)
    assert gn[1] == 0.0 and (math.isnan(gn[0]) if math.isnan(bad) else gn[0] == math.inf)
    assert tr.step_count == 2                                  # the host cannot know: the skipped step still counts
    assert acc.skipped_step_count() == 1 and acc.skipped_step_count() == 0 and tr.skipped_step_count() == 0
    # the next ordinary clipped step: the update of step 3 on the untouched state
    acc.micro(*batch)
    idx = _tensor_index(tr)
    Gf = acc.flat.cpu().numpy()[idx]
    acc.apply(max_norm=max_norm)
    hyper = (3,) + ADAM
    info = clip_ref.clip_scale([Gf], 1.0, max_norm)
    want = clip_ref.clipped_step([before[0][idx]], [before[1][idx]], [before[2][idx]], [Gf], hyper, 1.0, max_norm)
    bounds = ab.bounds(before[0][idx], before[1][idx], before[2][idx], Gf, hyper, grad_scale=info["gscale_eff"])
    after = _pmv(tr)
    worst = max(float(np.max(ab.ratios(g[idx], w[0], b))) for g, w, b in zip(after, want[:3], bounds))
    gn = acc.grad_norm.cpu().numpy()
    print(f"{_id(kc)}: the step after the skipped one: coef {gn[1]:.4f}, worst |error| / bound {worst:.3f}")
    assert worst <= 1.0 and not _same(after[0], before[0]) and 0.0 < gn[1] < 1.0 and acc.skipped_step_count() == 0


# ---- 6: two ranks sharing the GPU over gloo ----
DP_STEPS = 3


def _worker(rank, world, port, max_norms, q):
    import sys, traceback
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    try:
        import torch.distributed as dist
        import train_classifier_cases as ccm, train_generic_cases as gcm, train_info_cases as icm
        mods = tuple(importlib.import_module("disentangled-vae_amd." + n) for n in ("trainer_generic", "trainer_classifier", "trainer_info")) \
            + (gcm, ccm, icm)
        Am = importlib.import_module("disentangled-vae_amd.accumulate")
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ.pop("DVAE_ALLREDUCE", None)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        out = {}
        for kind, case in KIND_CASES:
            tr = _make(mods, kind, case, BM, 1)
            acc = Am.AccumulatedStep(tr, dist.group.WORLD)
            all_ = {"generic": gcm, "clf": ccm, "info": icm}[kind].inputs(case, 2 * BM)[1:]
            mine = tuple(None if a is None else torch.from_numpy(np.array(a[BM * rank:BM * (rank + 1)])).to(DEV) for a in all_)
            norms = []
            for _ in range(DP_STEPS):
                acc.micro(*mine)
                acc.apply(max_norm=max_norms[kind])
                norms.append(acc.grad_norm.cpu().numpy().copy())
            out[kind] = dict(pmv=tuple(t.cpu().numpy() for t in (tr.params, tr.m, tr.v)), norms=norms, equal=acc.replicas_equal(),
                             skipped=acc.skipped_step_count())
        q.put((rank, out, None))
        dist.destroy_process_group()
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@functools.lru_cache(maxsize=None)
def _ranks():
    import torch.multiprocessing as mp
    max_norms = {kind: 0.1 * _norm_of(kind, case, 2 * BM) for kind, case in KIND_CASES}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37000 + (os.getpid() * 3 + 1) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, max_norms, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = []
    for _ in procs:
        got.append(q.get(timeout=300))
        if got[-1][2] is not None:
            for pr in procs:
                pr.kill()
            raise AssertionError(f"rank {got[-1][0]} failed:\n{got[-1][2]}")
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    got.sort(key=lambda t: t[0])
    return max_norms, got[0][1], got[1][1]


@pytest.mark.parametrize("kc", KIND_CASES, ids=_id)
def test_two_ranks_clip_alike_and_equal_one_trainer_of_the_whole_batch(kc):
    kind, case = kc
    max_norms, r0, r1 = _ranks()
    r0, r1 = r0[kind], r1[kind]
    one = _trainer(kind, case, 2 * BM, 2)
    assert one.plan.ksplit == 2 and one.plan.slice_frames == BM
    batch = _batch(kind, case, 2 * BM)
    norms = []
    for _ in range(DP_STEPS):
        one.step(*batch, max_norm=max_norms[kind])
        norms.append(one.grad_norm.cpu().numpy().copy())
    print(f"{_id(kc)}: [total_norm, coef] per step, one trainer {[n.tolist() for n in norms]}, rank 0 {[n.tolist() for n in r0['norms']]}")
    assert r0["equal"] is True and r1["equal"] is True and r0["skipped"] == 0 and r1["skipped"] == 0
    for s in range(DP_STEPS):
        assert _same(r0["norms"][s], r1["norms"][s]) and _same(r0["norms"][s], norms[s]), s
        assert 0.0 < norms[s][1] < 1.0                          # every step was clipped
    _assert_same_pmv(r0["pmv"], r1["pmv"], f"{_id(kc)} rank 0 against rank 1")
    _assert_same_pmv(r0["pmv"], _pmv(one), f"{_id(kc)} the ranks against one trainer")

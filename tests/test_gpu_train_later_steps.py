"""Steps two and three of the any-size train steps held to step one's bounds (tests/later_steps.py; tests/test_later_steps_cpu.py shows on
the CPU which faults the rest of the suite cannot see).
Every gradient check of the suite starts from a fresh trainer.  Here a trainer takes three steps at lr 1e-3 (a weight moves by 1 - 3 %),
another batch (BATCH_SEED + k; the ReLU nets' frames selected again at the parameters in force) and other hyper-parameters (SCHEDULE,
set on the trainer between steps) every step, with explicit noise.  Before step k the test reads state_dict_numpy(), m, v and
step_count; after it:
  A  grads_numpy() under grad_columns_generic.check against reference_at(the parameters read before the step, this step's batch):
     MARGIN 4, floor 2^-24, unchanged.  From step 2 on stale_ratio >= 100 is asserted as well: the float64 gradient at the PREVIOUS
     step's parameters on this batch against this step's reference -- the premise that a stale copy would be seen, from the oracle alone.
  B  the losses against the float64 oracle at those parameters under the cases module's LOSS_RTOL; the classifier's counts exactly.
  C  the update: adam_figures with hyper = (k, lr_k, b1_k, b2_k, eps_k) on the p, m, v read before, the device's own gradient and the
     p, m, v read after: at most 1 for each (SLACK 2).  Accumulated and clipped steps pass their grad_scale / gscale_eff.
  D  a fresh trainer built from the parameters read before the step, m, v and step_count copied in, takes the same step: losses,
     gradients, p, m, v equal bit for bit.  Its packed copies come from the repack path, not from a preceding apply launch.
One line per step is printed before anything is asserted.

Cases.  50 frames and one 1-frame case per kind: M2 (3, 17, (129, 127)) in one and in four slices, (513, 128, (512, 512)), (1, 5, (48, 200)),
M1 (0, 32, (256, 64)); the classifier ((129, 127), 17) and ((512, 512), 513); M2_info (3, 17, (129, 127)) in the default mode and fed by its
classifier with the entropy adversary; the generic step with std_norm.  Interleavings on one geometry per kind: a trainer and its fork
taking turns with an evaluate and a load_state_dict of one tensor between them; two AccumulatedSteps of 48 + 48 + 20 (the 20 on a
fork), then main.step, then tail.step; three clipped steps, and the same with a skipped one in the middle (p, m, v bit-equal, the step
counted, the next update held under C with the step number the trainer reports).  The reference-size trainer.Trainer: M2 y 513 at 33
frames and M1 at 1000 under fp32, bf16x3 and bf16, the update deferred or not -- A under grad_columns.check and the rule of the
precision, B under test_fused_step_vs_oracle's tolerance, D under fp32 (its update is held per step by tests/test_gpu_fused_apply.py).
The module path: three iterations with stock torch.optim.Adam(lr=1e-3), every iteration's loss / outputs and parameter gradients
against float64 at the module's own parameters -- the KL-weighted script loop on the generic engine, and a loss that is linear in the
outputs (the rule's "all" upstream set) on the resident engine (M2 y 1, 33 frames, bf16x3) and on the M2_info body.

MEASURED on the MI355X against the unmodified library: 41 tests, 16 s of wall time with the CPU references; the slowest test
1.4 s ((513, 128, (512, 512)): three references and three twins), every other under 0.6 s but the generic-engine loop (2.3 s, its first
call builds the engine).  Nothing failed: no bug found.  Worst ratio per kind at steps 1 / 2 / 3 -- a device that errs exactly as the
restatement does reaches 0.25 in A, an update that performs exactly the counted roundings about 0.5 in C:
                   A gradients          B losses               C update (worst of p, m, v)
  M1 / M2          0.43  0.47  0.43     0.002  0.001  0.001    0.49  0.49  0.50
  std_norm         0.43  0.37  0.42     0.001  0.000  0.001    0.46  0.49  0.50
  classifier       0.29  0.31  0.26     0.001  0.010  0.012    0.46  0.49  0.50     counts exact
  M2_info          0.56  0.37  0.70     0.41   0.17   0.02     0.50  0.49  0.50
  interleavings    0.68 (tail.step after two accumulated steps and a plain one)   0.21   0.50
  Trainer          0.31 ... 0.49 at steps 2 and 3 under every policy; losses 0.001 / 0.03 / 0.10 of 1e-4 / 1e-5 / 2e-3 (fp32 / bf16x3 / bf16)
  module engines   generic 0.33 (loss 0.01 of its bound), resident 0.32 (outputs 0.27), M2_info body 0.63 (outputs 0.30)
The highest A, 0.70, is M2_info (classifier, entropy) at step 3.  Every bit-for-bit twin holds, the deferred update included (where
DVAE_DEFER_APPLY is on, all three updates were deferred, and the state a fresh trainer leaves after update k is what step k + 1 ran on).
The smallest stale_ratio seen: 272 (tail.step on 20 frames after main.step), 387 at M2's one-frame step 2, 1.9e3 ... 2.9e5 elsewhere.

Scratch breakages, one at a time, nothing of them committed; each leaves every address inside its allocation.  This module and tests/test_gpu_train_generic.py,
tests/test_gpu_train_columns.py, tests/test_gpu_frames.py were RUN once against each:
  a  apply_body (csrc/train_tables.hip) skips the write of a tensor's transposed copy (d.t0) when g.adam is set
       this module: 23 of 41 fail, all at step 2 under A, 4.8e4 ... 1.9e5 column bounds (B and C pass: the forward copies are fresh).
       Of the 18 that pass, three are the fork interleavings (every step there follows another trainer's, so the copies are repacked whole);
       the other 15 -- the reference-size trainer, the module engines -- run none of the broken code.
       test_gpu_train_generic.py: 9 fail, all test_three_steps_follow_the_float64_trajectory -- its rate is 1e-2, not 1e-6, and at 1e-2
       two steps on a stale backward copy move the third loss past 1e-4 (tests/test_later_steps_cpu.py, 4).  It says "loss errors",
       not which state.  test_gpu_train_columns.py and test_gpu_frames.py: none.
  b  dvae_train_generic_step passes step - 1 to its apply launch (from step 2 on; step 0 would be refused by the argument check)
       this module: 10 of 41 fail -- every test that takes a plain GenericTrainer.step after step 1 -- at step 2 under C, p at 2.4e5
       Adam bounds, A and B passing.  test_gpu_train_generic.py: the same 9 trajectory tests.  columns, frames: none.
  c  GenericTrainer.step leaves _shared["version"] as it was, so a fork does not repack
       this module: 1 of 41 fails, test_a_trainer_and_its_fork_take_turns on the generic trainer, at fork.step 2 under A (1.0e5 column
       bounds) and B (5.4 LOSS_RTOL); the classifier's and M2_info's trainers have a step of their own and were not broken.  The
       accumulated interleaving passes: _apply_flat, which was left alone, had moved the version before.
       test_gpu_train_generic.py: test_evaluate_and_fork fails (its fork's forward losses).  columns, frames: none
       (test_gpu_frames.py forks the reference-size Trainer, another class).
So the trajectory tests of the M1 / M2 step, run at 1e-2, do notice (a) and (b) -- through three loss scalars, 1e-4 wide, and only
there: the classifier's run at 1e-2 too, M2_info's at 1e-6 (blind to a stale weight, tests/test_later_steps_cpu.py), accumulated,
clipped and deferred steps have none.  What this module adds is the size and the place: the same faults at 1e4 ... 1e5 bounds, named
by step, check and tensor, on every kind of step.
"""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import adam_bounds as ab
import clip_ref
import grad_columns_generic as gg
import later_steps as ls
import std_norm_cases as sn
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic

pytestmark = pytest.mark.gpu
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")
CLIP = importlib.import_module("disentangled-vae_amd.clip")

DEV = "cuda:0"
# (lr, betas, adam_eps) of steps 1, 2, 3, ...: set on the trainer before each step, as a schedule would (the trainers read them per step)
SCHEDULE = [(ls.LR, (0.9, 0.999), 1e-8), (2e-3, (0.8, 0.99), 1e-6), (5e-4, (0.95, 0.9999), 1e-7), (1e-3, (0.9, 0.999), 1e-8)]
_M2, _CLF, _INFO = (3, 17, (129, 127)), ((129, 127), 17), (3, 17, (129, 127))
ENTROPY = ("classifier", "entropy")
# (kind, case, mode, B, ksplit)
CASES = ([("generic", _M2, None, 50, 1), ("generic", _M2, None, 50, 4), ("generic", (513, 128, (512, 512)), None, 50, 1),
          ("generic", (1, 5, (48, 200)), None, 50, 1), ("generic", (0, 32, (256, 64)), None, 50, 1), ("generic", _M2, None, 1, 1),
          ("clf", _CLF, None, 50, 1), ("clf", ((512, 512), 513), None, 50, 1), ("clf", _CLF, None, 1, 1),
          ("info", _INFO, gg.DEFAULT_MODE, 50, 1), ("info", _INFO, ENTROPY, 50, 1), ("info", _INFO, gg.DEFAULT_MODE, 1, 1),
          ("norm", _M2, None, 50, 1), ("norm", _M2, None, 1, 1)])
KIND_CASES = [("generic", _M2, None), ("clf", _CLF, None), ("info", _INFO, gg.DEFAULT_MODE)]          # the interleavings: one geometry per kind
MICRO = gg.MICRO


def _id(c):
    return ls.case_label(*c, *((50,) if len(c) == 3 else ())).replace(" ", "-")


def _initial(kind, case):
    if kind == "clf":
        return cc.params_of(case)
    return ic.params_of(case) if kind == "info" else gc.inputs(case, 1)[0]


def _make(kind, case, mode, params, batch, ksplit=0):
    if kind in ("generic", "norm"):
        return G.GenericTrainer(gc.model_of(case), gc.dims_of(case), params, batch=batch, device=DEV, lr=ls.LR, ksplit=ksplit,
                                std_norm=sn.stats(case) if kind == "norm" else None)
    if kind == "clf":
        return C.ClassifierTrainer(cc.dims_of(case), params=params, batch=batch, device=DEV, lr=ls.LR, ksplit=ksplit)
    a, b, g = ic.WEIGHTS
    return I.InfoTrainer(ic.dims_of(case), params=params, batch=batch, device=DEV, lr=ls.LR, alpha=a, beta=b, gamma=g, ksplit=ksplit,
                         dec_label=mode[0], aux_enc=mode[1])


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _args(kind, x, y, e, lo=0, hi=None):
    """the positional arguments of step / evaluate / micro for frames lo:hi (the classifier takes no noise; M1 no labels)"""
    arrays = (x, y) if kind == "clf" else (x, y, e)
    return tuple(_dev(None if a is None else a[lo:hi]) for a in arrays)


def _index(tr):
    return np.concatenate([np.arange(tr.plan.tensor_offset[i], tr.plan.tensor_offset[i] + tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i])
                           for i in range(len(tr.names))])


def _state(tr):
    """what a step starts from (and ends on): the parameters per tensor, the flat p, m, v restricted to the tensors, the step number"""
    idx = _index(tr)
    return dict(params=tr.state_dict_numpy(), pmv=tuple(t.cpu().numpy()[idx] for t in (tr.params, tr.m, tr.v)), t=tr.step_count)


def _set(trainers, k):
    lr, betas, eps = SCHEDULE[k - 1]
    for tr in trainers:
        tr.lr, tr.betas, tr.adam_eps = lr, betas, eps
    return (lr, betas[0], betas[1], eps)


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(ab.same_bits(a, b).all())


class Held:
    """The checks A - C of one step, printed on one line before anything is asserted."""

    def __init__(self, kind, case, mode, tag):
        self.kind, self.case, self.mode, self.tag = kind, case, mode, tag
        self.prev = None                               # the parameters the previous update started from
        self.tops = []

    def step(self, before, after, batch, ksplit, grads, losses, flat, hyper_t, hyper, grad_scale=1.0, micro=None, counts=None, what="step",
             ref=None):
        """before / after: _state() around the update; batch: this step's float32 frames; grads: what grads_numpy() reports; flat: the
        float32 gradient the update read (before grad_scale), restricted to the tensors."""
        kind, case, mode = self.kind, self.case, self.mode
        if ref is None:
            ref = ls.reference_at(kind, case, mode, before["params"], *batch, ksplit, micro)
        fails, top_a = ls.check(grads, ref, quiet=True)
        stale = None
        if self.prev is not None:
            stale = ls.stale_ratio(ref, ls.oracle_step(kind, case, mode, self.prev, *batch)[1])
        l64, _, c64 = ls.oracle_step(kind, case, mode, before["params"], *batch)
        top_b = ls.loss_err(kind, mode, losses, l64) / ls.loss_rtol(kind)
        fig = ls.adam_figures(*before["pmv"], flat, *after["pmv"], (hyper_t,) + tuple(hyper), grad_scale)
        print(f"[{self.tag}] {what} {hyper_t} on {batch[0].shape[0]} frames: A gradients {top_a:.3f} of the column bound, B losses {top_b:.3f} of "
              f"LOSS_RTOL, C update p {fig['p']:.3f} m {fig['m']:.3f} v {fig['v']:.3f} of the Adam bounds"
              + ("" if stale is None else f"; stale_ratio {stale:.3g}"))
        self.tops.append((top_a, top_b, max(fig.values()), stale))
        assert after["t"] == hyper_t
        assert stale is None or stale >= ls.STALE_MIN, f"the premise fails: a gradient on the previous parameters is only {stale} bounds away"
        assert not fails, fails
        assert top_b <= 1.0, (losses, l64)
        assert counts is None or np.array_equal(np.asarray(counts), c64), (counts, c64)
        assert max(fig.values()) <= 1.0, fig
        self.prev = before["params"]
        return ref


def _flat_of(tr, grads):
    return ls.flat(grads, tr.names).astype(np.float32)


def _plain_step(held, tr, k, seed, ksplit, twin=False, what="step"):
    """One plain step of `tr` under schedule entry k on the batch of `seed`, held to A - C; twin: and D against a fresh trainer."""
    kind, case, mode = held.kind, held.case, held.mode
    before = _state(tr)
    batch = ls.frames_at(kind, case, before["params"], tr.B, seed)
    tw = None
    if twin:
        tw = _make(kind, case, mode, before["params"], tr.B, ksplit)
        tw.m.copy_(tr.m); tw.v.copy_(tr.v); tw.step_count = tr.step_count
    hyper = _set([tr] + ([tw] if twin else []), k)
    args = _args(kind, *batch)
    losses = tr.step(*args).cpu().numpy().copy()
    counts = tr.counts.cpu().numpy().copy() if kind == "clf" else None
    grads, after = tr.grads_numpy(), _state(tr)
    held.step(before, after, batch, ksplit, grads, losses, _flat_of(tr, grads), before["t"] + 1, hyper, counts=counts, what=what)
    if twin:
        l2 = tw.step(*args).cpu().numpy()
        g2, a2 = tw.grads_numpy(), _state(tw)
        same = dict(losses=_bits(losses, l2), gradients=all(_bits(grads[n], g2[n]) for n in tr.names),
                    p=_bits(after["pmv"][0], a2["pmv"][0]), m=_bits(after["pmv"][1], a2["pmv"][1]), v=_bits(after["pmv"][2], a2["pmv"][2]))
        if kind == "clf":
            same["counts"] = bool(np.array_equal(counts, tw.counts.cpu().numpy()))
        assert all(same.values()), f"[{held.tag}] step {before['t'] + 1}: a fresh trainer on the same state differs in {[n for n, s in same.items() if not s]}"
    return after


# ---- the common sequence ----
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_three_steps_each_on_its_own_inputs(case):
    """A - D of the module docstring at steps 1, 2, 3 of one trainer: another batch and other hyper-parameters every step."""
    kind, c, mode, B, ksplit = case
    tr = _make(kind, c, mode, _initial(kind, c), B, ksplit)
    held = Held(kind, c, mode, _id(case))
    for k in range(1, ls.STEPS + 1):
        _plain_step(held, tr, k, gc.BATCH_SEED + k, ksplit, twin=True)
    assert tr.step_count == ls.STEPS


# ---- a trainer and its fork ----
@pytest.mark.parametrize("kc", KIND_CASES, ids=_id)
def test_a_trainer_and_its_fork_take_turns(kc):
    """main(50).step, fork(20).step, main.step, fork.evaluate, main.load_state_dict({one tensor}, strict=False), fork.step, main.step: every
    step held to A - C against the shared parameters then in force (each trainer's packed copies are rebuilt when the other has
    stepped or loaded), the evaluate to float64."""
    kind, case, mode = kc
    main = _make(kind, case, mode, _initial(kind, case), 50, 1)
    fork = main.fork(20)
    held = Held(kind, case, mode, _id(kc) + "-fork")
    seed = gc.BATCH_SEED
    _plain_step(held, main, 1, seed + 1, 1, what="main.step")
    _plain_step(held, fork, 2, seed + 2, 1, what="fork.step")
    _plain_step(held, main, 3, seed + 3, 1, what="main.step")
    params = main.state_dict_numpy()
    batch = ls.frames_at(kind, case, params, 20, seed + 4)
    got = fork.evaluate(*_args(kind, *batch)).cpu().numpy()
    l64, _, c64 = ls.oracle_step(kind, case, mode, params, *batch)
    err = ls.loss_err(kind, mode, got, l64) / ls.loss_rtol(kind)
    print(f"[{held.tag}] fork.evaluate after main.step: losses {err:.3f} of LOSS_RTOL")
    assert err <= 1.0 and (kind != "clf" or np.array_equal(fork.counts.cpu().numpy(), c64))
    name = main.names[0]
    main.load_state_dict({name: _initial(kind, case)[name]}, strict=False)
    assert _bits(main.state_dict_numpy()[name], _initial(kind, case)[name]) and main.step_count == 3
    held.prev = None                                   # the parameters were set, not stepped: no previous update to be stale from
    _plain_step(held, fork, 4, seed + 5, 1, what="fork.step after load_state_dict")
    _plain_step(held, main, 2, seed + 6, 1, what="main.step")
    assert main.step_count == fork.step_count == 5


# ---- accumulated steps ----
def _accumulated_step(held, acc, tail, k, seed, max_norm_factor=None):
    kind, case, mode = held.kind, held.case, held.mode
    tr = acc.trainer
    before = _state(tr)
    batch = ls.frames_at(kind, case, before["params"], sum(MICRO), seed)
    hyper = _set([tr, tail], k)
    lo = 0
    for b, t in zip(MICRO, (tr, tr, tail)):
        acc.micro(*_args(kind, *batch, lo, lo + b), trainer=t)
        lo += b
    idx = _index(tr)
    flat = acc.flat.cpu().numpy()[idx]
    gs = acc._grad_scale(acc._pending)
    losses = acc.apply().cpu().numpy().copy()
    counts = acc.counts.cpu().numpy().copy() if kind == "clf" else None
    held.step(before, _state(tr), batch, 0, acc.grads_numpy(), losses, flat, before["t"] + 1, hyper, grad_scale=gs, micro=MICRO, counts=counts,
              what="accumulated step")


@pytest.mark.parametrize("kc", KIND_CASES, ids=_id)
def test_accumulated_steps_then_plain_steps(kc):
    """Two consecutive AccumulatedSteps of 48 + 48 + 20 frames, the 20 on a fork; then main.step and tail.step."""
    kind, case, mode = kc
    tr = _make(kind, case, mode, _initial(kind, case), 48, 0)
    tail = tr.fork(20)
    acc = A.AccumulatedStep(tr, micro_batches=list(MICRO))
    held = Held(kind, case, mode, _id(kc) + "-accumulated")
    seed = gc.BATCH_SEED
    _accumulated_step(held, acc, tail, 1, seed + 1)
    _accumulated_step(held, acc, tail, 2, seed + 2)
    _plain_step(held, tr, 3, seed + 3, 0, what="main.step")
    _plain_step(held, tail, 4, seed + 4, 0, what="tail.step")
    assert tr.step_count == tail.step_count == 4


# ---- clipped steps ----
def _norm64(ref):
    return math.sqrt(clip_ref.sum_squares(list(ref.truth.values())))


def _clipped_step(held, tr, k, seed, poison=None):
    """step(max_norm = a tenth of the float64 norm of this step's gradient); poison: through AccumulatedStep, the flat gradient's last
    float set to it before the clipped apply (the recipe of tests/test_gpu_train_clip.py): the step is skipped."""
    kind, case, mode = held.kind, held.case, held.mode
    before = _state(tr)
    batch = ls.frames_at(kind, case, before["params"], tr.B, seed)
    hyper = _set([tr], k)
    args = _args(kind, *batch)
    ref = ls.reference_at(kind, case, mode, before["params"], *batch, 0) if poison is None else None
    max_norm = 0.1 * _norm64(ref) if poison is None else 1.0
    idx = _index(tr)
    if poison is not None:
        acc = A.AccumulatedStep(tr)
        acc.micro(*args)
        acc.flat[int(idx[-1])] = poison
        acc.apply(max_norm=max_norm)
        after = _state(tr)
        gn = tr.grad_norm.cpu().numpy()
        print(f"[{held.tag}] step {before['t'] + 1} with flat[-1] = {poison}: [total_norm, coef] {gn.tolist()}")
        assert all(_bits(a, b) for a, b in zip(after["pmv"], before["pmv"])), "a skipped step wrote p, m or v"
        assert after["t"] == before["t"] + 1 and gn[1] == 0.0 and tr.skipped_step_count() == 1
        return
    losses = tr.step(*args, max_norm=max_norm).cpu().numpy().copy()
    counts = tr.counts.cpu().numpy().copy() if kind == "clf" else None
    flat = CLIP.step_flat(tr).cpu().numpy()[idx]
    info = clip_ref.clip_scale([flat], 1.0, max_norm)
    gn = tr.grad_norm.cpu().numpy()
    assert 0.09 < info["coef"] < 0.11 and abs(gn[1] - info["coef"]) <= 2.0 ** -22 * info["coef"], (info, gn)
    held.step(before, _state(tr), batch, 0, tr.grads_numpy(), losses, flat, before["t"] + 1, hyper, grad_scale=info["gscale_eff"], counts=counts,
              what="clipped step", ref=ref)


@pytest.mark.parametrize("skip", [False, True], ids=["three_clipped", "a_skipped_step_between"])
@pytest.mark.parametrize("kc", KIND_CASES, ids=_id)
def test_clipped_steps(kc, skip):
    """step(max_norm = a tenth of the total norm) three times; and the same with a step in the middle that the device skips for a
    gradient that is not finite: it leaves p, m, v bit-equal and counts in step_count, so the next update is held under C with the step
    number the trainer reports (3, not 2)."""
    kind, case, mode = kc
    tr = _make(kind, case, mode, _initial(kind, case), 50, 0)
    held = Held(kind, case, mode, _id(kc) + ("-clipped-skip" if skip else "-clipped"))
    seed = gc.BATCH_SEED
    _clipped_step(held, tr, 1, seed + 1)
    _clipped_step(held, tr, 2, seed + 2, poison=math.inf if skip else None)
    _clipped_step(held, tr, 3, seed + 3)
    assert tr.step_count == 3 and tr.skipped_step_count() == 0


# ---- the reference-size trainer ----
T = importlib.import_module("disentangled-vae_amd.trainer")
N = importlib.import_module("disentangled-vae_amd.native")
REF_CASES = [("M2", 513, 33), ("M1", 0, 1000)]
LOSS_TOL = {"fp32": 1e-4, "bf16x3": 1e-5, "bf16": 2e-3}                   # test_fused_step_vs_oracle's (tests/test_gpu_fused.py)


def _raw(tr):
    """p, m, v as they lie in memory: no flush of a pending update"""
    return tuple(t.cpu().numpy().copy() for t in (tr._params, tr._m, tr._v))


def _tensors(tr, flat):
    out = {}
    for i, name in enumerate(tr.names):
        o, r, c = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i], tr.plan.tensor_cols[i]
        out[name] = flat[o:o + r * c].reshape((r, c) if name.endswith("weight") else (r * c,)).copy()
    return out


@pytest.mark.parametrize("defer", ["0", "1"], ids=["three_launch", "DVAE_DEFER_APPLY"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("model,y_dim,B", REF_CASES, ids=[f"{m}_y{y}_B{b}" for m, y, b in REF_CASES])
def test_reference_size_trainer_steps_two_and_three(model, y_dim, B, precision, defer, monkeypatch):
    """trainer.Trainer at the reference geometry: the gradients of steps 2 and 3 under grad_columns.check and the rule of the precision,
    the losses under test_fused_step_vs_oracle's tolerance, each against the float64 oracle at the parameters the step ran on.  Those
    are read from memory without a flush: where the update is deferred it runs in the opening of the NEXT call, after which the buffers
    hold what that call's step used (tests/test_gpu_fused_apply.py, part B, which holds the update itself).  Under fp32 a fresh
    trainer given that state takes the same step: losses and gradients equal bit for bit, and its p, m, v after the update are what
    the next step of this trainer ran on."""
    import golden_util as gu
    import grad_columns as gcol
    monkeypatch.setenv("DVAE_DEFER_APPLY", defer)
    dims = gcol.dims_of(y_dim)
    tr = T.Trainer(model, dims, gu.make_params(model, dims, gc.PARAM_SEED), batch=B, precision=precision, lr=ls.LR)
    pending = lambda t: bool(t.lib.dvae_train_pending(N.ptr(t.ws)))
    case, tag = (y_dim, 16, (128, 128)), f"Trainer {model} y{y_dim} B{B} {precision} defer {defer}"
    expected, deferred, idx = None, 0, _index(tr)        # (the floats between the tensors belong to nobody and are not compared)
    for k in range(1, ls.STEPS + 1):
        x, y, e = gu.make_batch(dims, B, gc.BATCH_SEED + k)
        args = tuple(_dev(a) for a in (x, y, e))
        lr, b1, b2, eps = _set([tr], k)
        pre, was_pending = _raw(tr), pending(tr)
        losses = tr.step(*args).cpu().numpy().copy()
        grads = tr.grads_numpy()
        if pending(tr):                                # this step's update waits: memory holds what the step ran on
            assert defer == "1"
            used, deferred = _raw(tr), deferred + 1
        else:
            assert not was_pending, "the parameters this step ran on were never in memory"
            used = pre
        if expected is not None:
            assert all(_bits(a[idx], b[idx]) for a, b in zip(used, expected)), f"[{tag}] step {k} did not start from the state a fresh trainer left"
        params = _tensors(tr, used[0])
        if k >= 2:
            ref = gcol.Reference.at(model, y_dim, params, x, y, e)
            fails, top = gcol.check(grads, ref, precision, label=f"[{tag} step {k}]")
            l64 = ls.oracle_step("generic", case, None, params, x, y, e)[0]
            err = float(np.max(np.abs(losses[:3] - l64) / np.abs(l64)))
            print(f"[{tag}] step {k}: A gradients {top:.3f} of the column bound, B losses {err / LOSS_TOL[precision]:.3f} of {LOSS_TOL[precision]:g}")
            assert not fails, fails
            assert err <= LOSS_TOL[precision], (losses, l64)
        if precision == "fp32":
            tw = T.Trainer(model, dims, params, batch=B, precision=precision, lr=ls.LR)
            tw._m.copy_(_dev(used[1])); tw._v.copy_(_dev(used[2])); tw.step_count = k - 1
            _set([tw], k)
            l2 = tw.step(*args).cpu().numpy()
            g2 = tw.grads_numpy()
            assert _bits(losses, l2) and all(_bits(grads[n], g2[n]) for n in tr.names), f"[{tag}] step {k}: a fresh trainer on the same state differs"
            tw.flush()
            expected = _raw(tw)
    tr.flush()
    assert tr.step_count == ls.STEPS and (deferred > 0) == (defer == "1" and bool(tr.lib.dvae_train_can_defer(ctypes.byref(tr.plan), N.ptr(tr.ws))))
    if expected is not None:
        assert all(_bits(a[idx], b[idx]) for a, b in zip(_raw(tr), expected)), f"[{tag}] the last update differs from a fresh trainer's"


# ---- the module path: the script loop with stock torch.optim.Adam ----
def test_script_loop_on_the_generic_engine_every_iteration_against_float64(monkeypatch):
    """test_script_loop_with_a_kl_weight_runs_on_the_generic_engine (tests/test_gpu_module_generic.py) holds its first iteration; here
    every one of three, with another batch each and torch.optim.Adam(lr=1e-3) between them: the loss and every parameter gradient
    against float64 at the module's own state_dict() of that iteration, by module_generic_cases' rule -- the engine reads the
    parameters again after optimizer.step() wrote them."""
    import module_generic_cases as mg
    from test_gpu_module_generic import U24, _elbo_upstreams, _load, _loop_step
    case, B, W = (0, 32, (256, 64)), 50, 0.25
    model = gc.model_of(case)
    monkeypatch.delenv("DVAE_MODULE_PATH", raising=False)
    monkeypatch.setenv("DVAE_MODULE_GENERIC", "1")
    m = _load(case)
    opt = torch.optim.Adam(m.parameters(), lr=ls.LR)
    up, prev = mg.make_upstream(B, case[1]), None
    for it in range(1, ls.STEPS + 1):
        params = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
        x, y, e = gc.inputs(case, B, gc.BATCH_SEED + it)[1:]
        (loss, _, _), _, grads = _loop_step(m, model, _dev(x), _dev(y), _dev(e), W)
        eng = m.__dict__.get("_dvae_engine")
        assert eng is not None and eng.kind == "generic"
        g = {k: v.detach().cpu().numpy() for k, v in grads.items()}
        ref = mg.Reference.at(case, params, x, y, e, up)
        runs = {}
        for name, dtype, hook in (("truth", np.float64, None), ("numpy", np.float32, None),
                                  ("k-steps", np.float32, gg.StepOrderF32(ref.slice_frames, case[1]))):
            args = (case, params, x, y, e)
            ups = _elbo_upstreams(mg.run(*args, {}, dtype, hook)[0], x, B, W, dtype)
            runs[name] = mg.run(*args, {"kl": ups}, dtype, hook)[1]["kl"]
        truth = runs["truth"]
        fig32 = mg.mc.merge(mg.mc.grad_figures(runs["numpy"], truth), mg.mc.grad_figures(runs["k-steps"], truth))
        x64, o = x.astype(np.float64), ref.out
        recon = float(np.sum(x64 / o["r"] - np.log(x64 + 1e-8) + o["a"] - 1.0) / B)
        kl = float(np.sum(-0.5 * (o["lv"] - o["mu"] ** 2 - np.exp(o["lv"]))) / B)
        out_b = mg.mc.gc.bound(ref.out_fig["r"])[0] * max(1.0, float(np.abs(o["a"]).max()))        # the loss bound of the test named above
        terms = np.abs(x64 / o["r"]) * out_b + out_b + U24 * (np.abs(x64 / o["r"]) + np.abs(np.log(x64 + 1e-8)) + np.abs(o["a"]) + 1.0)
        loss_bound = (4.0 * (float(terms.sum()) / B + U24 * abs(recon))
                      + 4.0 * W * 4.0 * U24 * float(np.sum(np.abs(o["lv"]) + o["mu"] ** 2 + np.exp(o["lv"]))) / B)
        fails, top, _ = mg.mc.check(mg.mc.grad_figures(g, truth), g, truth, fig32, None, f"[module loop, iteration {it}]")
        off = abs(float(loss.detach()) - (recon + W * kl))
        line = f"[module loop, generic engine] iteration {it}: gradients {top:.3f} of the bound, loss {off / loss_bound:.3f} of its bound"
        if prev is not None:                           # the premise, from the oracle alone: the same gradients at the previous iteration's parameters
            ups = _elbo_upstreams(mg.run(case, prev, x, y, e, {})[0], x, B, W, np.float64)
            before = mg.run(case, prev, x, y, e, {"kl": ups})[1]["kl"]
            stale, _, _ = mg.mc.check(mg.mc.grad_figures(before, truth), before, truth, fig32, None, "")
            line += f"; the float64 gradients at the previous parameters miss the rule in {len(stale)} figures"
            assert stale
        print(line)
        assert not fails, fails
        assert off <= loss_bound
        prev = params
        opt.step()


def _linear_loss(outs, up):
    """sum of every output times a fixed upstream gradient: the rule's "all" entry as a loss a script could write"""
    r, z, mu, lv = outs
    return (r * up["r"]).sum() + (z * up["z"]).sum() + (mu * up["mu"]).sum() + (lv * up["lv"]).sum()


def _module_loop(tag, engine_of, names, batch_of, reference_at, check):
    """Three iterations of forward, a loss, backward and torch.optim.Adam(lr=1e-3).step() on the engine's own parameters, another batch
    each: the outputs and every parameter gradient of EVERY iteration by the engine's rule against float64 at the parameters the module
    holds when the iteration starts; and, from the oracle alone, the float64 gradients at the previous iteration's parameters miss that
    rule (the premise that an engine which did not read the parameters again would be seen)."""
    mp = importlib.import_module("disentangled-vae_amd.module_path")
    opt, prev = None, None
    for it in range(1, ls.STEPS + 1):
        x, y, e, up = batch_of(it)
        dx, dy, de = _dev(x), _dev(y), _dev(e)
        eng = engine_of(dx, dy)
        if opt is None:
            opt = torch.optim.Adam(list(eng.params), lr=ls.LR)
        params = {k: p.detach().cpu().numpy().copy() for k, p in zip(names, eng.params)}
        r, z, mu, lv = mp.run(eng, dx, dy, de)
        opt.zero_grad(set_to_none=True)
        _linear_loss((r, z, mu, lv), {k: _dev(v) for k, v in up.items()}).backward()
        got = {k: v.detach().cpu().numpy() for k, v in (("r", r), ("z", z), ("mu", mu), ("lv", lv))}
        g = {k: p.grad.detach().cpu().numpy() for k, p in zip(names, eng.params)}
        ref = reference_at(params, x, y, e, up)
        fo, to, fg, tg = check(ref, got, g, f"[{tag}, iteration {it}]")
        line = f"[{tag}] iteration {it}: outputs {to:.3f} of the bound, gradients {tg:.3f}"
        if prev is not None:
            before = reference_at(prev, x, y, e, up).truth["all"]
            stale = check(ref, None, {k: before[k] for k in names}, "")[2]
            line += f"; the float64 gradients at the previous parameters miss the rule in {len(stale)} figures"
            assert stale
        print(line)
        assert not fo and not fg, (fo, fg)
        prev = params
        opt.step()


def test_module_loop_on_the_resident_engine_every_iteration_against_float64(monkeypatch):
    """The reference geometry (M2, one label, 33 frames, bf16x3) on the resident engine, by tests/test_gpu_module_oracle.py's rule."""
    import golden_util as gu
    import module_cases as mc
    from impl_modules import build_model
    mp = importlib.import_module("disentangled-vae_amd.module_path")
    model, y_dim, B, precision = "M2", 1, 33, "bf16x3"
    for k in ("DVAE_MODULE_PATH", "DVAE_MODULE_GENERIC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DVAE_MODULE_PRECISION", precision)
    params = mc.params_of(model, y_dim)
    m = build_model(model, mc.gc.dims_of(y_dim))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.cuda()

    def engine_of(x, y):
        eng = mp.engine_for(m, model, x, y)
        assert eng is not None and eng.kind != "generic" and eng.precision == precision
        return eng

    def check(ref, got, g, label):
        fo, to = ([], 0.0) if got is None else ref.check_outputs(got, precision, label)[:2]
        fg, tg = ref.check_grads(g, "all", precision, label)[:2]
        return fo, to, fg, tg

    _module_loop("module loop, resident engine", engine_of, list(params),
                 lambda it: gu.make_batch(mc.gc.dims_of(y_dim), B, mc.BATCH_SEED + it) + (mc.make_upstream(B),),
                 lambda p, x, y, e, up: mc.Reference.at(model, y_dim, p, x, y, e, up), check)


def test_module_loop_on_the_m2_info_body_every_iteration_against_float64(monkeypatch):
    """The M2_info body (DeepGenerativeModel_v3) at (3, 17, (129, 127)), 50 frames, on its generic engine, by
    tests/test_gpu_module_info.py's rule."""
    import golden_util as gu
    import module_info_cases as mi
    from test_gpu_module_info import NAMES, _env, _v3
    mp = importlib.import_module("disentangled-vae_amd.module_path")
    case, B = (3, 17, (129, 127)), 50
    _env(monkeypatch, "1")
    m = _v3(case)

    def engine_of(x, y):
        eng = mp.engine_for(m, "M2_DEC", x, y)
        assert eng is not None and eng.kind == "generic"
        return eng

    def check(ref, got, g, label):
        fo, to = ([], 0.0) if got is None else ref.check_outputs(got, label)[:2]
        fg, tg = ref.check_grads(g, "all", label)[:2]
        return fo, to, fg, tg

    _module_loop("module loop, M2_info body", engine_of, NAMES,
                 lambda it: gu.make_batch(gc.dims_of(case), B, gc.BATCH_SEED + it) + (mi.mg.make_upstream(B, case[1]),),
                 lambda p, x, y, e, up: mi.Reference.at(case, p, x, y, e, up), check)

"""The geometry cases, inputs, float64 truths and bars of the generic M2_info fused train step (csrc/train_info.hip;
disentangled-vae_amd/trainer_info.py), shared by tests/test_train_info_cpu.py and tests/test_gpu_train_info.py.  No GPU here.

Cases (y, z, (h1, h2)): sizes off every multiple of 4 and 16, every limit at once, IBM labels on a narrow net, the reference geometry
(which the resident step serves by default), seven labels at the reference widths, and (1, 1, (1, 1)).
Parameters: gu.make_params("M2_info", dims, 11).  Loss weights: grad_columns.INFO_WEIGHTS = (0.5, 10, 1), so that all three terms pull.

Frames.  Both side nets are ReLU classifiers under a sigmoid, and two things make float32 and float64 disagree through no fault of a
kernel (tests/train_classifier_cases.py): a ReLU unit within rounding of zero flips its mask, and a saturated sigmoid makes
log(1 - p + eps) depend on the arithmetic width.  So the B frames of a case are the FIRST B frames of the pool
gu.make_batch(dims, 8 B + 16, 12) that pass, in the float64 oracle, for BOTH the classifier on x and the auxiliary net on z (z from
vo.encoder_fwd with the pool's eps):
  1. every unit of all three layers has |pre| / (sum |w in| + |b|) >= MARGIN = 1e-4;
  2. every logit has |a| <= LOGIT_MAX = 12.
The selected frames keep their own eps rows.  The pool must suffice: that is asserted (a condition of the inputs).

Truth: vo.m2info_losses_and_grads / vo.train_step_m2info in float64; the gradient of an auxiliary tensor is what the script's second
optimizer steps with, (gamma - beta) dBCE (g1 + g2 of the oracle).
Bars: the project's fp32 bars of the fused step -- each of the seven losses 1e-4 relative, every gradient tensor within 1e-4 of its
maximum; a tensor whose truth is all zero (the auxiliary net's dead unit at (1, 1, (1, 1))) must be all zero.

Trajectory: STEPS_TRAJ = 3 steps at LR_TRAJ = 1e-6 on frames of the B_TRAJ = 50 batch.  The loss bars are asked at every step on frames
that still pass the selection under the float64 parameters the step starts from.  An Adam step moves every weight by about lr, which
shifts a pre-activation by lr sum |x| against its scale sum |w x|: a relative lr / |w|, with |w| ~ 0.05.  At the lr of 1e-2 of the
M1 / M2 and classifier trajectories that is 0.2, two thousand margins: every frame is drawn again at every step, a third to all of
them fail, and float32 numpy itself leaves the float64 trajectory by up to 0.7 of a loss.  So the frames of the trajectory are the
fixed point of traj_frames(): run the float64 trajectory, take out the frames that fail at any step, run it again on the rest.
Checked on the CPU (tests/test_train_info_cpu.py: test_trajectory_premises) for three steps:
    lr 1e-5   every case but (1, 1, (1, 1)) loses 16 to 32 % of its frames, (513, 128, (512, 512)) all of them
    lr 1e-6   (513, 128, (512, 512)) keeps 25 of 50, every other case at least 48
    lr 1e-7   (513, 128, (512, 512)) keeps 41, every other case at least 49 -- but the losses then move by less than the bar itself
lr 1e-6 is the largest at which at most a quarter of the cases drop (one of eight: a case counts as dropped when it keeps fewer than
three quarters of its frames) and the float64 losses still move by 2 to 19 bars over the steps at six cases of the eight, so that a
step taken with stale weights or moments fails.  A dropped case is still compared, on the frames it keeps."""
import functools

import numpy as np

import golden_util as gu
import grad_columns as gc
from oracle import vae_oracle as vo

CASES = [(1, 32, (256, 64)), (1, 5, (48, 200)), (513, 64, (16, 16)), (3, 17, (129, 127)), (513, 128, (512, 512)), (1, 16, (128, 128)),
         (7, 16, (128, 128)), (1, 1, (1, 1))]
PARAM_SEED, BATCH_SEED = 11, 12
WEIGHTS = gc.INFO_WEIGHTS              # alpha, beta, gamma
BATCHES = (1, 50)                      # one frame; three tiles and a ragged fourth
LOSS_RTOL = 1e-4
GRAD_TOL = 1e-4                        # of the tensor's largest gradient
LR_TRAJ, STEPS_TRAJ, B_TRAJ = 1e-6, 3, 50
TRAJ_DROPPED_MAX = 0.25                # share of the cases that may drop, and of a kept case's frames that may
LOOPS_CASE = (1, 5, (48, 200))
MARGIN, LOGIT_MAX = 1e-4, 12.0
ELBO_EPS = 1e-8
LOSS_NAMES = ("ELBO", "recon", "kl", "enc_loss", "classif_loss", "aux_loss", "aux_enc_loss")     # the order of the step's loss scalars
ENC, CLF, AUX = "enc_dec_clf.encoder.", "enc_dec_clf.classifier.", "auxiliary."


def case_id(case):
    y, z, (h1, h2) = case
    return f"y{y}_z{z}_h{h1}x{h2}"


def dims_of(case):
    y, z, h = case
    return dict(x_dim=513, y_dim=y, z_dim=z, h_dim=tuple(h))


@functools.lru_cache(maxsize=None)
def params_of(case):
    p = gu.make_params("M2_info", dims_of(case), PARAM_SEED)
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def pool(case, B, batch_seed=BATCH_SEED):
    """The raw frames the selection draws from: (x, y, eps) of 8 B + 16 frames."""
    x, y, eps = gu.make_batch(dims_of(case), 8 * B + 16, batch_seed)
    for a in (x, y, eps):
        a.setflags(write=False)
    return x, y, eps


def _net_ok(p, prefix, h):
    ok = np.ones(h.shape[0], bool)
    for name in ("hidden.0", "hidden.1", "output_layer"):
        W, b = p[prefix + name + ".weight"], p[prefix + name + ".bias"]
        pre = h @ W.T + b
        ok &= (np.abs(pre) / (np.abs(h) @ np.abs(W).T + np.abs(b) + 1e-300)).min(axis=1) >= MARGIN
        if name == "output_layer":
            ok &= np.abs(pre).max(axis=1) <= LOGIT_MAX
        h = np.maximum(pre, 0)
    return ok


def frames_ok(params, x, eps):
    """Per frame (float64 oracle, any parameters): both conditions of the module docstring hold for the classifier on x and for the
    auxiliary net on z."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    x64, e64 = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    z = vo.encoder_fwd(p, ENC, x64, e64)["z"]
    return _net_ok(p, CLF, x64) & _net_ok(p, AUX, z)


@functools.lru_cache(maxsize=None)
def selection(case, B, batch_seed=BATCH_SEED):
    """(indices of the first B passing frames of the pool, number of pool frames that pass)."""
    x, _, eps = pool(case, B, batch_seed)
    ok = frames_ok(params_of(case), x, eps)
    idx = np.flatnonzero(ok)
    assert idx.size >= B, f"{case_id(case)} B {B}: only {idx.size} of {x.shape[0]} pool frames pass the selection"
    return idx[:B], int(ok.sum())


@functools.lru_cache(maxsize=None)
def inputs(case, B, batch_seed=BATCH_SEED):
    """(params, x, y, eps) in float32; shared, never written."""
    x, y, eps = pool(case, B, batch_seed)
    idx, _ = selection(case, B, batch_seed)
    out = tuple(np.ascontiguousarray(a[idx]) for a in (x, y, eps))
    for a in out:
        a.setflags(write=False)
    return (params_of(case),) + out


def losses_of(out):
    return np.array([out[k] for k in LOSS_NAMES], np.float64)


def step_grads(p, g1, aux_total):
    """What one step deposits per tensor: enc_loss.backward() in the enc_dec_clf tensors, (gamma - beta) dBCE in the auxiliary ones."""
    g = {k: v for k, v in g1.items() if not k.startswith(AUX)}
    g.update(aux_total)
    return {k: np.asarray(v, np.float64).reshape(p[k].shape) for k, v in g.items()}


def run_on(params, x, y, eps, dtype, steps=1, lr=1e-4, weights=WEIGHTS):
    """`steps` oracle train steps on the same batch in `dtype`: ([7 losses], [grads], params after, [params each step started from])."""
    p = {k: v.astype(dtype) for k, v in params.items()}
    x, y, eps = x.astype(dtype), y.astype(dtype), eps.astype(dtype)
    a, b, g = weights
    opt_edc = vo.AdamState([k for k in p if not k.startswith(AUX)])
    opt_aux = vo.AdamState([k for k in p if k.startswith(AUX)])
    losses, grads, starts = [], [], []
    for _ in range(steps):
        starts.append({k: v.copy() for k, v in p.items()})
        out, g1, _, aux_total = vo.train_step_m2info(p, opt_edc, opt_aux, x, y, eps, alpha=a, beta=b, gamma=g, eps=ELBO_EPS, lr=lr)
        losses.append(losses_of(out))
        grads.append(step_grads(p, g1, aux_total))
    return losses, grads, p, starts


def run(case, B, dtype, steps=1, lr=1e-4, weights=WEIGHTS, batch_seed=BATCH_SEED):
    return run_on(*inputs(case, B, batch_seed), dtype, steps, lr, weights)


@functools.lru_cache(maxsize=None)
def truth(case, B, steps=1, lr=1e-4, weights=WEIGHTS, batch_seed=BATCH_SEED):
    return run(case, B, np.float64, steps, lr, weights, batch_seed)


@functools.lru_cache(maxsize=None)
def traj_frames(case):
    """Indices into inputs(case, B_TRAJ) of the frames the trajectory runs on: every one of them passes the selection under the float64
    parameters each of the STEPS_TRAJ steps starts from, on the trajectory of exactly these frames (the fixed point of the module
    docstring; it shrinks at every round, so it ends)."""
    p, x, y, eps = inputs(case, B_TRAJ)
    idx = np.arange(B_TRAJ)
    while idx.size:
        starts = run_on(p, x[idx], y[idx], eps[idx], np.float64, STEPS_TRAJ, LR_TRAJ)[3]
        ok = np.ones(idx.size, bool)
        for s in starts:
            ok &= frames_ok(s, x[idx], eps[idx])
        if ok.all():
            break
        idx = idx[ok]
    assert idx.size, f"{case_id(case)}: no frame passes the selection along the trajectory"
    idx.setflags(write=False)
    return idx


def traj_dropped(case):
    return traj_frames(case).size < (1 - TRAJ_DROPPED_MAX) * B_TRAJ


@functools.lru_cache(maxsize=None)
def traj_inputs(case):
    p, x, y, eps = inputs(case, B_TRAJ)
    idx = traj_frames(case)
    out = tuple(np.ascontiguousarray(a[idx]) for a in (x, y, eps))
    for a in out:
        a.setflags(write=False)
    return (p,) + out


@functools.lru_cache(maxsize=None)
def traj_truth(case):
    return run_on(*traj_inputs(case), np.float64, STEPS_TRAJ, LR_TRAJ)


def loss_err(got, ref):
    """Worst relative error of the seven losses; a loss whose truth is zero (alpha = 0: classif_loss) must be zero."""
    got, ref = np.asarray(got, np.float64)[:7], np.asarray(ref, np.float64)[:7]
    worst = 0.0
    for a, r in zip(got, ref):
        e = (0.0 if a == 0.0 else float("inf")) if r == 0.0 else abs(a - r) / abs(r)
        if not np.isfinite(e):
            return float("inf")
        worst = max(worst, float(e))
    return worst


def grad_err(got, ref):
    """Worst error of a gradient tensor over that tensor's largest gradient, and the tensor's name; a tensor whose truth is all zero
    must be all zero (its error is then 0, otherwise infinite)."""
    worst, name = 0.0, None
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        top = float(np.max(np.abs(r)))
        if top == 0.0:
            e = 0.0 if not np.any(g) else float("inf")
        else:
            e = float(np.max(np.abs(g - r)) / top)
        if not np.isfinite(e) or e >= worst:
            worst, name = e, k
    return worst, name


def loops_batch(plan_of):
    """The smallest batch of the ladder of tests/train_generic_cases.py at which the plan of LOOPS_CASE strides its rows grid over more
    tiles than it has workgroups and cuts the frames into at least two slices, the last one shorter.  plan_of(B) -> plan."""
    for tiles in (8, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        B = 16 * tiles + 16 * 3 + 5
        p = plan_of(B)
        if -(-B // 16) > p.rows_grid and p.ksplit >= 2 and B % p.slice_frames != 0 and (p.ksplit - 1) * p.slice_frames < B:
            return B, p
    raise AssertionError("no batch of the ladder makes the rows kernel stride and the frames split")

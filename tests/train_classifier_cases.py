"""The geometry cases, inputs, float64 truths and bars of the classifier's fused train step (csrc/train_classifier.hip;
disentangled-vae_amd/trainer_classifier.py), shared by tests/test_train_classifier_cpu.py and tests/test_gpu_train_classifier.py.  No GPU.

Cases: those of the generic classifier kernel (tests/mlp_generic_cases.py: CLASSIFIER_CASES -- every limit, sizes off every multiple of
4 and 16, (1, 1)) plus the reference geometry with one label and a narrow first layer under a wide second one.
Parameters: the classifier tensors of gu.make_params("M2_info", dims(z_dim=1), 11), the prefix stripped.

Frames.  A classifier sees raw power spectra up to 1e4, and two things make float32 and float64 disagree through no fault of a kernel
(tests/test_gpu_fused.py: test_fused_m2info_vs_oracle_full_batch, _relu_margins): a ReLU unit within rounding of zero flips its mask, and
a saturated sigmoid makes log(1 - p + eps) depend on the arithmetic width.  So the B frames of a case are the FIRST B frames of the pool
gu.make_batch(dims, 8 B + 16, 12) that pass, in the float64 oracle,
  1. every unit of all three layers has |pre| / (sum |w in| + |b|) >= MARGIN = 1e-4 -- above the worst-case float32 dot-product error
     (K + 2) 2^-24 = 3.1e-5 at K = 513;
  2. every logit has |a| <= LOGIT_MAX = 12, so 1 - p stays above 6e-6.
The pool must suffice: that is asserted (a condition of the inputs, not a measurement of the code under test).

Truth: vo.classifier_fwd, binary_cross_entropy, bce_bwd, classifier_bwd and AdamState in float64.
Bars: the project's fp32 bar of the fused step -- loss 1e-4 relative, every gradient tensor within 1e-4 of its maximum; a tensor whose
truth is all zero (the dead unit of (1, 1)) must be all zero."""
import functools

import numpy as np

import golden_util as gu
from mlp_generic_cases import CLASSIFIER_CASES
from oracle import vae_oracle as vo

CASES = list(CLASSIFIER_CASES) + [((128, 128), 1), ((16, 512), 7)]
PARAM_SEED, BATCH_SEED = 11, 12
BATCHES = (1, 50)                      # one frame; three tiles and a ragged fourth
LOSS_RTOL = 1e-4
GRAD_TOL = 1e-4                        # of the tensor's largest gradient
LR_TRAJ, STEPS_TRAJ, B_TRAJ = 1e-2, 3, 50
LOOPS_CASE = ((48, 200), 2)
MARGIN, LOGIT_MAX = 1e-4, 12.0
BCE_EPS = 1e-8
PREFIX = "enc_dec_clf.classifier."
NAMES = ["hidden.0.weight", "hidden.0.bias", "hidden.1.weight", "hidden.1.bias", "output_layer.weight", "output_layer.bias"]


def case_id(case):
    (h1, h2), y = case
    return f"h{h1}x{h2}_y{y}"


def dims_of(case):
    """The reference's dims list of Classifier."""
    (h1, h2), y = case
    return [513, [h1, h2], y]


def _info_dims(case):
    (h1, h2), y = case
    return dict(x_dim=513, y_dim=y, z_dim=1, h_dim=(h1, h2))


@functools.lru_cache(maxsize=None)
def params_of(case):
    p = gu.make_params("M2_info", _info_dims(case), PARAM_SEED)
    out = {k[len(PREFIX):]: v for k, v in p.items() if k.startswith(PREFIX)}
    assert list(out) == NAMES
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pool(case, B, batch_seed=BATCH_SEED):
    """The raw frames and labels the selection draws from: (x, y) of 8 B + 16 frames."""
    x, y, _ = gu.make_batch(_info_dims(case), 8 * B + 16, batch_seed)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


def frame_ok(case, x):
    """Per frame of x (float64 oracle): both conditions of the module docstring hold under the case's own parameters."""
    return frames_ok(params_of(case), x)


def frames_ok(params, x):
    """frame_ok under any parameters (tests/later_steps.py: those a later step starts from)."""
    p = {k: np.asarray(v).astype(np.float64) for k, v in params.items()}
    h = x.astype(np.float64)
    ok = np.ones(x.shape[0], bool)
    for name in ("hidden.0", "hidden.1", "output_layer"):
        W, b = p[name + ".weight"], p[name + ".bias"]
        pre = h @ W.T + b
        ok &= (np.abs(pre) / (np.abs(h) @ np.abs(W).T + np.abs(b) + 1e-300)).min(axis=1) >= MARGIN
        if name == "output_layer":
            ok &= np.abs(pre).max(axis=1) <= LOGIT_MAX
        h = np.maximum(pre, 0)
    return ok


@functools.lru_cache(maxsize=None)
def selection(case, B, batch_seed=BATCH_SEED):
    """(indices of the first B passing frames of the pool, fraction of the pool that passes)."""
    x, _ = pool(case, B, batch_seed)
    ok = frame_ok(case, x)
    idx = np.flatnonzero(ok)
    assert idx.size >= B, f"{case_id(case)} B {B}: only {idx.size} of {x.shape[0]} pool frames pass the selection"
    return idx[:B], float(ok.mean())


@functools.lru_cache(maxsize=None)
def inputs(case, B, batch_seed=BATCH_SEED):
    """(params, x, y) in float32; shared, never written."""
    x, y = pool(case, B, batch_seed)
    idx, _ = selection(case, B, batch_seed)
    xs, ys = np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])
    xs.setflags(write=False); ys.setflags(write=False)
    return params_of(case), xs, ys


LOGIT_ALONE = 6.0


@functools.lru_cache(maxsize=None)
def alone_frames(case, B):
    """The frames of inputs(case, B) whose loss a test may compare ALONE with float64 under LOSS_RTOL: every logit within LOGIT_ALONE.
    A float32 p carries an absolute error of a few 2^-24 (its own rounding near 1 is 2^-25; exp and the division add theirs), and
    log(1 - p + eps) turns it into a relative error of 1 - p: at |a| <= 12 that is up to 4 * 2^-24 / 6e-6 = 4e-2 on one term of a
    confidently wrong label, which a batch averages away (test_float32_arithmetic_needs_less_than_a_third_of_the_bars) and one frame
    does not.  At |a| <= 6, 1 - p >= 2.5e-3: at most 4 * 2^-24 / 2.5e-3 = 1e-4 absolute on a term of at least 6, 1.6e-5 of the loss."""
    p, x, _ = inputs(case, B)
    h = x.astype(np.float64)
    for name in ("hidden.0", "hidden.1"):
        h = np.maximum(h @ p[name + ".weight"].astype(np.float64).T + p[name + ".bias"], 0)
    a = h @ p["output_layer.weight"].astype(np.float64).T + p["output_layer.bias"]
    return np.flatnonzero(np.abs(a).max(axis=1) <= LOGIT_ALONE)


def counts_of(p, y):
    """tp, tn, fp, fn of p > 0.5 against y != 0 over every element (the order of label_counts_batch)."""
    hat, tru = p > 0.5, y != 0
    return np.array([np.sum(hat & tru), np.sum(~hat & ~tru), np.sum(hat & ~tru), np.sum(~hat & tru)], np.int64)


def loss_and_grads(p, x, y, eps=BCE_EPS):
    """One forward / backward of the oracle in the dtype of its inputs: (loss, grads, counts, soft labels)."""
    cache = vo.classifier_fwd(p, "", x)
    loss = vo.binary_cross_entropy(cache["p"], y, eps)
    grads = {}
    vo.classifier_bwd(p, grads, "", cache, vo.bce_bwd(cache["p"], y, eps, 1.0), need_dx=False)
    return loss, grads, counts_of(cache["p"], y), cache["p"]


def run_on(params, x, y, dtype, steps=1, lr=1e-4):
    p = {k: v.astype(dtype) for k, v in params.items()}
    x, y = x.astype(dtype), y.astype(dtype)
    opt = vo.AdamState(list(p))
    losses, grads, counts = [], [], []
    for _ in range(steps):
        loss, g, c, _ = loss_and_grads(p, x, y)
        opt.step(p, g, lr=lr)
        losses.append(float(loss))
        grads.append({k: np.asarray(v, np.float64).reshape(p[k].shape) for k, v in g.items()})
        counts.append(c)
    return losses, grads, counts, p


def run(case, B, dtype, steps=1, lr=1e-4, batch_seed=BATCH_SEED):
    """`steps` oracle train steps on the same batch in `dtype`: ([loss], [grads], [counts], params after)."""
    return run_on(*inputs(case, B, batch_seed), dtype, steps, lr)


@functools.lru_cache(maxsize=None)
def truth(case, B, steps=1, lr=1e-4, batch_seed=BATCH_SEED):
    return run(case, B, np.float64, steps, lr, batch_seed)


def loss_err(got, ref):
    return float(abs(float(got) - float(ref)) / abs(float(ref)))


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
    """The smallest batch of the ladder at which the plan of LOOPS_CASE strides its rows grid over more tiles than it has workgroups and
    cuts the frames into at least two slices, the last one shorter (the ladder of tests/train_generic_cases.py).  plan_of(B) -> plan."""
    for tiles in (8, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        B = 16 * tiles + 16 * 3 + 5
        p = plan_of(B)
        if -(-B // 16) > p.rows_grid and p.ksplit >= 2 and B % p.slice_frames != 0 and (p.ksplit - 1) * p.slice_frames < B:
            return B, p
    raise AssertionError("no batch of the ladder makes the rows kernel stride and the frames split")

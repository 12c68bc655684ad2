"""The float64 truth of the generic train step with a standardised encoder input (std_norm: csrc/train_generic.hip, NORM;
disentangled-vae_amd/trainer_generic.py), shared by tests/test_std_norm_cpu.py and tests/test_gpu_train_std_norm.py.  No GPU here.

The truth is the scripts' loop body (scripts/training_M2.py:136-144: `model(x_norm, y)`, `elbo(x, r, ...)`) composed from the pieces of
oracle.vae_oracle: encoder_fwd on [xn32 | y], decoder_fwd, elbo / elbo_bwd against the RAW x, decoder_bwd, encoder_bwd.  xn32 is the
float32 torch forms, (x - mean) / (std + eps) with std + eps rounded to float32 first: the step's input by contract, so the truth starts
from it in every precision.

Cases, inputs, bars: those of tests/train_generic_cases.py.  The statistics come from a 200-frame pool drawn with another seed
(inputs(case, 200, 77)), not from the batch: |xn| reaches 2.5e3 in the batch and tanh units saturate, as on real data."""
import functools

import numpy as np

import frame_stats_ref as fs
import train_generic_cases as tc
from oracle import vae_oracle as vo

CASES, BATCHES, LOSS_RTOL, GRAD_TOL = tc.CASES, tc.BATCHES, tc.LOSS_RTOL, tc.GRAD_TOL
LR_TRAJ, STEPS_TRAJ, B_TRAJ, LOOPS_CASE = tc.LR_TRAJ, tc.STEPS_TRAJ, tc.B_TRAJ, tc.LOOPS_CASE
POOL, POOL_SEED = 200, 77
NORM_EPS = 1e-8


@functools.lru_cache(maxsize=None)
def stats(case):
    """(mean, std) float32 [513] of the pool; shared, never written."""
    mean, std = fs.stats_ref(tc.inputs(case, POOL, POOL_SEED)[1])
    mean.setflags(write=False)
    std.setflags(write=False)
    return mean, std


def normalise(x, mean, std, norm_eps=NORM_EPS):
    """xn32: float32 numpy is IEEE, as torch's (x - mean) / (std + eps) is."""
    div = (np.asarray(std, np.float32) + np.float32(norm_eps)).astype(np.float32)
    return ((np.asarray(x, np.float32) - np.asarray(mean, np.float32)) / div).astype(np.float32)


def loss_and_grads(model, params, xn, x, y, eps_noise, eps=1e-8):
    """One loop body in the dtype of the arguments: (loss, recon, kl), grads."""
    enc_in = xn if model == "M1" else np.concatenate([xn, y], axis=1)
    enc = vo.encoder_fwd(params, "encoder.", enc_in, eps_noise)
    dec = vo.decoder_fwd(params, "decoder.", enc["z"] if model == "M1" else np.concatenate([enc["z"], y], axis=1))
    loss, recon, kl = vo.elbo(x, dec["r"], enc["mu"], enc["lv"], eps)
    grads = {}
    da, dmu_kl, dlv_kl = vo.elbo_bwd(x, dec["a"], enc["mu"], enc["lv"])
    ddec_in = vo.decoder_bwd(params, grads, "decoder.", dec, da)
    vo.encoder_bwd(params, grads, "encoder.", enc, ddec_in[:, :enc["z"].shape[1]], dmu_kl, dlv_kl, need_dx=False)
    return np.array([loss, recon, kl], np.float64), grads


def cast_inputs(case, B, dtype, batch_seed=tc.BATCH_SEED, stats_of=None):
    """(params, xn, x, y, eps) in `dtype`; stats_of: (mean, std) in the place of the pool's."""
    params, x, y, eps = tc.inputs(case, B, batch_seed)
    xn = normalise(x, *(stats_of or stats(case)))
    f = lambda a: None if a is None else a.astype(dtype)
    return {k: f(v) for k, v in params.items()}, f(xn), f(x), f(y), f(eps)


def run(case, B, dtype, steps=1, lr=1e-4, batch_seed=tc.BATCH_SEED):
    """`steps` train steps on the same batch in `dtype`: ([(loss, recon, kl)], [grads], params after)."""
    p, xn, x, y, eps = cast_inputs(case, B, dtype, batch_seed)
    opt = vo.AdamState(list(p))
    losses, grads = [], []
    for _ in range(steps):
        l, g = loss_and_grads(tc.model_of(case), p, xn, x, y, eps)
        opt.step(p, g, lr=lr)
        losses.append(l)
        grads.append({k: np.asarray(v, np.float64).reshape(p[k].shape) for k, v in g.items()})
    return losses, grads, p


@functools.lru_cache(maxsize=None)
def truth(case, B, steps=1, lr=1e-4, batch_seed=tc.BATCH_SEED):
    return run(case, B, np.float64, steps, lr, batch_seed)


# ---- encoder.hidden.0.weight per input column: the one tensor whose operand path is new (read from the stash block, not from x) ----
COLUMN_TENSOR = "encoder.hidden.0.weight"
COLUMN_CASES = [((3, 17, (129, 127)), 1, 1), ((3, 17, (129, 127)), 50, 1), ((513, 128, (512, 512)), 1, 1), ((513, 128, (512, 512)), 50, 1),
                ((513, 64, (16, 16)), 1, 1), ((513, 64, (16, 16)), 50, 1), ((3, 17, (129, 127)), 50, 4)]      # (case, B, ksplit)


@functools.lru_cache(maxsize=None)
def column_bound(case, B, ksplit):
    """(worst, median) bound of tests/grad_columns.py for COLUMN_TENSOR and its float64 truth: MARGIN x the larger figure of the float32
    restatement of this step in the two summation orders of tests/grad_columns_generic.py (numpy's, and the kernels' k-steps through
    its hook).  No device figure enters."""
    import contextlib

    import grad_columns_generic as gcg
    G = truth(case, B)[1][0][COLUMN_TENSOR]
    p, xn, x, y, eps = cast_inputs(case, B, np.float32)
    draws = []
    for order in gcg.ORDERS:
        hook = gcg.StepOrderF32(gcg.slice_plan(B, ksplit)[0], case[1]) if order == "k-steps" else None
        with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
            g = loss_and_grads(tc.model_of(case), p, xn, x, y, eps)[1][COLUMN_TENSOR]
        draws.append(gcg.column_figures(np.asarray(g, np.float64), G))
    return gcg.bound(gcg.merge_figures(*draws)), G

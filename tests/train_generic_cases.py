"""The geometry cases, inputs, float64 truths and bars of the generic fused train step (csrc/train_generic.hip;
disentangled-vae_amd/trainer_generic.py), shared by tests/test_train_generic_cpu.py and tests/test_gpu_train_generic.py.  No GPU here.

Cases: those of the generic encoder (tests/mlp_generic_cases.py: every limit, sizes off every multiple of 4 and 16, (0, 1, (1, 1)), the
reference geometry) plus an M2 with seven labels at the reference widths, which the resident step refuses.
Inputs: gu.make_params(model, dims, 11), gu.make_batch(dims, B, 12).  Truth: oracle.vae_oracle in float64.
Bars: the project's fp32 bar of the fused step (tests/test_gpu_fused.py: test_fused_step_vs_oracle) -- losses 1e-4 relative, every
gradient tensor 1e-4 of its maximum.  tests/test_train_generic_cpu.py shows what float32 arithmetic itself needs of them."""
import functools

import numpy as np

import golden_util as gu
from mlp_generic_cases import ENCODER_CASES
from oracle import vae_oracle as vo

CASES = list(ENCODER_CASES) + [(7, 16, (128, 128))]
PARAM_SEED, BATCH_SEED = 11, 12
BATCHES = (1, 50)                      # one frame; three tiles and a ragged fourth
LOSS_RTOL = 1e-4
GRAD_TOL = 1e-4                        # of the tensor's largest gradient
LR_TRAJ, STEPS_TRAJ, B_TRAJ = 1e-2, 3, 50
LOOPS_CASE = (1, 5, (48, 200))


def case_id(case):
    y, z, (h1, h2) = case
    return f"y{y}_z{z}_h{h1}x{h2}"


def model_of(case):
    return "M1" if case[0] == 0 else "M2"


def dims_of(case):
    y, z, h = case
    return dict(x_dim=513, y_dim=y, z_dim=z, h_dim=tuple(h))


@functools.lru_cache(maxsize=None)
def inputs(case, B, batch_seed=BATCH_SEED):
    """(params, x, y, eps) in float32; shared, never written."""
    dims = dims_of(case)
    params = gu.make_params(model_of(case), dims, PARAM_SEED)
    x, y, eps = gu.make_batch(dims, B, batch_seed)
    for a in list(params.values()) + [x, eps] + ([y] if y is not None else []):
        a.setflags(write=False)
    return params, x, y, eps


def _cast(case, B, dtype, batch_seed=BATCH_SEED):
    params, x, y, eps = inputs(case, B, batch_seed)
    f = lambda a: None if a is None else a.astype(dtype)
    return {k: f(v) for k, v in params.items()}, f(x), f(y), f(eps)


def run(case, B, dtype, steps=1, lr=1e-4, batch_seed=BATCH_SEED):
    """`steps` oracle train steps on the same batch in `dtype`: ([(loss, recon, kl)], [grads], params after)."""
    p, x, y, eps = _cast(case, B, dtype, batch_seed)
    opt = vo.AdamState(list(p))
    losses, grads = [], []
    for _ in range(steps):
        out, g = vo.train_step_vae(model_of(case), p, opt, x, y, eps, lr=lr)
        losses.append(np.array([out["loss"], out["recon"], out["kl"]], np.float64))
        grads.append({k: np.asarray(v, np.float64).reshape(p[k].shape) for k, v in g.items()})
    return losses, grads, p


@functools.lru_cache(maxsize=None)
def truth(case, B, steps=1, lr=1e-4, batch_seed=BATCH_SEED):
    return run(case, B, np.float64, steps, lr, batch_seed)


def loss_err(got, ref):
    """Worst relative error of (ELBO, recon, KL)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def grad_err(got, ref):
    """Worst error of a gradient tensor over that tensor's largest gradient, and the tensor's name."""
    worst, name = 0.0, None
    for k, r in ref.items():
        e = float(np.max(np.abs(np.asarray(got[k], np.float64).reshape(r.shape) - r)) / (np.max(np.abs(r)) + 1e-300))
        if not np.isfinite(e) or e >= worst:
            worst, name = e, k
    return worst, name


def loops_batch(plan_of):
    """The smallest batch of the ladder at which the plan of LOOPS_CASE strides its rows grid over more tiles than it has workgroups and
    cuts the frames into at least two slices, the last one shorter.  plan_of(B) -> the library's plan."""
    for tiles in (8, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        B = 16 * tiles + 16 * 3 + 5
        p = plan_of(B)
        if -(-B // 16) > p.rows_grid and p.ksplit >= 2 and B % p.slice_frames != 0 and (p.ksplit - 1) * p.slice_frames < B:
            return B, p
    raise AssertionError("no batch of the ladder makes the rows kernel stride and the frames split")

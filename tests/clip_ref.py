"""Truth of the clipped optimizer step of the any-size train steps (include/dvae_train.h: dvae_train_*_apply_flat_clipped;
tests/test_train_clip_cpu.py, tests/test_gpu_train_clip.py): the documented semantics restated in numpy on float64 copies.  Nothing
here is fitted to what the code under test returns.

    s          = sum over all tensors of G[i]^2                  G = the float32 flat gradient, squared and summed in float64
    total_norm = |gs| sqrt(s)                                    gs = the step's grad_scale
    coef       = min(1, max_norm / (total_norm + 1e-6))          torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2)
    gscale_eff = fl32(gs coef)                                   formed in double, rounded once
    p', m', v' = oracle.vae_oracle.adam_step on g = G gscale_eff
    s not finite: p, m, v unchanged, coef = 0, total_norm as it came out (inf or NaN), the step counts as skipped.

`scale_dtype` is the one thing a caller chooses: numpy.float32 is the device's contract (the scale travels as the float32 the apply
kernel multiplies by); numpy.float64 leaves the product unrounded, which is clip_grad_norm_ followed by torch.optim.Adam in float64 --
the form tests/test_train_clip_cpu.py holds against torch.  The two differ by the one rounding, at most 2^-24 relative."""
import math

import numpy as np

from oracle import vae_oracle as vo

NORM_EPS = 1e-6          # clip_grad_norm_'s


def sum_squares(grads):
    """s over a list of arrays (any shapes), float64."""
    with np.errstate(all="ignore"):
        return float(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads))


def clip_scale(grads, grad_scale, max_norm, scale_dtype=np.float32):
    """dict(s, total_norm, coef, gscale_eff, skipped) for the gradient tensors `grads`."""
    s = sum_squares(grads)
    gs = float(grad_scale)
    with np.errstate(all="ignore"):
        total_norm = float(abs(gs) * np.sqrt(np.float64(s)))
    if not math.isfinite(s):
        return dict(s=s, total_norm=total_norm, coef=0.0, gscale_eff=0.0, skipped=True)
    coef = min(1.0, float(max_norm) / (total_norm + NORM_EPS))
    return dict(s=s, total_norm=total_norm, coef=coef, gscale_eff=float(scale_dtype(gs * coef)), skipped=False)


def clipped_step(p, m, v, grads, hyper, grad_scale, max_norm, scale_dtype=np.float32):
    """One clipped Adam step over lists of tensors p, m, v, grads (hyper = (t, lr, b1, b2, eps)).  Returns (p', m', v', info) as
    lists of float64 arrays and clip_scale's dict; a skipped step returns float64 copies of the inputs."""
    t, lr, b1, b2, eps = hyper[:5]
    f = lambda a: np.asarray(a).astype(np.float64)
    info = clip_scale(grads, grad_scale, max_norm, scale_dtype)
    if info["skipped"]:
        return [f(a) for a in p], [f(a) for a in m], [f(a) for a in v], info
    out = [vo.adam_step(f(pi), f(gi) * info["gscale_eff"], f(mi), f(vi), t, lr, b1, b2, eps) for pi, mi, vi, gi in zip(p, m, v, grads)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], info

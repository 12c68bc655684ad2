"""Global-norm gradient clipping on the device for the fused train steps of any covered size (include/dvae_train.h:
dvae_train_*_apply_flat_clipped; csrc/train_tables.hip: train_generic_gradnorm_kernel, train_generic_apply_clipped_kernel): what
GenericTrainer, ClassifierTrainer and InfoTrainer share.  The semantics are torch.nn.utils.clip_grad_norm_(parameters, max_norm) over all
tensors of the plan at once; a gradient whose sum of squares is not finite skips the update and is counted (DESIGN 4a'''').  The state
-- scratch of the norm launch, [total_norm, coef], the skip counter, the flat gradient of step(max_norm=...) -- lives in the trainer's
`_shared`, so a trainer and its forks report the same.  No host sync anywhere but in skipped_step_count()."""
import ctypes
import math

import torch

from . import native as N


def check_max_norm(max_norm):
    """max_norm as a float; ValueError unless it is a positive number (+inf is legal: it clips nothing).  Host logic only."""
    m = float(max_norm)
    if math.isnan(m) or m <= 0.0:
        raise ValueError(f"max_norm must be a positive number (+inf clips nothing), got {max_norm!r}")
    return m


def state(tr):
    """The clip state of `tr` and its forks, allocated on first use."""
    st = tr._shared.get("clip")
    if st is None:
        P = int(tr.plan.n_params)
        nbytes = int(tr.lib.dvae_train_gradnorm_scratch_bytes(P))
        if nbytes <= 0:
            N.check(1, "dvae_train_gradnorm_scratch_bytes")
        with torch.cuda.device(tr.device):
            st = {"scratch": torch.zeros(nbytes // 8, dtype=torch.float64, device=tr.device),
                  "grad_norm": torch.zeros(2, dtype=torch.float32, device=tr.device),
                  "skipped": torch.zeros(1, dtype=torch.int32, device=tr.device),
                  "flat": None}
        tr._shared["clip"] = st
    return st


def step_flat(tr):
    """The private flat gradient of step(max_norm=...)."""
    st = state(tr)
    if st["flat"] is None:
        st["flat"] = torch.zeros(int(tr.plan.n_params), dtype=torch.float32, device=tr.device)
    return st["flat"]


def apply_flat_clipped(tr, kind, flat, grad_scale, max_norm):
    """One clipped Adam step on g = grad_scale * flat (norm launch + guarded apply launch); counts as a step exactly as step() does,
    also when the device skips it: the host cannot know without a sync."""
    max_norm = check_max_norm(max_norm)
    st = state(tr)
    tr._sync_copies()                                     # a skipped step rewrites no packed copy: they must be current before it
    tr.step_count += 1
    tr._shared["version"] += 1
    tr._copy_version = tr._shared["version"]
    name = f"dvae_train_{kind}_apply_flat_clipped"
    with torch.cuda.device(tr.device):
        N.check(getattr(tr.lib, name)(ctypes.byref(tr.plan), N.ptr(tr._params), N.ptr(tr._m), N.ptr(tr._v), N.ptr(tr.ws), N.ptr(flat),
                                      tr.step_count, tr.lr, tr.betas[0], tr.betas[1], tr.adam_eps, float(grad_scale), max_norm,
                                      N.ptr(st["scratch"]), N.ptr(st["grad_norm"]), N.ptr(st["skipped"]), N.stream()), name)


def skipped_step_count(tr):
    """Clipped steps the device skipped (non-finite gradient) since the last call (synchronises)."""
    st = tr._shared.get("clip")
    if st is None:
        return 0
    n = int(st["skipped"].item())
    if n:
        st["skipped"].zero_()
    return n

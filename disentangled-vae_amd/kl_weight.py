"""The weighted KL term of the fused any-size train steps (GenericTrainer, InfoTrainer; include/dvae_train.h: kl_weight / kl_floor of the
plan structs): a beta-VAE weight, a linear warm-up over the first optimizer steps, and free bits per element.

With k_bj = -0.5 (lv_bj - mu_bj^2 - exp(lv_bj)) the element of the reference's KL (packages/models/utils.py: it has no "+1", so its
minimum is 0.5), the objective of the VAE body is

    loss = recon + w * mean_b sum_j max(k_bj, kl_floor)

with torch.clamp(k, min=kl_floor)'s gradient (it passes where k >= kl_floor and is exactly 0 below; kl_floor <= 0.5 clamps nothing).
The weight of optimizer step s (1-based: the trainer's step_count after the step) is

    w_s = kl_weight * min(1, s / kl_warmup)    for kl_warmup > 0, else kl_weight

formed here in double and rounded to float32 once -- no device read-back, no sync.  All micro-batches of an accumulated step use the
weight of the step they end in; a skipped (clipped, non-finite) step advances the schedule as it advances step_count; evaluate() uses
the target kl_weight without warm-up.  The recon and KL slots of the reported scalars stay the raw, unweighted, unclamped means.

This is the per-element form of free bits.  The batch-mean form needs a reduction over the whole batch between the forward and the
backward pass; it stays with the autograd path (module_path.py), where it is a line of torch.  Host logic only."""
import math
import operator

import numpy as np


def check_options(kl_weight=1.0, kl_warmup=0, kl_floor=0.0, who="kl_weight"):
    """(kl_weight, kl_warmup, kl_floor) as (float, int, float); ValueError for a negative or non-finite weight or floor and for a
    negative or non-integer warm-up."""
    out = []
    for name, v in (("kl_weight", kl_weight), ("kl_floor", kl_floor)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}") from None
        if isinstance(v, bool) or not math.isfinite(f) or f < 0.0:
            raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}")
        out.append(f)
    try:
        if isinstance(kl_warmup, (bool, float)) and not (isinstance(kl_warmup, float) and kl_warmup.is_integer()):
            raise TypeError
        n = operator.index(int(kl_warmup) if isinstance(kl_warmup, float) else kl_warmup)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{who}: kl_warmup must be an integer number of optimizer steps >= 0, got {kl_warmup!r}") from None
    if n < 0:
        raise ValueError(f"{who}: kl_warmup must be an integer number of optimizer steps >= 0, got {kl_warmup!r}")
    return out[0], int(n), out[1]


def is_default(kl_weight=None, kl_warmup=None, kl_floor=None):
    """Whether the three options (None: not given) are the unweighted step's, which is all the resident step offers."""
    return (kl_weight is None or kl_weight == 1.0) and (kl_warmup is None or kl_warmup == 0) and (kl_floor is None or kl_floor == 0.0)


def weight_at(kl_weight, kl_warmup, step):
    """w_s of optimizer step `step` (1-based) as a Python float that holds a float32 value."""
    w = float(kl_weight)
    if kl_warmup > 0:
        w = w * min(1.0, float(step) / float(kl_warmup))
    return float(np.float32(w))


class KLOptions:
    """What GenericTrainer and InfoTrainer share: the three options, their checks, and the plan fields of a call.  The options live in
    the trainer's `_shared` dict, so a trainer and its forks follow one schedule."""

    def _kl_init(self, kl_weight, kl_warmup, kl_floor, share):
        if share is None:
            self._shared["kl"] = list(check_options(kl_weight, kl_warmup, kl_floor, type(self).__name__))

    def _kl(self):
        return self._shared.setdefault("kl", [1.0, 0, 0.0])       # (a trainer assembled without the constructor: the unweighted step)

    @property
    def kl_weight(self):
        """The target weight of the KL term (reassignable between steps)."""
        return self._kl()[0]

    @kl_weight.setter
    def kl_weight(self, v):
        self._kl()[0] = check_options(v, 0, 0.0, type(self).__name__)[0]

    kl_warmup = property(lambda self: self._kl()[1], doc="Optimizer steps of the linear warm-up (0: none).")
    kl_floor = property(lambda self: self._kl()[2], doc="The floor of a KL element (free bits per element; <= 0.5 clamps nothing).")

    @property
    def kl_weight_next(self):
        """The weight the next optimizer step will use (read-only; float32-valued)."""
        return weight_at(self.kl_weight, self.kl_warmup, self.step_count + 1)

    def _kl_plan(self, step=None):
        """Write the plan fields of a call that belongs to optimizer step `step`; None: the target weight (evaluate())."""
        w, n, lam = self._kl()
        self.plan.kl_weight = float(np.float32(w)) if step is None else weight_at(w, n, step)
        self.plan.kl_floor = lam

"""Steps two and three of a train step held to step one's bounds: the references of a step that starts from GIVEN parameters, moments
and step number (numpy only; tests/test_later_steps_cpu.py and tests/test_gpu_train_later_steps.py use it).

Every gradient check of the suite starts from a fresh trainer; the state a trainer carries into its next step -- both packed weight
copies the apply kernels rewrite, m, v, step_count, the version protocol between a trainer and its forks -- is read by no assertion
that could tell a fresh value from the previous step's.  Adam is sign-like in its first steps, so two correct implementations leave
each other after one update and a fixed trajectory cannot be held tightly.  Each step is therefore judged ON ITS OWN INPUTS: the truth
of step k is the float64 oracle at the parameters the device itself reports before step k, on that step's batch; the update of step k
is adam_bounds.truth on the p, m, v read before it and the gradient the device reports.  No bound is new:

  reference_at   grad_columns_generic.Reference (truth, the two float32 restatements, column and row figures) on given float32
                 parameters and frames; check(grads, ref) is grad_columns_generic.check unchanged (MARGIN 4, floor 2^-24).
                 kind "norm" is the generic step with a standardised encoder input (std_norm_cases: the pool's statistics).
  frames_at      the ReLU nets' frame selection (train_classifier_cases, train_info_cases) evaluated at the parameters in force: the
                 first B passing frames of pool(case, B, batch_seed); that B frames pass is asserted (a condition of the inputs).
  oracle_step    losses, gradients (and the classifier's counts) of one step of a kind in a dtype.
  adam_figures   adam_bounds.ratios over truth / bounds (SLACK 2) for p, m, v: the worst ratio per output.
  stale_ratio    how far a gradient computed on OTHER parameters lies from the column bound of this step's reference: per tensor the
                 smaller of (worst column / its bound, median column / its bound), then the smallest over the tensors.  With the
                 float64 gradient at the previous step's parameters it is the premise that a stale weight copy would be seen; no
                 device figure enters it.
"""
import contextlib

import numpy as np

import adam_bounds as ab
import grad_columns_generic as gg
import std_norm_cases as sn
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic
import train_info_modes_cases as mc
from oracle import vae_oracle as vo

LR = 1e-3                              # a step moves a typical weight (|w| ~ 0.01 .. 0.1) by 1 to 10 %
STEPS = 3
STALE_MIN = 100.0                      # the premise: a gradient on the previous step's parameters is at least this many bounds away
CASES_MOD = {"generic": gc, "norm": gc, "clf": cc, "info": ic}


def case_label(kind, case, mode, B, ksplit=1, micro=None):
    s = f"{kind} {CASES_MOD[kind].case_id(case)}"
    if kind == "info" and mode not in (None, gg.DEFAULT_MODE):
        s += " " + mc.mode_id(mode)
    return s + f" B{B}" + (f" ksplit{ksplit}" if ksplit not in (0, 1) else "") + (" micro " + "+".join(map(str, micro)) if micro else "")


def _cast(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


def _norm_step(case, params, x, y, e, dtype, hook=None):
    """std_norm_cases.run's loop body on given parameters: xn32 from the pool's statistics, then everything in `dtype`."""
    xn = sn.normalise(x, *sn.stats(case))
    p = {k: _cast(v, dtype) for k, v in params.items()}
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
        losses, g = sn.loss_and_grads(gc.model_of(case), p, _cast(xn, dtype), _cast(x, dtype), _cast(y, dtype), _cast(e, dtype))
    return losses, {k: np.asarray(v, np.float64).reshape(params[k].shape) for k, v in g.items()}


def oracle_step(kind, case, mode, params, x, y, e, dtype=np.float64):
    """(losses, grads, counts) of one step of the cases module's own oracle on given parameters and frames: losses as the trainer of
    the kind reports them (3 / 1 / 7 scalars, float64), counts None but for the classifier."""
    if kind == "generic":
        p = {k: _cast(v, dtype) for k, v in params.items()}
        out, g = vo.train_step_vae(gc.model_of(case), p, vo.AdamState(list(p)), _cast(x, dtype), _cast(y, dtype), _cast(e, dtype))
        return (np.array([out["loss"], out["recon"], out["kl"]], np.float64),
                {k: np.asarray(v, np.float64).reshape(params[k].shape) for k, v in g.items()}, None)
    if kind == "norm":
        return _norm_step(case, params, x, y, e, dtype) + (None,)
    if kind == "clf":
        losses, grads, counts, _ = cc.run_on(params, x, y, dtype)
        return np.array([losses[0]], np.float64), grads[0], counts[0]
    if mode in (None, gg.DEFAULT_MODE):
        losses, grads = ic.run_on(params, x, y, e, dtype)[:2]
    else:
        losses, grads = mc.run_on(params, x, y, e, dtype, tuple(mode))[:2]
    return losses[0], grads[0], None


def loss_err(kind, mode, got, want):
    """The cases module's own loss figure (held to its LOSS_RTOL)."""
    if kind == "clf":
        return cc.loss_err(np.asarray(got).reshape(-1)[0], np.asarray(want).reshape(-1)[0])
    if kind == "info":
        return ic.loss_err(got, want) if mode in (None, gg.DEFAULT_MODE) else mc.loss_err(got, want)
    return gc.loss_err(np.asarray(got)[:3], want)


def loss_rtol(kind):
    return CASES_MOD[kind].LOSS_RTOL


class _NormReference(gg.Reference):
    def run(self, frames, dtype, hook=None):
        sub = lambda a: None if a is None else a[frames]
        return _norm_step(self.key[1], self.params, sub(self.x), sub(self.y), sub(self.e), dtype, hook)[1]


def reference_at(kind, case, mode, params, x, y, e, ksplit, micro=None):
    """grad_columns_generic.Reference of one step on the given float32 parameters and frames."""
    B = int(x.shape[0])
    label = case_label(kind, case, mode, B, ksplit, micro)
    if kind == "norm":
        return _NormReference.at("norm", case, None, params, x, y, e, ksplit, micro, label)
    return gg.Reference.at(kind, case, mode, params, x, y, e, ksplit, micro, label)


def check(grads, ref, label=None, quiet=False):
    return gg.check(grads, ref, label, quiet=quiet)


def frames_at(kind, case, params, B, batch_seed):
    """(x, y, eps) of B frames for a step that starts from `params`: the batch of the cases module drawn with `batch_seed`; for the ReLU
    nets the first B frames of its pool that pass the selection under `params` in the float64 oracle."""
    if kind in ("generic", "norm"):
        return gc.inputs(case, B, batch_seed)[1:]
    if kind == "clf":
        x, y = cc.pool(case, B, batch_seed)
        e, ok = None, cc.frames_ok(params, x)
    else:
        x, y, e = ic.pool(case, B, batch_seed)
        ok = ic.frames_ok(params, x, e)
    idx = np.flatnonzero(ok)
    assert idx.size >= B, f"{case_label(kind, case, None, B)} seed {batch_seed}: only {idx.size} of {x.shape[0]} pool frames pass the selection"
    return tuple(None if a is None else np.ascontiguousarray(a[idx[:B]]) for a in (x, y, e))


def flat(tensors, names=None):
    """the tensors of a dict as one vector, in the order of `names` (default: the dict's)"""
    return np.concatenate([np.asarray(tensors[k]).reshape(-1) for k in (tensors if names is None else names)])


def adam_figures(p0, m0, v0, g, p1, m1, v1, hyper, grad_scale=1.0):
    """Worst |got - float64| / bound of the update (p0, m0, v0, g) -> (p1, m1, v1) under hyper = (t, lr, b1, b2, eps): dict p, m, v.
    g is the float32 gradient before grad_scale, as adam_bounds takes it."""
    want = ab.truth(p0, m0, v0, g, hyper, grad_scale)
    bnd = ab.bounds(p0, m0, v0, g, hyper, grad_scale)
    return {n: float(np.max(ab.ratios(got, w, b))) for n, got, w, b in zip("pmv", (p1, m1, v1), want, bnd)}


def stale_ratio(ref_now, grads_before):
    """See the module docstring.  Tensors without a live column (a truth that is identically zero) have no figure and take no part."""
    worst = np.inf
    for k, G in ref_now.truth.items():
        if not np.any(G):
            continue
        f = gg.column_figures(grads_before[k], G)
        bw, bm = gg.bound(ref_now.figures[k])
        worst = min(worst, f["worst"] / bw, f["median"] / bm)
    return float(worst)

"""The float64 truth of the fused any-size train steps under a weighted KL term (kl_weight / kl_warmup / kl_floor:
disentangled-vae_amd/kl_weight.py; csrc/train_generic.hip and csrc/train_info.hip, the KLW instantiations of the rows kernels), shared
by tests/test_kl_weight_cpu.py and tests/test_gpu_train_kl_weight.py.  No GPU here.

With k_bj = -0.5 (lv_bj - mu_bj^2 - exp(lv_bj)) the objective is recon + w mean_b sum_j max(k_bj, lam), with torch.clamp's gradient.
The truth is composed from the pieces of oracle.vae_oracle the way tests/std_norm_cases.py composes its own -- encoder_fwd, decoder_fwd,
elbo, elbo_bwd, decoder_bwd, encoder_bwd -- with the two KL gradients of elbo_bwd scaled by w and masked by k >= lam before
encoder_bwd, and the objective formed from the element terms.  M2_info: the composition of tests/train_info_modes_ref.py (the default
mode is oracle.vae_oracle.m2info_losses_and_grads statement for statement) with the same two pieces in the place of elbo / elbo_bwd.

Cases, inputs, bars: tests/train_generic_cases.py (CASES, BATCHES, LOSS_RTOL, GRAD_TOL); M2_info: tests/train_info_modes_cases.py's
cases and tests/train_info_cases.py's inputs, for the modes (truth, bce) and (classifier, entropy).

The floor lam* of a (case, batch) is chosen so that float32 and float64 can agree on the mask -- a condition of the inputs, not a
measurement of the code under test: the float64 k_bj of the batch are sorted, and lam* is the midpoint of the widest gap between
neighbours inside the middle fifth of the sorted values.  floors() asserts that half that gap is at least GAP_FACTOR = 100 times the
largest |k32 - k64| of the float32 restatement of the encoder on the case, and for B = 50 that at least a tenth of the elements lie on
each side.  A batch with fewer than five elements (B 1 at z 1) has no middle fifth: it gets two floors, k / 2 (nothing clamped) and
2 k (everything clamped).  Every listed case meets both conditions with the committed seeds (tests/test_kl_weight_cpu.py:
test_floor_conditions), but for one: the M2_info case (513, 128, (512, 512)) at B 50 has a half-gap of only 48 k-errors under batch
seed 12, so this file draws that one batch with INFO_BATCH_SEED: seed 23, the first above 12 whose pool passes the frame selection of
tests/train_info_cases.py (14 .. 22 do not) and meets the conditions (13 gives 68 k-errors, 23 gives 137)."""
import contextlib
import functools

import numpy as np

import std_norm_cases as sc
import train_generic_cases as tc
import train_info_cases as ic
import train_info_modes_cases as mc
import train_info_modes_ref as mr
from oracle import vae_oracle as vo

CASES, BATCHES, LOSS_RTOL, GRAD_TOL, LOOPS_CASE = tc.CASES, tc.BATCHES, tc.LOSS_RTOL, tc.GRAD_TOL, tc.LOOPS_CASE
INFO_CASES = mc.CASES
INFO_MODES = [("truth", "bce"), ("classifier", "entropy")]
NORM_CASE = (3, 17, (129, 127))                          # the one std_norm case
GAP_FACTOR = 100.0
INFO_BATCH_SEED = {((513, 128, (512, 512)), 50): 23}     # (case, B) -> batch seed, where ic.BATCH_SEED misses the gap condition
# (w, floor): "*" is lam* of the (case, batch)
SETTINGS = [(0.25, 0.0), (4.0, 0.0), (1.0, "*"), (0.5, "*")]
COLUMN_TENSORS = ("encoder.sample.mu.weight", "encoder.sample.mu.bias", "encoder.sample.log_var.weight", "encoder.sample.log_var.bias",
                  "encoder.hidden.1.weight")             # the tensors the KL gradient reaches first


def setting_id(s):
    return f"w{s[0]:g}_floor{'star' if s[1] == '*' else format(s[1], 'g')}"


# ---- the two pieces that change ----
def k_elements(mu, lv):
    return -0.5 * (lv - mu ** 2 - np.exp(lv))


def elbo_w(x, r, mu, lv, eps, w, lam):
    """(objective, recon, KL): recon and KL are vo.elbo's, raw."""
    _, recon, kl = vo.elbo(x, r, mu, lv, eps)
    dt = mu.dtype.type
    return recon + dt(w) * np.mean(np.sum(np.maximum(k_elements(mu, lv), dt(lam)), axis=-1)), recon, kl


def elbo_bwd_w(x, a, mu, lv, w, lam):
    da, dmu, dlv = vo.elbo_bwd(x, a, mu, lv)
    dt = mu.dtype.type
    mask = (k_elements(mu, lv) >= dt(lam)).astype(mu.dtype)
    return da, dmu * dt(w) * mask, dlv * dt(w) * mask


# ---- M1 / M2 ----
def loss_and_grads(model, params, x, y, eps_noise, w, lam, xn=None, eps=1e-8):
    """One loop body in the dtype of the arguments: (objective, recon, kl), grads.  xn: the standardised encoder input (std_norm)."""
    xe = x if xn is None else xn
    enc = vo.encoder_fwd(params, "encoder.", xe if model == "M1" else np.concatenate([xe, y], axis=1), eps_noise)
    dec = vo.decoder_fwd(params, "decoder.", enc["z"] if model == "M1" else np.concatenate([enc["z"], y], axis=1))
    losses = elbo_w(x, dec["r"], enc["mu"], enc["lv"], eps, w, lam)
    grads = {}
    da, dmu_kl, dlv_kl = elbo_bwd_w(x, dec["a"], enc["mu"], enc["lv"], w, lam)
    ddec_in = vo.decoder_bwd(params, grads, "decoder.", dec, da)
    vo.encoder_bwd(params, grads, "encoder.", enc, ddec_in[:, :enc["z"].shape[1]], dmu_kl, dlv_kl, need_dx=False)
    return np.array(losses, np.float64), {k: np.asarray(v, np.float64).reshape(params[k].shape) for k, v in grads.items()}


def cast_inputs(case, B, dtype, norm=False):
    """(params, x, y, eps, xn) in `dtype`; xn None without std_norm."""
    if norm:
        p, xn, x, y, e = sc.cast_inputs(case, B, dtype)
        return p, x, y, e, xn
    return tc._cast(case, B, dtype) + (None,)


def run(case, B, dtype, w, lam, norm=False, hook=None):
    p, x, y, e, xn = cast_inputs(case, B, dtype, norm)
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
        return loss_and_grads(tc.model_of(case), p, x, y, e, w, lam, xn)


@functools.lru_cache(maxsize=None)
def truth(case, B, w, lam, norm=False):
    return run(case, B, np.float64, w, lam, norm)


# ---- M2_info ----
def info_inputs(case, B):
    """(params, x, y, eps) in float32: tests/train_info_cases.py's selected frames, under this file's batch seed."""
    return ic.inputs(case, B, INFO_BATCH_SEED.get((case, B), ic.BATCH_SEED))


def info_run(case, B, dtype, mode, w, lam):
    """(7 losses, grads) of one M2_info step in `dtype`: train_info_modes_ref.losses_and_grads with the weighted pieces in the place of
    vo.elbo / vo.elbo_bwd while it runs (they call the originals)."""
    params, x, y, e = info_inputs(case, B)
    p = {k: v.astype(dtype) for k, v in params.items()}
    a, b, g = ic.WEIGHTS
    elbo, elbo_bwd = vo.elbo, vo.elbo_bwd

    def ew(x_, r, mu, lv, eps):
        _, recon, kl = elbo(x_, r, mu, lv, eps)
        dt = mu.dtype.type
        return recon + dt(w) * np.mean(np.sum(np.maximum(k_elements(mu, lv), dt(lam)), axis=-1)), recon, kl

    def ebw(x_, a_, mu, lv, scale=1.0):
        da, dmu, dlv = elbo_bwd(x_, a_, mu, lv, scale)
        dt = mu.dtype.type
        mask = (k_elements(mu, lv) >= dt(lam)).astype(mu.dtype)
        return da, dmu * dt(w) * mask, dlv * dt(w) * mask

    vo.elbo, vo.elbo_bwd = ew, ebw
    try:
        out, g1, g2 = mr.losses_and_grads(p, x.astype(dtype), y.astype(dtype), e.astype(dtype), a, b, g, eps=ic.ELBO_EPS, dec_label=mode[0],
                                          aux_enc=mode[1])
    finally:
        vo.elbo, vo.elbo_bwd = elbo, elbo_bwd
    return ic.losses_of(out), ic.step_grads(p, g1, {k: g1[k] + g2[k] for k in g2})


@functools.lru_cache(maxsize=None)
def info_truth(case, B, mode, w, lam):
    return info_run(case, B, np.float64, mode, w, lam)


# ---- the floor ----
def _k_of(kind, case, B, dtype, norm=False):
    if kind == "info":
        params, x, _, e = info_inputs(case, B)
        p = {k: v.astype(dtype) for k, v in params.items()}
        enc = vo.encoder_fwd(p, ic.ENC, x.astype(dtype), e.astype(dtype))
    else:
        p, x, y, e, xn = cast_inputs(case, B, dtype, norm)
        xe = x if xn is None else xn
        enc = vo.encoder_fwd(p, "encoder.", xe if tc.model_of(case) == "M1" else np.concatenate([xe, y], axis=1), e)
    return np.asarray(k_elements(enc["mu"], enc["lv"]), np.float64).ravel()


@functools.lru_cache(maxsize=None)
def floor_figures(kind, case, B, norm=False):
    """dict(floors, half_gap, k_err, below, n): the floors of the (case, batch) and the figures of the two conditions."""
    k64, k32 = _k_of(kind, case, B, np.float64, norm), _k_of(kind, case, B, np.float32, norm)
    k_err = float(np.max(np.abs(k32 - k64)))
    s = np.sort(k64)
    n = s.size
    if n < 5:                                           # no middle fifth: nothing clamped, everything clamped
        lo, hi = float(s[0]) / 2, 2 * float(s[-1])
        half = min(float(s[0]) - lo, hi - float(s[-1]))
        return dict(floors=(lo, hi), half_gap=half, k_err=k_err, below=None, n=n)
    i0, i1 = (2 * n) // 5, min(n - 1, -(-(3 * n) // 5))
    gaps = s[i0 + 1:i1 + 1] - s[i0:i1]
    i = i0 + int(np.argmax(gaps))
    lam = 0.5 * (float(s[i]) + float(s[i + 1]))
    return dict(floors=(lam,), half_gap=0.5 * float(s[i + 1] - s[i]), k_err=k_err, below=float(np.mean(k64 < lam)), n=n)


def floors(kind, case, B, norm=False):
    """The floors lam* of the (case, batch): one, or two for a batch of fewer than five elements.  Asserts the conditions."""
    f = floor_figures(kind, case, B, norm)
    assert f["half_gap"] >= GAP_FACTOR * f["k_err"], (kind, case, B, f)
    if B == 50:
        assert f["below"] is not None and 0.1 <= f["below"] <= 0.9, (kind, case, B, f)
    return f["floors"]


def expand(kind, case, B, setting, norm=False):
    """[(w, lam)] of a setting: lam* expands to the floors of the (case, batch)."""
    w, lam = setting
    return [(w, l) for l in floors(kind, case, B, norm)] if lam == "*" else [(w, float(lam))]


# ---- per column (tests/grad_columns_generic.py) ----
@functools.lru_cache(maxsize=None)
def column_bounds(case, B, w, lam, ksplit=1):
    """{tensor: ((worst, median) bound, float64 truth)} for COLUMN_TENSORS: MARGIN x the larger figure of the float32 restatement of
    this step in the two summation orders of tests/grad_columns_generic.py.  No device figure enters."""
    import grad_columns_generic as gcg
    G = truth(case, B, w, lam)[1]
    draws = []
    for order in gcg.ORDERS:
        hook = gcg.StepOrderF32(gcg.slice_plan(B, ksplit)[0], case[1]) if order == "k-steps" else None
        draws.append(run(case, B, np.float32, w, lam, hook=hook)[1])
    return {t: (gcg.bound(gcg.merge_figures(*(gcg.column_figures(d[t], G[t]) for d in draws))), G[t]) for t in COLUMN_TENSORS}

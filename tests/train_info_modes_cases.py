"""The cases, float64 truths and bars of the generic M2_info fused train step under its two options (dec_label, aux_enc:
disentangled-vae_amd/trainer_info.py; csrc/train_info.hip), shared by tests/test_train_info_modes_cpu.py and
tests/test_gpu_train_info_modes.py.  No GPU here.

Cases: six of tests/train_info_cases.py -- label widths off every multiple of 16, the 33-block label tile, the LDS limit, the reference
geometry and the degenerate net.  Modes: the four non-default ones the reference trains with.  Parameters, frames and loss weights are
those of train_info_cases.py, unchanged: the frame selection depends only on the forward passes of the two side nets, which no mode
alters.  Truth: tests/train_info_modes_ref.py in float64.  Bars: train_info_cases.LOSS_RTOL / GRAD_TOL.

enc_loss = ELBO + classif_loss - aux_enc_loss is a difference, and under "uniform" / "entropy" nothing ties the size of beta V to the
ELBO, so its relative error is not bounded by the terms' own.  Where float32 numpy itself needs more than half the bar for it
(ENC_LOSS_BY_TERMS, checked by tests/test_train_info_modes_cpu.py: test_float32_premise), it is compared against
|ELBO| + |classif_loss| + |aux_enc_loss| instead, which is what the arithmetic can hold.  No (case, mode, B) here does: float32 numpy
stays within 1.3e-6 of enc_loss (the smallest |enc_loss| is an eighth of the ELBO), so the set is empty and every loss is held to the
plain relative bar.

Trajectory: as in train_info_cases.py, on the fixed point of traj_frames() run on the mode's own truth.  Frames kept of 50 after three
steps, per case in the order of CASES (tests/test_train_info_modes_cpu.py: test_trajectory_premises):
    lr     (classifier, entropy)      (classifier, bce)          (truth, entropy)           (truth, uniform)
    1e-5   42 36 41  0 32 50          40 38 40  0 37 50          42 34 41  0 33 50          44 34 41  0 37 50
    1e-6   49 50 48 25 48 50          49 50 49 23 48 50          50 50 48 28 48 50          50 50 49 22 48 50
    1e-7   50 50 49 47 50 50          50 50 50 43 50 50          50 50 49 46 50 50          50 50 49 43 50 50
LR_TRAJ = 1e-6 is the largest of the three at which at most a quarter of the (case, mode) pairs keep fewer than three quarters of
their frames (train_info_cases.TRAJ_DROPPED_MAX): 4 of 24, (513, 128, (512, 512)) in every mode, against 11 of 24 at 1e-5.  The float64
losses then move by 5 to 22 bars over the steps at four cases of the six.  A dropped case is still compared, on the frames it keeps."""
import functools

import numpy as np

import train_info_cases as ic
import train_info_modes_ref as mr
from oracle import vae_oracle as vo

CASES = [(1, 5, (48, 200)), (513, 64, (16, 16)), (3, 17, (129, 127)), (513, 128, (512, 512)), (1, 16, (128, 128)), (1, 1, (1, 1))]
MODES = [("classifier", "entropy"), ("classifier", "bce"), ("truth", "entropy"), ("truth", "uniform")]
PRETRAIN = ("classifier", "entropy")   # scripts/training_M2_info_vad_pretrain.py
BATCHES = ic.BATCHES
WEIGHTS = ic.WEIGHTS
LR_CANDIDATES = (1e-5, 1e-6, 1e-7)
LR_TRAJ = 1e-6
# (case, mode, B) at which float32 numpy misses half the bar for enc_loss relative to |enc_loss|
ENC_LOSS_BY_TERMS = frozenset()


def mode_id(mode):
    return f"{mode[0]}-{mode[1]}"


def run_on(params, x, y, eps, dtype, mode, steps=1, lr=1e-4, weights=WEIGHTS):
    """`steps` train steps of the mode's truth on the same batch in `dtype`: what train_info_cases.run_on returns."""
    p = {k: v.astype(dtype) for k, v in params.items()}
    x, y, eps = x.astype(dtype), y.astype(dtype), eps.astype(dtype)
    a, b, g = weights
    opt_edc = vo.AdamState([k for k in p if not k.startswith(ic.AUX)])
    opt_aux = vo.AdamState([k for k in p if k.startswith(ic.AUX)])
    losses, grads, starts = [], [], []
    for _ in range(steps):
        starts.append({k: v.copy() for k, v in p.items()})
        out, g1, _, aux_total = mr.train_step(p, opt_edc, opt_aux, x, y, eps, alpha=a, beta=b, gamma=g, eps=ic.ELBO_EPS, lr=lr,
                                              dec_label=mode[0], aux_enc=mode[1])
        losses.append(ic.losses_of(out))
        grads.append(ic.step_grads(p, g1, aux_total))
    return losses, grads, p, starts


@functools.lru_cache(maxsize=None)
def truth(case, B, mode, steps=1, lr=1e-4, weights=WEIGHTS):
    return run_on(*ic.inputs(case, B), np.float64, mode, steps, lr, weights)


@functools.lru_cache(maxsize=None)
def _traj_idx(case, mode, lr):
    p, x, y, eps = ic.inputs(case, ic.B_TRAJ)
    idx = np.arange(ic.B_TRAJ)
    while idx.size:
        starts = run_on(p, x[idx], y[idx], eps[idx], np.float64, mode, ic.STEPS_TRAJ, lr)[3]
        ok = np.ones(idx.size, bool)
        for s in starts:
            ok &= ic.frames_ok(s, x[idx], eps[idx])
        if ok.all():
            break
        idx = idx[ok]
    idx.setflags(write=False)
    return idx


def traj_frames(case, mode):
    """train_info_cases.traj_frames on the mode's own truth, at LR_TRAJ."""
    idx = _traj_idx(case, mode, LR_TRAJ)
    assert idx.size, f"{ic.case_id(case)} {mode_id(mode)}: no frame passes the selection along the trajectory"
    return idx


def traj_kept(case, mode, lr=LR_TRAJ):
    """Frames of the B_TRAJ that the fixed point keeps at learning rate `lr` (0: none)."""
    return int(_traj_idx(case, mode, lr).size)


def traj_dropped(case, mode, lr=LR_TRAJ):
    return traj_kept(case, mode, lr) < (1 - ic.TRAJ_DROPPED_MAX) * ic.B_TRAJ


@functools.lru_cache(maxsize=None)
def traj_inputs(case, mode):
    p, x, y, eps = ic.inputs(case, ic.B_TRAJ)
    idx = traj_frames(case, mode)
    out = tuple(np.ascontiguousarray(a[idx]) for a in (x, y, eps))
    for a in out:
        a.setflags(write=False)
    return (p,) + out


@functools.lru_cache(maxsize=None)
def traj_truth(case, mode):
    return run_on(*traj_inputs(case, mode), np.float64, mode, ic.STEPS_TRAJ, LR_TRAJ)


def loss_errs(got, ref, by_terms=False):
    """Relative error of each of the seven losses; a loss whose truth is zero must be zero.  by_terms: enc_loss against
    |ELBO| + |classif_loss| + |aux_enc_loss| of the truth."""
    got, ref = np.asarray(got, np.float64)[:7], np.asarray(ref, np.float64)[:7]
    out = []
    for i, (a, r) in enumerate(zip(got, ref)):
        scale = abs(ref[0]) + abs(ref[4]) + abs(ref[6]) if (by_terms and i == 3) else abs(r)
        e = (0.0 if a == 0.0 else float("inf")) if scale == 0.0 else abs(a - r) / scale
        out.append(float(e) if np.isfinite(e) else float("inf"))
    return out


def loss_err(got, ref, by_terms=False):
    return max(loss_errs(got, ref, by_terms))


def by_terms(case, mode, B):
    return (case, mode, B) in ENC_LOSS_BY_TERMS


DEC1 = "enc_dec_clf.decoder.hidden.0.weight"
CLF_WEIGHTS = tuple(ic.CLF + n + ".weight" for n in ("hidden.0", "hidden.1", "output_layer"))


def block_grads(grads, z):
    """The blocks held to GRAD_TOL of their OWN maximum: the label columns of decoder layer 1 and the classifier's three weight
    matrices, so that y read where p_c belongs, or the decoder's term missing in d p_c, cannot hide under a larger neighbour."""
    out = {DEC1 + "[:, z:]": np.asarray(grads[DEC1])[:, z:]}
    out.update({k: np.asarray(grads[k]) for k in CLF_WEIGHTS})
    return out

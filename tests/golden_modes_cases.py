"""The cases of tests/golden/vae_golden_modes.part*.npz (tests/golden/make_golden_modes.py: the reference's own M2_info loop body
under the two options of the fused step), and the replay that holds a step implementation to them with the tolerances
golden_check.check_case uses by default for M2_info.  No GPU here.

(name, dims, B, (dec_label, aux_enc), (alpha, beta, gamma), seed): a small geometry and the reference's, each in the pretrain script's
mode at its own weights, in (classifier, bce) with every term pulling, and in the two other adversarial terms on the true label."""
import numpy as np

import golden_util as gu

STEM = "vae_golden_modes"
_SMALL = dict(x_dim=37, y_dim=3, z_dim=5, h_dim=(12, 9))
_FULL = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
_MODES = [(("classifier", "entropy"), (0.0, 10.0, 10.0)),      # scripts/training_M2_info_vad_pretrain.py
          (("classifier", "bce"), (10.0, 10.0, 1.0)),
          (("truth", "entropy"), (0.5, 10.0, 1.0)),
          (("truth", "uniform"), (0.5, 10.0, 1.0))]
CASES = [(f"{g}_{m[0]}_{m[1]}", dims, B, m, w, 300 + 10 * gi + mi)
         for gi, (g, dims, B) in enumerate([("small", _SMALL, 5), ("full", _FULL, 32)]) for mi, (m, w) in enumerate(_MODES)]


def check_case(step_fn, fix, case, rtol_loss=2e-5, rtol_grad=1e-4, atol_grad=1e-7, atol_rel_grad=1e-5, rtol_param=1e-6, atol_param=2e-7):
    """step_fn(params, opt state or None, x, y, eps, mode, weights) -> (losses7, grads_enc, grads_aux_total, params, state): one train
    step from `params` (dict of arrays, float32 values) carrying `state` between steps."""
    name, dims, B, mode, weights, seed = case
    max_bad_frac = 0.12 if B < 4 else 0.01             # golden_check.check_case at wscale 1
    params = gu.make_params("M2_info", dims, seed, 1.0)
    chk = gu.checksum(params.values())
    cur, state = {k: v.copy() for k, v in params.items()}, None
    for step in range(1, gu.NSTEPS + 1):
        x, y, e = gu.make_batch(dims, B, seed * 1000 + step)
        chk += gu.checksum([x, y, e])
        losses, g_enc, g_aux, cur, state = step_fn(cur, state, x, y, e, mode, weights)
        pre = f"{name}/step{step}"
        np.testing.assert_allclose(np.array(losses, dtype=np.float64), fix[pre + "/losses"], rtol=rtol_loss, atol=1e-6, err_msg=pre + "/losses")
        if step == 1:
            for k in params:
                gu.compare_summary(f"{pre}/grad_enc/{k}", g_enc[k], fix, f"{pre}/grad_enc/{k}", rtol_grad, atol_grad, atol_rel_grad)
                if k.startswith("auxiliary."):
                    gu.compare_summary(f"{pre}/grad_aux_total/{k}", g_aux[k], fix, f"{pre}/grad_aux_total/{k}", rtol_grad, atol_grad, atol_rel_grad)
        if step in (1, gu.NSTEPS):
            for k in params:
                gu.compare_params(f"{pre}/param/{k}", cur[k], fix, f"{pre}/param/{k}", rtol_param, atol_param, max_bad_frac, 1.05e-4 * step)
    assert abs(chk - float(fix[name + "/input_checksum"])) <= 1e-9 * abs(chk), "regenerated inputs differ from the captured ones"

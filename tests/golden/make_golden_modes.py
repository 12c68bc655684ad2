"""Capture golden vectors of the M2_info train step under its two options (dec_label, aux_enc) by running the REFERENCE ITSELF (CPU,
fp32) on deterministic inputs.  Build-container only (imports /root/reference read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_modes.py     # -> vae_golden_modes.part*.npz

The loop body is that of scripts/training_M2_info_vad_pretrain.py:162-200 -- the reference's own DeepGenerativeModel_v5, elbo,
binary_cross_entropy / _v2 / _v3 and stock torch.optim.Adam -- with the two choices the script makes by commenting lines in and out
taken from the case: what the decoder is fed (line 163 or 164) and which adversarial term the encoder gets (line 173, 174 or 175).
Output: data only (inputs are regenerated from seeds by tests/golden_util.py; a checksum of them is stored).  For each case of
golden_util-style tuples in CASES it runs golden_util.NSTEPS steps and stores every loss scalar of every step, the step-1 gradients of
every parameter after enc_loss.backward() and the auxiliary net's after both backward passes, and the parameters after step 1 and
after the last step, summarised with golden_util.summarize.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

import numpy as np
import torch

import golden_util as gu
import golden_modes_cases as gm
from make_golden import model_call, put
from packages.models.models import DeepGenerativeModel_v5
from packages.models.utils import elbo, binary_cross_entropy, binary_cross_entropy_v2, binary_cross_entropy_v3

EPS = 1e-8
LR = 1e-4


def run_case(fix, case):
    name, dims, B, (dec_label, aux_enc), (alpha, beta, gamma), seed = case
    torch.manual_seed(0)
    m = DeepGenerativeModel_v5([dims["x_dim"], dims["y_dim"], dims["z_dim"], list(dims["h_dim"])])
    params = gu.make_params("M2_info", dims, seed, 1.0)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    named = dict(m.named_parameters())
    opt = torch.optim.Adam(m.enc_dec_clf.parameters(), lr=LR, betas=(0.9, 0.999))
    opt_aux = torch.optim.Adam(m.auxiliary.parameters(), lr=LR, betas=(0.9, 0.999))
    chk = gu.checksum(params.values())
    for step in range(1, gu.NSTEPS + 1):
        xn, yn, en = gu.make_batch(dims, B, seed * 1000 + step)
        chk += gu.checksum([xn, yn, en])
        x, y, e = torch.from_numpy(xn), torch.from_numpy(yn), torch.from_numpy(en)
        pre = f"{name}/step{step}"
        y_hat_class_soft = m.classify_fromX(x)
        r, z, mu, lv = model_call(m, "M2_info", x, y_hat_class_soft if dec_label == "classifier" else y, e)
        ELBO, recon, kl = elbo(x, r, mu, lv, EPS)
        classif_loss = alpha * binary_cross_entropy(y_hat_class_soft, y, EPS)
        y_hat_aux_soft = m.classify_fromZ(z)
        if aux_enc == "bce":
            aux_enc_loss = beta * binary_cross_entropy(y_hat_aux_soft, y, EPS)
        elif aux_enc == "uniform":
            aux_enc_loss = beta * binary_cross_entropy_v2(y_hat_aux_soft, EPS)
        else:
            aux_enc_loss = beta * binary_cross_entropy_v3(y_hat_aux_soft, EPS)
        enc_loss = ELBO + classif_loss - aux_enc_loss
        y_hat_aux_soft2 = m.classify_fromZ(z.detach())
        aux_loss = gamma * binary_cross_entropy(y_hat_aux_soft2, y, EPS)
        enc_loss.backward()
        fix[pre + "/losses"] = np.array([ELBO.item(), recon.item(), kl.item(), enc_loss.item(), classif_loss.item(), aux_loss.item(),
                                         aux_enc_loss.item()], dtype=np.float64)
        if step == 1:
            for k, p in named.items():          # everything enc_loss.backward() deposited
                put(fix, f"{pre}/grad_enc/{k}", p.grad.numpy())
        opt.step(); opt.zero_grad()
        aux_loss.backward()
        if step == 1:
            for k, p in named.items():
                if k.startswith("auxiliary."):  # gamma dBCE - beta dV: never zeroed in between
                    put(fix, f"{pre}/grad_aux_total/{k}", p.grad.numpy())
        opt_aux.step(); opt_aux.zero_grad()
        if step in (1, gu.NSTEPS):
            for k, p in named.items():
                put(fix, f"{pre}/param/{k}", p.detach().numpy())
    fix[name + "/input_checksum"] = np.float64(chk)


def main():
    fix = {}
    for case in gm.CASES:
        run_case(fix, case)
        print("captured", case[0])
    print("wrote", ", ".join(gu.save_golden(gm.STEM, fix)), len(fix), "arrays")
    print("torch", torch.__version__, "numpy", np.__version__)


if __name__ == "__main__":
    main()

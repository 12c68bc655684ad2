"""The reference's loop body (scripts/training_M1.py / training_M2.py: module forward, the elbo terms in torch, loss.backward(), stock
torch.optim.Adam) on an M1 / M2 module of ANY covered size, run as one autograd Function per model call on the fused kernels
(disentangled-vae_amd/module_path.py: GenericModuleEngine; forward 2 launches, backward 3).

    python examples/train_script_loop.py --model M2 --synthetic 20000 --z-dim 32 --h-dim 256 64
    # the KL term weighted, and warmed up over the first 200 steps as the reference's DeterministicWarmup does (variational.py:32-48):
    # an objective the fused train step does not have -- here it is three lines of torch on (r, mu, log_var)
    python examples/train_script_loop.py --model M1 --synthetic 20000 --z-dim 32 --h-dim 256 64 --kl-weight 0.25 --warmup 200

    # the M2_info loop bodies (two torch.optim.Adam, the drop-in DeepGenerativeModel_v5): the main script's, scripts/training_M2_info_vad.py:
    # 159-198, and under --decoder-label classifier the pretrain script's, scripts/training_M2_info_vad_pretrain.py:162-200, whose decoder
    # reads the classifier's output, so that the body's label input carries a gradient
    python examples/train_script_loop.py --model M2_info --synthetic 20000 --z-dim 32 --h-dim 256 64
    python examples/train_script_loop.py --model M2_info --y-dim 513 --z-dim 16 --h-dim 128 128 --decoder-label classifier --aux-enc entropy --gamma 10

The script sets the switch itself (DVAE_MODULE_GENERIC=1; `module_path.set_generic(model, "on")` does the same for one module) and prints
which engine the module takes: "generic" here, "resident" at the reference's z 16 / h 128 128, None outside the covered sizes (the
per-layer kernels).  For M2_info the switch is the body's own, module_path.set_info_body(model, "on") (DVAE_MODULE_INFO_BODY=1), and the
classifier and the auxiliary net stay per-layer calls, as the script makes them.  Whoever wants the whole step fused, optimizer included, uses examples/train_fused.py.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("DVAE_MODULE_GENERIC", "1")
module_path = importlib.import_module("disentangled-vae_amd.module_path")
script_loops = importlib.import_module("disentangled-vae_amd.script_loops")
from packages.models.models import DeepGenerativeModel, DeepGenerativeModel_v5, VariationalAutoencoder      # noqa: E402
from packages.models.utils import elbo                                               # noqa: E402


def synthetic(n, y_dim, seed):
    rng = np.random.default_rng(seed)
    scale = np.exp(np.random.default_rng(0).standard_normal((1, 513)) - 1)     # per-bin level
    X = (rng.standard_normal((n, 513)) ** 2 * scale).astype(np.float32)
    Y = (rng.random((n, y_dim)) > 0.5).astype(np.float32) if y_dim else None
    return X, Y


class Warmup:
    """DeterministicWarmup of the reference: t goes from 0 to t_max in n steps, then stays"""

    def __init__(self, n, t_max):
        self.t, self.t_max, self.inc = 0.0, t_max, (t_max / n if n > 0 else t_max)

    def __next__(self):
        self.t = min(self.t_max, self.t + self.inc)
        return self.t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["M1", "M2", "M2_info"], default="M2")
    ap.add_argument("--synthetic", type=int, default=20000, metavar="N", help="frames of synthetic power spectra")
    ap.add_argument("--y-dim", type=int, default=1)
    ap.add_argument("--z-dim", type=int, default=32)
    ap.add_argument("--h-dim", type=int, nargs=2, default=[256, 64])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--kl-weight", type=float, default=1.0, help="weight of the KL term, applied in torch")
    ap.add_argument("--warmup", type=int, default=0, help="steps over which the KL weight rises linearly from 0")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--decoder-label", choices=list(script_loops.DECODER_LABELS), default="truth", help="M2_info: what the decoder reads beside z")
    ap.add_argument("--aux-enc", choices=list(script_loops.AUX_ENCS), default="bce", help="M2_info: the adversarial term on the encoder")
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--beta", type=float, default=10.0)
    ap.add_argument("--gamma", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_script_loop.py needs the MI355X HIP path (no CPU fallback)")
    torch.manual_seed(a.seed)
    if a.model == "M2_info":
        return main_info(a)
    y_dim = a.y_dim if a.model == "M2" else 0
    if a.model == "M1":
        model = VariationalAutoencoder([513, a.z_dim, list(a.h_dim)])
    else:
        model = DeepGenerativeModel([513, y_dim, a.z_dim, list(a.h_dim)], None)
    model.cuda()
    print(f"engine_kind: {module_path.engine_kind(model, a.model)}", flush=True)
    X, Y = synthetic(a.synthetic, y_dim, a.seed)
    X = torch.from_numpy(X).cuda()
    Y = None if Y is None else torch.from_numpy(Y).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=a.lr, betas=(0.9, 0.999))
    beta = Warmup(a.warmup, a.kl_weight)
    for epoch in range(a.epochs):
        t0 = time.time()
        tot = torch.zeros(3, dtype=torch.float64, device="cuda")
        perm = torch.randperm(X.shape[0], device="cuda")
        nb = 0
        for lo in range(0, X.shape[0], a.batch):
            idx = perm[lo:lo + a.batch]
            x, y = X[idx], (None if Y is None else Y[idx])
            r, mu, logvar = model(x) if a.model == "M1" else model(x, y)
            _, recon, KL = elbo(x, r, mu, logvar, 1e-8)
            loss = recon + next(beta) * KL                    # the objective is the script's own: any torch expression of (r, mu, logvar)
            loss.backward()
            opt.step()
            opt.zero_grad()
            tot += torch.stack([loss.detach(), recon.detach(), KL.detach()]).double()
            nb += 1
        torch.cuda.synchronize()
        l, rc, kl = (tot / nb).tolist()
        print(f"epoch {epoch + 1:3d}  loss {l:.3f}  recon {rc:.3f}  KL {kl:.3f}  KL weight {beta.t:.3f}  "
              f"{1e6 * (time.time() - t0) / nb:.0f} us / step", flush=True)


def main_info(a):
    model = DeepGenerativeModel_v5([513, a.y_dim, a.z_dim, list(a.h_dim)]).cuda()
    module_path.set_info_body(model, "on")
    print(f"engine_kind: {module_path.engine_kind(model.enc_dec_clf, 'M2_DEC')}", flush=True)
    X, Y = synthetic(a.synthetic, a.y_dim, a.seed)
    X, Y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    opt_body = torch.optim.Adam(model.enc_dec_clf.parameters(), lr=a.lr, betas=(0.9, 0.999))      # one optimizer per sub-model, as in the scripts
    opt_aux = torch.optim.Adam(model.auxiliary.parameters(), lr=a.lr, betas=(0.9, 0.999))
    names = ("ELBO", "recon", "KL", "enc_loss", "classif_loss", "aux_loss")
    for epoch in range(a.epochs):
        t0 = time.time()
        tot = torch.zeros(len(names), dtype=torch.float64, device="cuda")
        perm = torch.randperm(X.shape[0], device="cuda")
        nb = 0
        for lo in range(0, X.shape[0], a.batch):
            idx = perm[lo:lo + a.batch]
            L = script_loops.info_step(model, opt_body, opt_aux, X[idx], Y[idx], decoder_label=a.decoder_label, aux_enc=a.aux_enc,
                                       alpha=a.alpha, beta=a.beta, gamma=a.gamma)
            tot += torch.stack([L[k] for k in names]).double()
            nb += 1
        torch.cuda.synchronize()
        print(f"epoch {epoch + 1:3d}  " + "  ".join(f"{k} {v:.3f}" for k, v in zip(names, (tot / nb).tolist()))
              + f"  {1e6 * (time.time() - t0) / nb:.0f} us / step", flush=True)


if __name__ == "__main__":
    main()

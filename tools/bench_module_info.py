"""The reference's M2_info loop bodies (disentangled-vae_amd/script_loops.py: the drop-in DeepGenerativeModel_v5, the losses in torch, two
stock torch.optim.Adam) on the MI355X at sizes the resident engine does not serve: microseconds per loop iteration with the body's
switch on (module_path.set_info_body(model, "on"): the body as ONE Function on the generic module engine, label gradient included)
beside the switch off -- the per-layer path such a model takes by default, the behaviour before the engine existed -- and, for context,
InfoTrainer.step on the same model and batch (the whole step fused, both optimizers included, no autograd).

    python tools/bench_module_info.py [--out profiles/module_info.json] [--reps 20] [--batches 128 8192]

Geometries: z 32, h (256, 64), y 1; z 16, h (128, 128), y 513; z 128, h (512, 512), y 513.  Loop bodies: the main script's (decoder on
[z | y], adversarial cross entropy) and the pretrain script's (decoder on [z | classifier(x)], entropy adversary, gamma = beta).  Method
as tools/bench_module_generic.py, whose window loop this imports: the sides take turns in one process, one window each, `--reps` rounds
after a warm-up round; device time from events around a window, wall time from a host clock that stops after the synchronise behind it;
medians with min and max.  Inputs are resident on the device and the noise is passed in.  Before timing, the two module sides are compared
at equal parameters: enc_loss and the largest difference of a gradient tensor over its maximum.
"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from bench_module_generic import alternating
synth = importlib.import_module("disentangled-vae_amd.synth")
mp = importlib.import_module("disentangled-vae_amd.module_path")
loops = importlib.import_module("disentangled-vae_amd.script_loops")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")

SETUPS = [("a", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))), ("b", dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))),
          ("c", dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512)))]
BODIES = [("main", dict(decoder_label="truth", aux_enc="bce", alpha=0.0, beta=10.0, gamma=1.0)),
          ("pretrain", dict(decoder_label="classifier", aux_enc="entropy", alpha=0.0, beta=10.0, gamma=10.0))]


class InfoLoop:
    """One iteration of a loop body on the drop-in _v5 of `dims`; mode: the body's switch, "off" or "on"."""

    def __init__(self, dims, mode, body):
        from packages.models import models as M
        self.M, self.body = M, body
        torch.manual_seed(0)
        self.m = synth.build_model("M2_info", dims).to("cuda")
        mp.set_info_body(self.m, mode)
        self.kind = mp.engine_kind(self.m.enc_dec_clf, "M2_DEC")
        self.opt_body = torch.optim.Adam(self.m.enc_dec_clf.parameters(), lr=1e-4, betas=(0.9, 0.999))
        self.opt_aux = torch.optim.Adam(self.m.auxiliary.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def loss_and_grads(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        L = loops.info_losses(self.m, x, y, **self.body)
        L["enc_loss"].backward()
        g = {k: (torch.zeros_like(p) if p.grad is None else p.grad.clone()) for k, p in self.m.named_parameters()}
        for p in self.m.parameters():
            p.grad = None
        return float(L["enc_loss"].detach()), g

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        return loops.info_step(self.m, self.opt_body, self.opt_aux, x, y, **self.body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "module_info.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    ap.add_argument("--setups", nargs="+", default=[t for t, _ in SETUPS])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_module_info.py measures on the GPU: none found")
    for k in ("DVAE_MODULE_PATH", "DVAE_MODULE_INFO_BODY"):
        os.environ.pop(k, None)
    rows = []
    for tag, dims in SETUPS:
        if tag not in a.setups:
            continue
        for name, body in BODIES:
            for B in a.batches:
                x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
                off, on = InfoLoop(dims, "off", body), InfoLoop(dims, "on", body)
                assert off.kind is None and on.kind == "generic", (off.kind, on.kind)
                la, ga = off.loss_and_grads(x, y, e)
                lb, gb = on.loss_and_grads(x, y, e)
                eng = on.m.enc_dec_clf.__dict__.get("_dvae_engine")
                assert eng is not None and eng.kind == "generic" and off.m.enc_dec_clf.__dict__.get("_dvae_engine") is None
                gdiff = max(float((ga[k] - gb[k]).abs().max() / (ga[k].abs().max() + 1e-30)) for k in ga)
                trainer = TI.make_info_trainer(dims, generic=True, dec_label=body["decoder_label"], aux_enc=body["aux_enc"], batch=B, device="cuda:0",
                                               seed=0, alpha=body["alpha"], beta=body["beta"], gamma=body["gamma"])
                inner = 50 if B <= 1024 else 10
                sides = {"switch_off_per_layer": lambda: off.step(x, y, e), "switch_on_generic_engine": lambda: on.step(x, y, e),
                         "info_trainer_step": lambda: trainer.step(x, y, e)}
                r = alternating(sides, a.reps, inner)
                med = lambda side, clock: r[side][clock]["median"]
                rows.append({"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "loop_body": name, "batch": B,
                             "iterations_per_window": inner, "us_per_iteration": r,
                             "on_over_off_device": round(med("switch_on_generic_engine", "device_us") / med("switch_off_per_layer", "device_us"), 3),
                             "on_over_off_wall": round(med("switch_on_generic_engine", "wall_us") / med("switch_off_per_layer", "wall_us"), 3),
                             "first_enc_loss_off": la, "first_enc_loss_on": lb, "first_gradient_max_rel_diff": gdiff})
                print(json.dumps(rows[-1]), flush=True)
                del off, on, trainer, sides
                torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

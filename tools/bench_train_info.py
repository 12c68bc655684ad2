"""The generic M2_info fused train step (csrc/train_info.hip; trainer_info.InfoTrainer) on the MI355X: microseconds per step beside
the per-layer module path, which was the only way to train such a model before it, and beside the resident step where both exist.

    python tools/bench_train_info.py [--out profiles/train_info.json] [--reps 20] [--batches 128 8192]
    python tools/bench_train_info.py --modes truth-bce classifier-bce classifier-entropy --out profiles/train_info_modes.json

--modes: dec_label-aux_enc pairs of the generic step (trainer_info.InfoTrainer); the default is truth-bce alone, the step of
scripts/training_M2_info_vad.py.  For any other mode the module path runs the loop body of
scripts/training_M2_info_vad_pretrain.py:162-200 with the same two choices, and the weights are that script's (alpha 0, beta = gamma = 10).
The share of the matrix peak counts the default step's products for every mode (the later classifier backward adds y h2 multiply-adds a
frame, the second auxiliary chain y h2 + h2 h1): a lower bound for the others.

Every time is device time from events around 10 steps in a row, the median (with min and max) over `--reps` such windows after a
warm-up window (tools/bench_train_generic.py's method); inputs are resident on the device, the noise is passed in; both sides run on
the same device in the same run.  The loss weights are the script's (alpha 0, beta 10, gamma 1) on both sides.
  a  z 32, h (256, 64), y_dim 1: the model examples/enhance_mcem.py --z-dim 32 --h-dim 256 64 --labels classifier takes.
  b  the reference's geometry (z 16, h (128, 128), y_dim 1): also against Trainer("M2_info", precision="fp32"), the resident step.
  c  z 16, h (128, 128), y_dim 513: IBM labels, which no fused M2_info step took before.
  d  z 128, h (512, 512), y_dim 513: the largest geometry.
Per kernel: mean device time of the three launches of a step from torch.profiler's device activity over 10 steps, and the share of the
157.3 TFLOP/s fp32 matrix peak of the step as a whole."""
import argparse, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
T = importlib.import_module("disentangled-vae_amd.trainer")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
synth = importlib.import_module("disentangled-vae_amd.synth")
INNER, PEAK_FLOPS = 10, 157.3e12


def windows(fn, reps):
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / INNER
    window()
    us = [window() for _ in range(reps)]
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


class ModuleStep:
    """DeepGenerativeModel_v5 of `dims` under torch autograd and two stock torch.optim.Adam (bench.py: ModulesImpl.step; the loop body of
    scripts/training_M2_info_vad.py:159-198)."""

    def __init__(self, dims, dec_label="truth", aux_enc="bce", weights=(0.0, 10.0, 1.0)):
        from packages.models import models as M
        from packages.models import utils as U
        self.M, self.elbo, self.bce = M, U.elbo, U.binary_cross_entropy
        self.dec_label, self.weights = dec_label, weights
        self.v = {"bce": None, "uniform": U.binary_cross_entropy_v2, "entropy": U.binary_cross_entropy_v3}[aux_enc]
        torch.manual_seed(0)
        self.m = synth.build_model("M2_info", dims).to("cuda")
        self.opt = torch.optim.Adam(self.m.enc_dec_clf.parameters(), lr=1e-4, betas=(0.9, 0.999))
        self.opt_aux = torch.optim.Adam(self.m.auxiliary.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        m = self.m
        alpha, beta, gamma = self.weights
        yc = m.classify_fromX(x)
        r, z, mu, lv = m(x, yc if self.dec_label == "classifier" else y)
        ELBO, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        pa = m.classify_fromZ(z)
        enc_loss = ELBO + alpha * self.bce(yc, y, 1e-8) - beta * (self.bce(pa, y, 1e-8) if self.v is None else self.v(pa, 1e-8))
        aux_loss = gamma * self.bce(m.classify_fromZ(z.detach()), y, 1e-8)
        enc_loss.backward()
        self.opt.step(); self.opt.zero_grad()
        aux_loss.backward()
        self.opt_aux.step(); self.opt_aux.zero_grad()
        return ELBO


def flops_per_frame(dims):
    """Forward, weight-gradient and backward-data products of the four nets (2 flops a multiply-add)."""
    y, z, (h1, h2) = dims["y_dim"], dims["z_dim"], dims["h_dim"]
    vae = h1 * 513 + h2 * h1 + 2 * z * h2 + h2 * (z + y) + h1 * h2 + 513 * h1
    vae_dx = h2 * h1 + 2 * z * h2 + z * h2 + h1 * h2 + 513 * h1
    clf, clf_dx = h1 * 513 + h2 * h1 + y * h2, h2 * h1 + y * h2
    aux, aux_dx = h1 * z + h2 * h1 + y * h2, h1 * z + h2 * h1 + y * h2
    return 2.0 * (2 * (vae + clf + aux) + vae_dx + clf_dx + aux_dx)


def kernel_times(fn):
    """Mean device microseconds per launch of every kernel of INNER calls of fn, by kernel name."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(INNER):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t and ev.count and "kernel" in ev.key:
            out[ev.key.split("(")[0].split("::")[-1]] = {"us": round(t / ev.count, 2), "launches_per_step": round(ev.count / INNER, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    ap.add_argument("--modes", nargs="+", default=["truth-bce"], metavar="DEC-AUX", help="dec_label-aux_enc, e.g. classifier-entropy")
    ap.add_argument("--setups", nargs="+", default=["a", "b", "c", "d"])
    ap.add_argument("--no-module-path", action="store_true", help="skip the module-path baseline")
    a = ap.parse_args()
    modes = [tuple(m.split("-")) for m in a.modes]
    for m in modes:
        I.mode_bits(*m)                                   # an unknown option: refused here, with the choices named
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    setups = [("a", dict(ref, z_dim=32, h_dim=(256, 64))), ("b", ref), ("c", dict(ref, y_dim=513)), ("d", dict(ref, y_dim=513, z_dim=128, h_dim=(512, 512)))]
    rows = []
    for B in a.batches:
        for tag, dims, (dec_label, aux_enc) in [(t, d, m) for t, d in setups if t in a.setups for m in modes]:
            default = (dec_label, aux_enc) == ("truth", "bce")
            weights = (0.0, 10.0, 1.0) if default else (0.0, 10.0, 10.0)
            x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
            gen = I.make_info_trainer(dims, generic=True, batch=B, device="cuda:0", seed=0, dec_label=dec_label, aux_enc=aux_enc,
                                      alpha=weights[0], beta=weights[1], gamma=weights[2])
            g = windows(lambda: gen.step(x, y, e), a.reps)
            kern = kernel_times(lambda: gen.step(x, y, e))
            plan = {"launches_per_step": gen.plan.launches_per_step, "lds_bytes": gen.plan.lds_bytes, "rows_grid": gen.plan.rows_grid,
                    "wgrad_items": gen.plan.wgrad_items, "ksplit": gen.plan.ksplit, "workspace_MB": round(gen.plan.workspace_bytes / 2 ** 20, 1)}
            del gen
            row = {"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B,
                   "dec_label": dec_label, "aux_enc": aux_enc, "weights": weights, "generic_us": g,
                   "generic_mfma_fraction_of_157TFLOPs": round(flops_per_frame(dims) * B / (g["median"] * 1e-6) / PEAK_FLOPS, 4),
                   "kernels": kern, "plan": plan}
            if not a.no_module_path:
                mod = ModuleStep(dims, dec_label, aux_enc, weights)
                m = windows(lambda: mod.step(x, y, e), a.reps)
                del mod
                row["module_path_us"], row["generic_over_module_path"] = m, round(g["median"] / m["median"], 3)
            if default and I.info_trainer_kind(dims) == "resident":
                res = T.Trainer("M2_info", dims, batch=B, device="cuda:0", precision="fp32", seed=0)
                r = windows(lambda: res.step(x, y, e), a.reps)
                del res
                row["resident_fp32_us"], row["generic_over_resident_fp32"] = r, round(g["median"] / r["median"], 3)
            torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

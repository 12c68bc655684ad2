"""The generic M2_info fused train step (csrc/train_info.hip; trainer_info.InfoTrainer) on the MI355X: microseconds per step beside
the per-layer module path, which was the only way to train such a model before it, and beside the resident step where both exist.

    python tools/bench_train_info.py [--out profiles/train_info.json] [--reps 20] [--batches 128 8192]

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

    def __init__(self, dims):
        from packages.models import models as M
        from packages.models.utils import elbo, binary_cross_entropy
        self.M, self.elbo, self.bce = M, elbo, binary_cross_entropy
        torch.manual_seed(0)
        self.m = synth.build_model("M2_info", dims).to("cuda")
        self.opt = torch.optim.Adam(self.m.enc_dec_clf.parameters(), lr=1e-4, betas=(0.9, 0.999))
        self.opt_aux = torch.optim.Adam(self.m.auxiliary.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        m = self.m
        yc = m.classify_fromX(x)
        r, z, mu, lv = m(x, y)
        ELBO, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        enc_loss = ELBO + 0.0 * self.bce(yc, y, 1e-8) - 10.0 * self.bce(m.classify_fromZ(z), y, 1e-8)
        aux_loss = 1.0 * self.bce(m.classify_fromZ(z.detach()), y, 1e-8)
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
    a = ap.parse_args()
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    setups = [("a", dict(ref, z_dim=32, h_dim=(256, 64))), ("b", ref), ("c", dict(ref, y_dim=513)), ("d", dict(ref, y_dim=513, z_dim=128, h_dim=(512, 512)))]
    rows = []
    for B in a.batches:
        for tag, dims in setups:
            x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
            gen = I.make_info_trainer(dims, generic=True, batch=B, device="cuda:0", seed=0)
            g = windows(lambda: gen.step(x, y, e), a.reps)
            kern = kernel_times(lambda: gen.step(x, y, e))
            plan = {"launches_per_step": gen.plan.launches_per_step, "lds_bytes": gen.plan.lds_bytes, "rows_grid": gen.plan.rows_grid,
                    "wgrad_items": gen.plan.wgrad_items, "ksplit": gen.plan.ksplit, "workspace_MB": round(gen.plan.workspace_bytes / 2 ** 20, 1)}
            del gen
            mod = ModuleStep(dims)
            m = windows(lambda: mod.step(x, y, e), a.reps)
            del mod
            row = {"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B, "generic_us": g,
                   "module_path_us": m, "generic_over_module_path": round(g["median"] / m["median"], 3),
                   "generic_mfma_fraction_of_157TFLOPs": round(flops_per_frame(dims) * B / (g["median"] * 1e-6) / PEAK_FLOPS, 4),
                   "kernels": kern, "plan": plan}
            if I.info_trainer_kind(dims) == "resident":
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

"""The generic fused train step (csrc/train_generic.hip; trainer_generic.GenericTrainer) on the MI355X: microseconds per step beside what
trained such a model before it, and beside the resident step where both exist.

    python tools/bench_train_generic.py [--out profiles/train_generic.json] [--reps 20] [--batches 128 8192]

Every time is device time from events around 10 steps in a row, the median (with min and max) over `--reps` such windows after a
warm-up window (tools/bench_encode_batch.py's method); inputs are resident on the device, the noise is passed in.
  a  z 32, h (256, 64), y_dim 1 (M2): GenericTrainer against the drop-in module of the same dims under torch autograd and stock
     torch.optim.Adam -- one Python trip and several launches per layer and direction, the only way to train it before.
  b  z 128, h (512, 512), y_dim 513: the same pair at the largest geometry, with the fraction of the 157.3 TFLOP/s fp32 matrix peak.
  c  the reference's geometry (z 16, h (128, 128), y_dim 513): GenericTrainer against Trainer(precision="fp32")."""
import argparse, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
T = importlib.import_module("disentangled-vae_amd.trainer")
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
    """The drop-in module of `dims` under torch autograd and stock torch.optim.Adam (bench.py: ModulesImpl.step)."""

    def __init__(self, model, dims):
        from packages.models import models as M
        from packages.models.utils import elbo
        self.M, self.elbo, self.model = M, elbo, model
        torch.manual_seed(0)
        self.m = synth.build_model(model, dims).to("cuda")
        self.opt = torch.optim.Adam(self.m.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        r, mu, lv = self.m(x) if self.model == "M1" else self.m(x, y)
        loss, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        loss.backward()
        self.opt.step(); self.opt.zero_grad()
        return loss


def flops_per_frame(dims):
    y, z, (h1, h2) = dims["y_dim"], dims["z_dim"], dims["h_dim"]
    mac = h1 * (513 + y) + h2 * h1 + 2 * z * h2 + h2 * (z + y) + h1 * h2 + 513 * h1
    dxm = h2 * h1 + 2 * z * h2 + z * h2 + h1 * h2 + 513 * h1
    return 2.0 * (2 * mac + dxm)


def setup(model, dims, B, reps, other):
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    gen = T.make_trainer(model, dims, generic=True, batch=B, device="cuda:0", seed=0)
    g = windows(lambda: gen.step(x, y, e), reps)
    o = other(model, dims, B)
    r = windows(lambda: o.step(x, y, e), reps)
    del gen, o
    torch.cuda.empty_cache()
    return g, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    a = ap.parse_args()
    module = lambda model, dims, B: ModuleStep(model, dims)
    resident = lambda model, dims, B: T.Trainer(model, dims, batch=B, device="cuda:0", precision="fp32", seed=0)
    setups = [("a", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64)), "module_path", module),
              ("b", dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512)), "module_path", module),
              ("c", dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128)), "resident_fp32", resident)]
    rows = []
    for B in a.batches:
        for tag, dims, name, other in setups:
            g, r = setup("M2", dims, B, a.reps, other)
            rows.append({"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B, "generic_us": g, name + "_us": r,
                         "generic_over_" + name: round(g["median"] / r["median"], 3),
                         "generic_mfma_fraction_of_157TFLOPs": round(flops_per_frame(dims) * B / (g["median"] * 1e-6) / PEAK_FLOPS, 4)})
            print(json.dumps(rows[-1]), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

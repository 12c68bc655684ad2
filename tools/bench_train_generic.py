"""The generic fused train step (csrc/train_generic.hip; trainer_generic.GenericTrainer) on the MI355X: microseconds per step beside what
trained such a model before it, and beside the resident step where both exist.

    python tools/bench_train_generic.py [--out profiles/train_generic.json] [--reps 20] [--batches 128 8192]

Every time is device time from events around 10 steps in a row, the median (with min and max) over `--reps` such windows after a
warm-up window (tools/bench_encode_batch.py's method); inputs are resident on the device, the noise is passed in.
  a  z 32, h (256, 64), y_dim 1 (M2): GenericTrainer against the drop-in module of the same dims under torch autograd and stock
     torch.optim.Adam -- one Python trip and several launches per layer and direction, the only way to train it before.
  b  z 128, h (512, 512), y_dim 513: the same pair at the largest geometry, with the fraction of the 157.3 TFLOP/s fp32 matrix peak.
  c  the reference's geometry (z 16, h (128, 128), y_dim 513): GenericTrainer against Trainer(precision="fp32").

    python tools/bench_train_generic.py --std-norm [--out profiles/train_std_norm.json] [--stats-frames 1048576 8388608]

The step with a standardised encoder input (GenericTrainer(..., std_norm=)) at setups a and b: beside the plain generic step and beside
the module path that normalises in torch, (x - mean) / (std + eps) per step as the scripts do -- the three sides take turns, one window
each, `--reps` times, in one process.  Then DeviceFrames.stats() on stores of --stats-frames frames: device time, the share of the
8 TB/s of HBM that N x 513 x 4 bytes in that time are, and torch's mean / std of the same store in float64 (conversion included: torch
has no float64 accumulation over a float32 tensor).

    rocprofv3 --kernel-trace --stats -- python tools/bench_train_generic.py --std-norm --trace-steps 20 --batches 8192

runs only 20 steps a side at setup b, for the per-kernel times of a kernel trace in a run of its own."""
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


def alternating(sides, reps):
    """{name: median / min / max} of one window a side in turn, `reps` rounds after a warm-up round"""
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / INNER
    for fn in sides.values():
        window(fn)
    us = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            us[k].append(window(fn))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in us.items()}


class NormModuleStep(ModuleStep):
    """ModuleStep with the scripts' normalisation in torch in front of the encoder (scripts/training_M2.py:136-144)."""

    def __init__(self, model, dims, mean, std):
        super().__init__(model, dims)
        self.mean, self.std = mean, std

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        xn = (x - self.mean) / (self.std + 1e-8)
        r, mu, lv = self.m(xn) if self.model == "M1" else self.m(xn, y)
        loss, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        loss.backward()
        self.opt.step(); self.opt.zero_grad()
        return loss


STD_SETUPS = [("a", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))), ("b", dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512)))]
HBM_BYTES_PER_S = 8e12


def std_norm_sides(dims, B):
    F = importlib.import_module("disentangled-vae_amd.frames")
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    pool = synth.device_batches(dims, 4096, 1, 1, "cuda")[0][0]
    mean, std = F.frame_stats(pool)
    norm = T.make_trainer("M2", dims, batch=B, device="cuda:0", seed=0, std_norm=(mean, std))
    plain = T.make_trainer("M2", dims, generic=True, batch=B, device="cuda:0", seed=0)
    mod = NormModuleStep("M2", dims, mean, std)
    return {"std_norm": lambda: norm.step(x, y, e), "plain_generic": lambda: plain.step(x, y, e), "module_path_norm_in_torch": lambda: mod.step(x, y, e)}, (norm, plain, mod)


def bench_stats(n, reps):
    F = importlib.import_module("disentangled-vae_amd.frames")
    x = torch.empty((n, 513), dtype=torch.float32, device="cuda")
    for lo in range(0, n, 1 << 20):                       # exponential power frames, a level per bin
        x[lo:lo + (1 << 20)].exponential_().mul_(torch.logspace(-2, 1.7, 513, device="cuda"))
    def timed(fn, k):
        fn(); torch.cuda.synchronize()
        out = []
        for _ in range(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            out.append(1e3 * e0.elapsed_time(e1))
        return {"median": round(statistics.median(out), 1), "min": round(min(out), 1), "max": round(max(out), 1)}
    ours = timed(lambda: F.frame_stats(x), reps)
    def torch64():
        d = x.double()
        return d.mean(0), d.std(0)
    theirs = timed(torch64, 3)
    mean, std = F.frame_stats(x)
    tm, ts = torch64()
    row = {"frames": n, "frame_stats_us": ours, "hbm_share": round(n * 513 * 4 / (ours["median"] * 1e-6) / HBM_BYTES_PER_S, 3),
           "torch_float64_mean_std_us": theirs, "torch_over_frame_stats": round(theirs["median"] / ours["median"], 2),
           "max_rel_diff_mean": float(((mean.double() - tm).abs() / tm.abs()).max()), "max_rel_diff_std": float(((std.double() - ts).abs() / ts).max())}
    del x
    torch.cuda.empty_cache()
    return row


def main_std_norm(a):
    if a.trace_steps:
        sides, keep = std_norm_sides(STD_SETUPS[1][1], a.batches[-1])
        for name in ("std_norm", "plain_generic"):
            for _ in range(a.trace_steps):
                sides[name]()
        torch.cuda.synchronize()
        return
    rows = []
    for B in a.batches:
        for tag, dims in STD_SETUPS:
            sides, keep = std_norm_sides(dims, B)
            r = alternating(sides, a.reps)
            rows.append({"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B, "us": r,
                         "std_norm_over_plain_generic": round(r["std_norm"]["median"] / r["plain_generic"]["median"], 3),
                         "std_norm_over_module_path": round(r["std_norm"]["median"] / r["module_path_norm_in_torch"]["median"], 3)})
            print(json.dumps(rows[-1]), flush=True)
            del sides, keep
            torch.cuda.empty_cache()
    stats = []
    for n in a.stats_frames:
        stats.append(bench_stats(n, a.reps))
        print(json.dumps(stats[-1]), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "rows": rows, "frame_stats": stats}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


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
    ap.add_argument("--std-norm", action="store_true", help="the step with a standardised encoder input, and DeviceFrames.stats()")
    ap.add_argument("--stats-frames", type=int, nargs="*", default=[1 << 20, 1 << 23])
    ap.add_argument("--trace-steps", type=int, default=0, help="with --std-norm: only this many steps a side at setup b (for a kernel trace)")
    a = ap.parse_args()
    if a.std_norm:
        return main_std_norm(a)
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

"""The classifier's fused train step (csrc/train_classifier.hip; trainer_classifier.ClassifierTrainer) on the MI355X: microseconds per
step beside the module path -- packages.models.models.Classifier + packages.models.utils.binary_cross_entropy + stock
torch.optim.Adam on the device, the only way to train these nets before.

    python tools/bench_train_classifier.py [--out profiles/train_classifier.json] [--reps 20] [--batches 128 8192]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_classifier.py --trace-steps 50      (a run of its own)
    python tools/bench_train_classifier.py --out ... --kernel-stats DIR                                      (merges that run's table)

Every time is device time from events around 10 steps in a row, the median (with min and max) over `--reps` such windows after a
warm-up window (tools/bench_train_generic.py's method); inputs are resident on the device.  Both sides are timed in the same run, the
fused step first.  Per geometry and batch:
  step_us          the three launches of ClassifierTrainer.step
  module_path_us   forward, BCE, backward, Adam.step, zero_grad of the module path
  grads_us         rows + weight-gradient launches alone (grads_only); apply_us = step - grads (the apply launch, by difference)
  eval_us          rows kernel forward-only + the finalising launch (evaluate)
  mfma_fraction    algorithmic flops of the step (forward, backward-data and weight-gradient products) over step time, as a fraction of
                   the 157.3 TFLOP/s fp32 matrix peak: a whole-step rate, not a kernel's
--kernel-stats adds the per-kernel device times of a rocprofv3 run (the split by kernel proper)."""
import argparse, csv, glob, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
synth = importlib.import_module("disentangled-vae_amd.synth")
INNER, PEAK_FLOPS = 10, 157.3e12
GEOMETRIES = [((128, 128), 1), ((128, 128), 513), ((256, 64), 1), ((512, 512), 513)]


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
    """Classifier under torch autograd and stock torch.optim.Adam."""

    def __init__(self, dims):
        from packages.models.models import Classifier
        from packages.models.utils import binary_cross_entropy
        self.bce = binary_cross_entropy
        torch.manual_seed(0)
        self.m = Classifier(dims).to("cuda")
        self.opt = torch.optim.Adam(self.m.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def step(self, x, y):
        loss = self.bce(self.m(x), y, 1e-8)
        loss.backward()
        self.opt.step(); self.opt.zero_grad()
        return loss


def flops_per_frame(h1, h2, y):
    mac = 513 * h1 + h1 * h2 + h2 * y                     # forward; the weight gradients take the same again
    dxm = h2 * y + h1 * h2                                # backward-data (no d x)
    return 2.0 * (2 * mac + dxm)


def batch_of(h, y, B):
    x, yy, _ = synth.device_batches(dict(x_dim=513, y_dim=y, z_dim=1, h_dim=h), B, 1, 0, "cuda")[0]
    return x, yy


def kernel_stats(path):
    """{kernel: {calls, total_us, mean_us}} of the classifier step's kernels from rocprofv3's *kernel_stats.csv under `path`."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if "train_clf" in name or "train_generic" in name:
                short = name.split("(")[0].split("::")[-1]
                out[short] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1),
                              "mean_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    ap.add_argument("--trace-steps", type=int, default=0, help="no timing: this many fused steps at (512, 512) / y 513, 8192 frames, for a "
                    "kernel trace taken from outside")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="the output directory of such a trace: its per-kernel table goes into the result")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_classifier: no GPU (there is nothing to measure without one)")
    if a.trace_steps:
        (h, y), B = GEOMETRIES[-1], 8192
        x, yy = batch_of(h, y, B)
        tr = C.ClassifierTrainer([513, list(h), y], batch=B, device="cuda:0", seed=0)
        for _ in range(a.trace_steps):
            tr.step(x, yy)
        torch.cuda.synchronize()
        return
    rows = []
    for B in a.batches:
        for h, y in GEOMETRIES:
            dims = [513, list(h), y]
            x, yy = batch_of(h, y, B)
            tr = C.ClassifierTrainer(dims, batch=B, device="cuda:0", seed=0)
            step = windows(lambda: tr.step(x, yy), a.reps)
            grads = windows(lambda: tr.grads_only(x, yy), a.reps)
            ev = windows(lambda: tr.evaluate(x, yy), a.reps)
            mod = ModuleStep(dims)
            module = windows(lambda: mod.step(x, yy), a.reps)
            rows.append({"geometry": f"h {h}, y_dim {y}", "batch": B, "step_us": step, "module_path_us": module,
                         "step_over_module_path": round(step["median"] / module["median"], 3),
                         "grads_us": grads, "apply_us_by_difference": round(step["median"] - grads["median"], 2), "eval_us": ev,
                         "rows_grid": tr.plan.rows_grid, "wgrad_items": tr.plan.wgrad_items, "slices": tr.plan.ksplit, "lds_bytes": tr.plan.lds_bytes,
                         "step_mfma_fraction_of_157TFLOPs": round(flops_per_frame(h[0], h[1], y) * B / (step["median"] * 1e-6) / PEAK_FLOPS, 4)})
            print(json.dumps(rows[-1]), flush=True)
            del tr, mod
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "rows": rows}
    if a.kernel_stats:
        res["kernels_h512x512_y513_B8192"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernels_h512x512_y513_B8192"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

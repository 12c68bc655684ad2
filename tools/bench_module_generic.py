"""The script loop on a module of another size than the reference's (examples/train_script_loop.py: module forward, elbo in torch,
loss.backward(), stock torch.optim.Adam, zero_grad) on the MI355X: microseconds per loop iteration on the generic module engine
(disentangled-vae_amd/module_path.py: GenericModuleEngine, DVAE_MODULE_GENERIC=1) beside the per-layer path such a module takes by
default -- the behaviour before the engine existed -- and, for context, GenericTrainer.step on the same model and batch (the whole
step fused, optimizer included, no autograd).

    python tools/bench_module_generic.py [--out profiles/module_generic.json] [--reps 20] [--batches 128 8192]

Geometries: z 32, h (256, 64), y_dim 1 and z 128, h (512, 512), y_dim 513 (M2).  The three sides take turns in one process, one window
each, `--reps` rounds after a warm-up round.  A window is `iterations_per_window` loop iterations in a row: device time from events
around them, wall time from a host clock that stops after the synchronise behind them; the medians (with min and max) over the rounds.
Inputs are resident on the device and the noise is passed in.  Before timing, the two module sides are compared at equal parameters:
loss and the largest relative difference of a gradient tensor over its maximum.
"""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
T = importlib.import_module("disentangled-vae_amd.trainer")
synth = importlib.import_module("disentangled-vae_amd.synth")
mp = importlib.import_module("disentangled-vae_amd.module_path")

SETUPS = [("a", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))), ("b", dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512)))]


class ScriptLoop:
    """One iteration of the script loop on the drop-in module of `dims`; mode: "off" (per-layer Functions) or "on" (the generic engine)."""

    def __init__(self, model, dims, mode):
        from packages.models import models as M
        from packages.models.utils import elbo
        self.M, self.elbo, self.model = M, elbo, model
        torch.manual_seed(0)
        self.m = synth.build_model(model, dims).to("cuda")
        mp.set_generic(self.m, mode)
        self.kind = mp.engine_kind(self.m, model)
        self.opt = torch.optim.Adam(self.m.parameters(), lr=1e-4, betas=(0.9, 0.999))

    def loss_and_grads(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        r, mu, lv = self.m(x) if self.model == "M1" else self.m(x, y)
        loss, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        loss.backward()
        g = {k: p.grad.clone() for k, p in self.m.named_parameters()}
        self.opt.zero_grad()
        return float(loss.detach()), g

    def step(self, x, y, e):
        self.M.Stochastic.epsilon_fn = lambda mu: e
        r, mu, lv = self.m(x) if self.model == "M1" else self.m(x, y)
        loss, _, _ = self.elbo(x, r, mu, lv, 1e-8)
        loss.backward()
        self.opt.step(); self.opt.zero_grad()
        return loss


def alternating(sides, reps, inner):
    """{name: {device_us, wall_us: median / min / max}} of one window a side in turn, `reps` rounds after a warm-up round"""
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / inner, 1e6 * (time.perf_counter() - t0) / inner
    for fn in sides.values():
        window(fn)
    dev, wall = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            d, w = window(fn)
            dev[k].append(d); wall[k].append(w)
    stat = lambda v: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    return {k: {"device_us": stat(dev[k]), "wall_us": stat(wall[k])} for k in sides}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "module_generic.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_module_generic.py measures on the GPU: none found")
    os.environ.pop("DVAE_MODULE_PATH", None)
    rows = []
    for tag, dims in SETUPS:
        for B in a.batches:
            x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
            layers, generic = ScriptLoop("M2", dims, "off"), ScriptLoop("M2", dims, "on")
            assert layers.kind is None and generic.kind == "generic", (layers.kind, generic.kind)
            la, ga = layers.loss_and_grads(x, y, e)
            lb, gb = generic.loss_and_grads(x, y, e)
            assert generic.m.__dict__.get("_dvae_engine") is not None and layers.m.__dict__.get("_dvae_engine") is None
            gdiff = max(float((ga[k] - gb[k]).abs().max() / (ga[k].abs().max() + 1e-30)) for k in ga)
            trainer = T.make_trainer("M2", dims, generic=True, batch=B, device="cuda:0", seed=0)
            inner = 50 if B <= 1024 else 10
            sides = {"per_layer": lambda: layers.step(x, y, e), "generic_engine": lambda: generic.step(x, y, e),
                     "generic_trainer_step": lambda: trainer.step(x, y, e)}
            r = alternating(sides, a.reps, inner)
            rows.append({"setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B,
                         "iterations_per_window": inner, "us_per_iteration": r,
                         "generic_engine_over_per_layer_device": round(r["generic_engine"]["device_us"]["median"] / r["per_layer"]["device_us"]["median"], 3),
                         "generic_engine_over_per_layer_wall": round(r["generic_engine"]["wall_us"]["median"] / r["per_layer"]["wall_us"]["median"], 3),
                         "first_loss_per_layer": la, "first_loss_generic_engine": lb, "first_gradient_max_rel_diff": gdiff})
            print(json.dumps(rows[-1]), flush=True)
            del layers, generic, trainer, sides
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

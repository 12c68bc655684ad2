"""The weighted KL term of the fused any-size train steps (GenericTrainer / InfoTrainer(..., kl_weight=, kl_warmup=, kl_floor=);
disentangled-vae_amd/kl_weight.py) on the MI355X: microseconds per step of a weighted step beside the default call in the same run.

    python tools/bench_train_kl.py [--out profiles/train_kl.json] [--reps 20] [--batches 128 8192] [--default-only]

Setups: M2 and M2_info at  a  z 32, h (256, 64), y_dim 1  and  b  z 128, h (512, 512), y_dim 513.  The two sides -- the default call and
kl_weight 0.5 / kl_warmup 200 / kl_floor 0.7 -- take turns, one window each, `--reps` times, in one process; every time is device time
from events around 10 steps in a row, the median (with min and max) over the windows after a warm-up window
(tools/bench_train_generic.py: alternating); inputs are resident on the device, the noise is passed in.  The default side appears
twice ("default", "default_again"): the difference of the two is the run-to-run spread the other figures are read against.

--default-only runs the default side alone (twice): the figure to compare with another build of the library (DVAE_LIB=<path>) on the
same box, e.g. the commit before the weighted KL term."""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from bench_train_generic import alternating, INNER
T = importlib.import_module("disentangled-vae_amd.trainer")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
synth = importlib.import_module("disentangled-vae_amd.synth")

SETUPS = [("a", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))), ("b", dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512)))]
KL = dict(kl_weight=0.5, kl_warmup=200, kl_floor=0.7)


def make(model, dims, B, **kw):
    if model == "M2_info":
        return I.make_info_trainer(dims, generic=True, batch=B, device="cuda:0", seed=0, **kw)
    return T.make_trainer(model, dims, generic=True, batch=B, device="cuda:0", seed=0, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 8192])
    ap.add_argument("--default-only", action="store_true", help="the default call alone, twice (another library build under DVAE_LIB)")
    a = ap.parse_args()
    rows = []
    for model in ("M2", "M2_info"):
        for B in a.batches:
            for tag, dims in SETUPS:
                x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
                trainers = {"default": make(model, dims, B), "default_again": make(model, dims, B)}
                if not a.default_only:
                    trainers["kl_weighted"] = make(model, dims, B, **KL)
                r = alternating({k: (lambda t=t: t.step(x, y, e)) for k, t in trainers.items()}, a.reps)
                row = {"model": model, "setup": tag, "geometry": f"z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}", "batch": B, "us": r,
                       "default_again_over_default": round(r["default_again"]["median"] / r["default"]["median"], 4)}
                if not a.default_only:
                    row["kl_weighted_over_default"] = round(r["kl_weighted"]["median"] / r["default"]["median"], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del trainers
                torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "kl_options": None if a.default_only else KL,
           "library": os.environ.get("DVAE_LIB", "this tree's"), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

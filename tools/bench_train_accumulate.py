"""Gradient accumulation on the any-size fused train steps (disentangled-vae_amd/accumulate.py; csrc/train_tables.hip:
train_generic_reduce_kernel) on the MI355X.

    python tools/bench_train_accumulate.py [--out profiles/train_accumulate.json] [--reps 10] [--trace-stats kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_accumulate.py --kernels-only        # a run of its own

Every time is device time from events around 10 steps in a row, the median (with min and max) over `--reps` such windows after a
warm-up window (tools/bench_train_generic.py's method); the two sides of a comparison alternate window by window in the same run;
inputs are resident on the device, the noise is passed in.
  1  microseconds per EFFECTIVE step of K in {2, 8} micro-batches of 8192 frames + one apply, against K plain step()s of 8192 on the
     same trainer: K - 1 fewer Adam passes, K more reduce launches.
  2  the reduce launch alone (10 back to back, so launch-to-launch device time) at ksplit 1 and 16: the bytes it moves,
     (ksplit + 1 + accumulate) n_params 4, over that time as a share of the 8 TB/s HBM peak -- the slabs were written by the launch
     before and are read from the caches, so this is a rate, not an HBM measurement -- beside the apply launch on the flat gradient.
     --trace-stats adds the per-kernel averages of a kernel trace taken in a run of its own (--kernels-only).
  3  workspace_bytes of the M2_info plan at the largest geometry for 65 536 frames in one step against the 8192-frame plan an
     eight-micro-batch step uses (host only), and the eight-micro-batch step itself (row 1, K = 8).
  2b the device time of each micro-batch (rows + weight gradients + reduce; events around one, a synchronise after it) by its position
     after the apply, as AccumulatedStep runs it and with a repack of the packed weight copies before every micro-batch, beside one
     plain step timed the same way: where an accumulated step's time goes at the largest geometries.
  4  more than one device visible: frames/s over the ranks is NOT measured by this tool on a one-GPU machine; it says so.

    python tools/bench_train_accumulate.py --clip [--out profiles/train_clip.json] [--reps 20]

--clip measures what clipping the global gradient norm on the device costs (csrc/train_tables.hip: train_generic_gradnorm_kernel,
train_generic_apply_clipped_kernel), against the unclipped call in the same run, alternating, at M2 z 32 / h (256, 64) / y 1 and the
largest M2_info geometry, 128 and 8192 frames: the optimizer launch of apply() on the flat gradient of one micro-batch against the two
launches of apply(max_norm=inf), and step() (three launches) against step(max_norm=inf) (five: the reduce and the norm launch more).
max_norm = inf clips nothing, so both sides walk the same parameters."""
import argparse, csv, ctypes, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
T = importlib.import_module("disentangled-vae_amd.trainer")
TI = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")
N = importlib.import_module("disentangled-vae_amd.native")
synth = importlib.import_module("disentangled-vae_amd.synth")
INNER, HBM_PEAK, B = 10, 8.0e12, 8192
LARGEST = dict(x_dim=513, y_dim=513, z_dim=128, h_dim=(512, 512))
GEOMETRIES = [("M2", dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))), ("M2", LARGEST),
              ("M2", dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))), ("M2_info", LARGEST)]


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / INNER


def summary(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def alternating(fa, fb, reps):
    window(fa); window(fb)
    ua, ub = [], []
    for _ in range(reps):
        ua.append(window(fa)); ub.append(window(fb))
    return summary(ua), summary(ub)


def make(model, dims, ksplit=0, batch=B):
    kw = dict(batch=batch, device="cuda:0", seed=0, ksplit=ksplit)
    return TI.make_info_trainer(dims, generic=True, **kw) if model == "M2_info" else T.make_trainer(model, dims, generic=True, **kw)


def geometry(model, dims):
    return f"{model} z {dims['z_dim']}, h {dims['h_dim']}, y_dim {dims['y_dim']}"


def effective_steps(model, dims, reps):
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    tr = make(model, dims)
    acc = A.AccumulatedStep(tr)
    rows = []
    for K in (2, 8):
        def accumulated():
            for _ in range(K):
                acc.micro(x, y, e)
            acc.apply()

        def plain():
            for _ in range(K):
                tr.step(x, y, e)
        a, p = alternating(accumulated, plain, reps)
        rows.append({"geometry": geometry(model, dims), "micro_batch": B, "K": K, "effective_frames": K * B, "ksplit": tr.plan.ksplit,
                     "accumulated_us": a, "plain_steps_us": p, "accumulated_over_plain": round(a["median"] / p["median"], 4)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def reduce_alone(model, dims, ksplit, reps):
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    tr = make(model, dims, ksplit)
    acc = A.AccumulatedStep(tr)
    acc.micro(x, y, e)                                             # the slabs of one micro-batch
    kind = "info" if model == "M2_info" else "generic"
    red, app = getattr(tr.lib, f"dvae_train_{kind}_reduce"), getattr(tr.lib, f"dvae_train_{kind}_apply_flat")
    plan, P, ks = ctypes.byref(tr.plan), tr.plan.n_params, tr.plan.ksplit
    out = {"geometry": geometry(model, dims), "ksplit": ks, "n_params": P}
    for accumulate in (0, 1):
        us = [window(lambda: N.check(red(plan, N.ptr(tr.ws), N.ptr(acc.flat), accumulate, 1.0, N.ptr(tr.losses), N.stream()), "reduce"))
              for _ in range(reps + 1)][1:]
        nbytes = (ks + 1 + accumulate) * P * 4
        out[f"reduce_accumulate{accumulate}"] = {"us": summary(us), "bytes": nbytes,
                                                 "share_of_8TBs": round(nbytes / (statistics.median(us) * 1e-6) / HBM_PEAK, 4)}
    acc.flat.zero_()                                               # (a zero gradient: the parameters stay finite over the windows)
    us = [window(lambda: N.check(app(plan, N.ptr(tr.params), N.ptr(tr.m), N.ptr(tr.v), N.ptr(tr.ws), N.ptr(acc.flat), 1, 1e-4, 0.9, 0.999, 1e-8,
                                     1.0, N.stream()), "apply_flat")) for _ in range(reps + 1)][1:]
    out["apply_flat_us"] = summary(us)
    print(json.dumps(out), flush=True)
    return out


def by_position(model, dims, K=4, reps=8):
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    tr = make(model, dims)
    acc = A.AccumulatedStep(tr)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1)
    out = {"geometry": geometry(model, dims), "micro_batch": B, "K": K}
    for repack in (False, True):
        per = [[] for _ in range(K)]
        for rep in range(reps + 1):
            for k in range(K):
                if repack:
                    tr._repack()
                us = timed(lambda: acc.micro(x, y, e))
                if rep:
                    per[k].append(us)
            acc.apply()
            torch.cuda.synchronize()
        out["micro_batch_us_by_position_repack_before_each" if repack else "micro_batch_us_by_position"] = [round(statistics.median(p), 1) for p in per]
    out["plain_step_us"] = round(statistics.median([timed(lambda: tr.step(x, y, e)) for _ in range(reps + 1)][1:]), 1)
    print(json.dumps(out), flush=True)
    return out


def clip_cost(model, dims, batch, reps):
    x, y, e = synth.device_batches(dims, batch, 1, 0, "cuda")[0]
    tr = make(model, dims, batch=batch)
    acc = A.AccumulatedStep(tr)
    acc.micro(x, y, e)                                             # the flat gradient of one micro-batch
    inf = float("inf")
    ap, ac = alternating(lambda: tr._apply_flat(acc.flat, 1.0), lambda: tr._apply_flat_clipped(acc.flat, 1.0, inf), reps)
    sp, sc = alternating(lambda: tr.step(x, y, e), lambda: tr.step(x, y, e, max_norm=inf), reps)
    P = tr.plan.n_params
    out = {"geometry": geometry(model, dims), "frames": batch, "n_params": P, "norm_chunks": (P + 4095) // 4096, "ksplit": tr.plan.ksplit,
           "apply_us": ap, "apply_clipped_us": ac, "apply_added_us": round(ac["median"] - ap["median"], 2),
           "apply_clipped_over_apply": round(ac["median"] / ap["median"], 4),
           "step_us": sp, "step_clipped_us": sc, "step_added_us": round(sc["median"] - sp["median"], 2),
           "step_clipped_over_step": round(sc["median"] / sp["median"], 4),
           "skipped_steps": tr.skipped_step_count(), "last_grad_norm": tr.grad_norm.cpu().tolist()}
    print(json.dumps(out), flush=True)
    return out


def clip_mode(a):
    reps = a.reps if a.reps != 10 else 20
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "calls_per_window": INNER,
           "method": "device time from events around 10 calls in a row; median (min, max) of `reps` windows after a warm-up window; the two "
                     "sides of a comparison alternate window by window; max_norm = inf", "clip": []}
    for model, dims in (GEOMETRIES[0], GEOMETRIES[3]):
        for batch in (128, B):
            res["clip"].append(clip_cost(model, dims, batch, reps))
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def kernels_only():
    """For a kernel trace: 20 effective steps of two micro-batches at the M2_info largest geometry, ksplit as the plan chooses."""
    model, dims = GEOMETRIES[3]
    x, y, e = synth.device_batches(dims, B, 1, 0, "cuda")[0]
    acc = A.AccumulatedStep(make(model, dims))
    for _ in range(20):
        acc.micro(x, y, e); acc.micro(x, y, e); acc.apply()
    torch.cuda.synchronize()


def trace_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if any(k in name for k in ("train_generic_reduce_kernel", "train_generic_apply_kernel", "train_info_rows_kernel", "train_generic_wgrad_kernel")):
                key = "reduce" if "reduce" in name else "apply" if "apply" in name else "rows" if "rows" in name else "wgrad"
                out[key] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                            "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--clip", action="store_true", help="the cost of clipping the global gradient norm on the device (see the module's text)")
    ap.add_argument("--trace-stats", default=None, help="kernel_stats.csv of a kernel trace of --kernels-only")
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only()
    if a.clip:
        return clip_mode(a)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "steps_per_window": INNER, "effective_steps": [], "reduce_alone": []}
    for model, dims in GEOMETRIES:
        res["effective_steps"] += effective_steps(model, dims, a.reps)
        torch.cuda.empty_cache()
    for ksplit in (1, 16):
        res["reduce_alone"].append(reduce_alone(*GEOMETRIES[3], ksplit, a.reps))
        torch.cuda.empty_cache()
    res["by_position"] = [by_position(*GEOMETRIES[3]), by_position(*GEOMETRIES[1])]
    torch.cuda.empty_cache()
    if a.trace_stats:
        res["kernel_trace_M2_info_largest"] = trace_stats(a.trace_stats)
    one, micro = TI.make_plan(LARGEST, 65536), TI.make_plan(LARGEST, B)
    res["memory_M2_info_largest"] = {"workspace_bytes_one_step_of_65536": one.workspace_bytes, "workspace_bytes_micro_batch_8192": micro.workspace_bytes,
                                     "flat_gradient_bytes": micro.n_params * 4,
                                     "ratio": round(one.workspace_bytes / (micro.workspace_bytes + micro.n_params * 4), 2),
                                     "effective_step_of_65536": "effective_steps: M2_info largest, K = 8"}
    ndev = torch.cuda.device_count()
    res["multi_gpu"] = {"devices_visible": ndev, "scaling": "not measured" if ndev < 2 else "not measured by this tool: run examples/train_fused.py --gpus N"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

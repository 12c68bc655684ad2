"""Batched training-set front end against the per-utterance loop, on the MI355X.

    python tools/bench_front_end_batch.py [--out profiles/front_end_batch.json] [--reps 10] [--utterances 256]

256 synthetic utterances of 4-6 s (float64, on the host as soundfile returns them), for vad_labels and ibm_labels.  In alternation
(one round = one run of each variant, median of the rounds): utterances_to_frames on the whole list, and the loop of
utterance_to_frames over the same utterances -- wall clock from host arrays to training rows on the device, device synchronised
(what examples/build_train_set.py waits for).  Both give bit-identical rows (checked first).  Device time per kernel: the same script
with --reps 1 under `rocprofv3 --kernel-trace --stats` (profiles/front_end_batch_kernel_stats.csv)."""
import argparse, importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
T = importlib.import_module("disentangled-vae_amd.target")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(variants, reps):
    """variants: name -> callable; every round runs each once (warm-up round first); median seconds per name."""
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(wall(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def speechlike(n, rng):
    env = np.repeat((rng.random(n // 1600 + 1) > 0.4).astype(np.float64), 1600)[:n]
    return env * rng.standard_normal(n) * 0.3 + 0.003 * rng.standard_normal(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--utterances", type=int, default=256)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    speeches = [speechlike(int(n), rng) for n in rng.integers(4 * 16000, 6 * 16000, a.utterances)]
    res = {"device": torch.cuda.get_device_name(0), "utterances": a.utterances, "samples": int(sum(len(s) for s in speeches))}
    for labels in ("vad_labels", "ibm_labels"):
        fb = T.utterances_to_frames(speeches, labels)
        loop = [T.utterance_to_frames(s, labels) for s in speeches]
        assert all(torch.equal(fb.frames(u)[0], loop[u][0]) and torch.equal(fb.frames(u)[1], loop[u][1]) for u in range(len(speeches)))
        del loop
        t = alternate({"batch": lambda: T.utterances_to_frames(speeches, labels),
                       "loop": lambda: [T.utterance_to_frames(s, labels) for s in speeches]}, a.reps)
        res[labels] = {"frames": int(sum(fb.counts)), "batch_ms": round(t["batch"] * 1e3, 2), "loop_ms": round(t["loop"] * 1e3, 2),
                       "loop_over_batch": round(t["loop"] / t["batch"], 1),
                       "batch_Mframes_s": round(sum(fb.counts) / t["batch"] / 1e6, 1)}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

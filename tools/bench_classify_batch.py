"""classify_batch and f1_batch on the MI355X: device time on the evaluation's workload, against the matrix peak and HBM, beside the
per-utterance path they replace.

    python tools/bench_classify_batch.py [--out profiles/classify_batch.json] [--reps 20] [--utterances 256] [--seconds 5]

Workload: `--utterances` x `--seconds` s at 16 kHz, 1024 / 256 STFT (256 x 5 s: 79 360 frames), complex frames resident on the device,
y_dim 1 and 513, seeded default-init weights.
  classify_ms    one classify_batch call (table, two output allocations, one launch) from events around 10 calls in a row, the median
                 over `--reps` such windows after a warm-up window
  mfma_fraction  frames x 2 (513 x 128 + 128 x 128 + 128 x y_dim) flop over the device time, as a fraction of 157.3 TFLOP/s (fp32 matrix)
  hbm_fraction   frames x (513 x 8 read + 2 x y_dim x 4 written) bytes over the device time, as a fraction of 8 TB/s
  f1_ms          one f1_batch call (count launch + the [U, 4] finishing in torch) the same way
  per_utterance  the same labels and scores through the path of the parent commit, in the same run: per utterance a host-formed
                 |X|^2 uploaded, model.classifier on the layer kernels, a torch threshold, f1_loss -- wall time around the loop with
                 a synchronisation at its end (it is bound by the host, so events around it would say the same)."""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from packages.models.models import Classifier
from packages.models.utils import f1_loss
C = importlib.import_module("disentangled-vae_amd.classify")
H = importlib.import_module("disentangled-vae_amd.stft")
INNER, PEAK_FLOPS, PEAK_BYTES_PER_S = 10, 157.3e12, 8e12


def windows(fn, reps):
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER
    window()
    ms = [window() for _ in range(reps)]
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def one_case(y_dim, spec, reps):
    torch.manual_seed(1)
    clf = Classifier([513, [128, 128], y_dim]).cuda().eval()
    for p in clf.parameters():
        p.requires_grad = False
    pack = C.ClassifierPack(clf)
    frames, U = sum(spec.counts), len(spec)
    lb = C.classify_batch(pack, spec)
    truth = (torch.rand_like(lb.hard) > 0.5).float()
    cls = windows(lambda: C.classify_batch(pack, spec), reps)
    f1 = windows(lambda: C.f1_batch(lb, truth, counts=spec.counts), reps)
    flop = frames * 2 * (513 * 128 + 128 * 128 + 128 * y_dim)
    nbytes = frames * (513 * 8 + 2 * y_dim * 4)
    # the per-utterance path: what an evaluation loop does without the batch ops
    X_host = spec.numpy()
    truth_host = [truth[a:b] for a, b in zip(spec.frame_off[:-1], spec.frame_off[1:])]

    def loop():
        out = []
        for X, t in zip(X_host, truth_host):
            S_abs_2 = torch.tensor(np.abs(X) ** 2, device="cuda")
            hard = (clf(torch.t(S_abs_2)) > 0.5).float()
            out.append(f1_loss(hard.flatten(), t.flatten(), 1e-8))
        torch.cuda.synchronize()
        return out
    loop()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        per = loop()
        walls.append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(torch.stack([torch.stack(r) for r in per]), C.f1_batch(lb, truth, counts=spec.counts)))
    return {"y_dim": y_dim, "utterances": U, "frames": frames, "classify_ms": cls, "f1_ms": f1,
            "frames_per_s": round(frames / (cls["median"] * 1e-3), 0), "flop": flop,
            "mfma_fraction_of_157TFLOPs": round(flop / (cls["median"] * 1e-3) / PEAK_FLOPS, 4),
            "bytes": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (cls["median"] * 1e-3) / PEAK_BYTES_PER_S, 4),
            "per_utterance_wall_ms": round(statistics.median(walls), 2), "per_utterance_f1_equals_batch": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=5.0)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n = int(a.seconds * 16000)
    spec = H.stft_batch([(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(a.utterances)])
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "calls_per_window": INNER, "cases": [one_case(y, spec, a.reps) for y in (1, 513)]}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

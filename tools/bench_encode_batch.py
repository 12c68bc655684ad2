"""encode_batch and the fused MCEM start on the MI355X: device time of the encoder launch against the matrix peak and HBM, and
McemBatch.init_parameters(fused_start=True) beside the default path in the same run.

    python tools/bench_encode_batch.py [--out profiles/encode_batch.json] [--reps 20] [--utterances 25 256] [--frames 300]

Workload: `--utterances` x `--frames` frames (300 frames: 4.8 s at 16 kHz, 1024 / 256 STFT), complex frames resident on the device,
y_dim 0, 1 and 513, seeded xavier weights with N(0, 0.05) biases.
  encode_ms      one encode_batch call (table, two output allocations, one launch of dvae_encode_batch) from events around 10 calls in
                 a row, the median over `--reps` such windows after a warm-up window
  mfma_fraction  frames x 2 ((513 + y_dim) x 128 + 128 x 128 + 128 x 32) flop over the device time, as a fraction of 157.3 TFLOP/s
  hbm_fraction   frames x (513 x 8 + y_dim x 4 read + 2 x 16 x 4 written) bytes over the device time, as a fraction of 8 TB/s
  init           McemBatch.init_parameters on the same SpecBatch (labels: a LabelBatch on the device for y_dim > 0), fused_start=True
                 and the default path (the per-utterance loop, unchanged): wall time with a synchronisation at the end and device
                 time from events around the call, each the median of three calls after a warm-up call."""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from packages.models.models import VariationalAutoencoder, DeepGenerativeModel
C = importlib.import_module("disentangled-vae_amd.classify")
E = importlib.import_module("disentangled-vae_amd.encode")
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.mcem")
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


def timed_init(mb, spec, labels, fused):
    def once():
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        mb.init_parameters(spec, labels, fused_start=fused)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
    once()
    runs = [once() for _ in range(3)]
    return {"wall_ms": round(statistics.median(r[0] for r in runs), 3), "device_ms": round(statistics.median(r[1] for r in runs), 3)}


def one_case(y_dim, spec, reps):
    torch.manual_seed(1)
    vae = (VariationalAutoencoder([513, 16, [128, 128]]) if y_dim == 0 else DeepGenerativeModel([513, y_dim, 16, [128, 128]], None))
    with torch.no_grad():
        for m in vae.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    vae = vae.cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False
    frames, U = sum(spec.counts), len(spec)
    y = (torch.rand((frames, y_dim), device="cuda") > 0.5).float() if y_dim else None
    labels = C.LabelBatch(y, y, spec.counts) if y_dim else None
    pack = E.EncoderPack(vae.encoder, y_dim)
    enc = windows(lambda: E.encode_batch(pack, spec, labels), reps)
    flop = frames * 2 * ((513 + y_dim) * 128 + 128 * 128 + 128 * 32)
    nbytes = frames * (513 * 8 + y_dim * 4 + 2 * 16 * 4)
    mb = M.McemBatch(vae, niter=1, label_in_encoder=y_dim > 0, label_in_decoder=y_dim > 0)
    fused = timed_init(mb, spec, labels, True)
    default = timed_init(mb, spec, labels, False)
    return {"y_dim": y_dim, "utterances": U, "frames": frames, "encode_ms": enc, "frames_per_s": round(frames / (enc["median"] * 1e-3), 0), "flop": flop,
            "mfma_fraction_of_157TFLOPs": round(flop / (enc["median"] * 1e-3) / PEAK_FLOPS, 4), "bytes": nbytes,
            "hbm_fraction_of_8TBps": round(nbytes / (enc["median"] * 1e-3) / PEAK_BYTES_PER_S, 4), "init_fused": fused, "init_default": default}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utterances", type=int, nargs="+", default=[25, 256])
    ap.add_argument("--frames", type=int, default=300)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n = 1024 + 256 * (a.frames - 1)
    cases = []
    for U in a.utterances:
        spec = H.stft_batch([(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(U)], pad_at_end=False)
        assert spec.counts == [a.frames] * U, spec.counts[:3]
        cases += [one_case(y, spec, a.reps) for y in (0, 1, 513)]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "calls_per_window": INNER, "cases": cases}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

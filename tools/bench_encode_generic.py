"""The generic encoder / classifier kernel (csrc/mlp_generic.hip) on the MI355X: device time of one launch beside the resident kernels
at the reference's geometry, beside the module path at a geometry only the generic kernel covers, and at the largest geometry.

    python tools/bench_encode_generic.py [--out profiles/encode_generic.json] [--reps 20] [--utterances 25 256] [--frames 300]

Workload: `--utterances` x `--frames` frames (300 frames: 4.8 s at 16 kHz, 1024 / 256 STFT), complex frames resident on the device,
seeded xavier weights with N(0, 0.05) biases.  Every time is device time from events around 10 calls in a row, the median over `--reps`
such windows after a warm-up window (tools/bench_encode_batch.py's method).
  a  the reference's geometry (z 16, h 128 / 128), y_dim 0 and 513: encode_batch with the generic pack against the resident pack;
     classify_batch (y_dim 1 and 513) likewise.  ratio = generic / resident.
  b  z 32, h (256, 64), y_dim 1: encode_batch with the generic pack against what such a model ran before the generic kernel:
     X2 = |X|^2 as McemBatch holds it ([513, N]) and the label rows ([1, N]) -> torch.cat, torch.t, vae.encoder through the module
     path.  McemBatch.init_parameters with fused_start=True and the pack against the default loop: wall time with a synchronisation at
     the end and device time from events around the call, the median of three calls after a warm-up call.
  c  the largest geometry (z 128, h 512 / 512, y_dim 513): the generic encode_batch and classify_batch alone, with the fraction of the
     157.3 TFLOP/s fp32 matrix peak."""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from packages.models.models import Classifier, DeepGenerativeModel, VariationalAutoencoder
C = importlib.import_module("disentangled-vae_amd.classify")
E = importlib.import_module("disentangled-vae_amd.encode")
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.mcem")
INNER, PEAK_FLOPS = 10, 157.3e12


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


def timed_init(mb, spec, labels, **kw):
    def once():
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        mb.init_parameters(spec, labels, **kw)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
    once()
    runs = [once() for _ in range(3)]
    return {"wall_ms": round(statistics.median(r[0] for r in runs), 3), "device_ms": round(statistics.median(r[1] for r in runs), 3)}


def frozen(m):
    with torch.no_grad():
        for l in m.modules():
            if isinstance(l, torch.nn.Linear):
                l.bias.normal_(0.0, 0.05)
    m = m.cuda().eval()
    for p in m.parameters():
        p.requires_grad = False
    return m


def vae_of(y_dim, z, h):
    torch.manual_seed(1)
    return frozen(VariationalAutoencoder([513, z, list(h)]) if y_dim == 0 else DeepGenerativeModel([513, y_dim, z, list(h)], None))


def labels_of(spec, y_dim):
    if not y_dim:
        return None
    y = (torch.rand((sum(spec.counts), y_dim), device="cuda") > 0.5).float()
    return C.LabelBatch(y, y, spec.counts)


def ratio(a, b):
    return round(a["median"] / b["median"], 3)


def part_a(spec, reps):
    out = []
    for y_dim in (0, 513):
        vae, labels = vae_of(y_dim, 16, (128, 128)), labels_of(spec, y_dim)
        res, gen = (windows(lambda p=E.EncoderPack(vae.encoder, y_dim, generic=g): E.encode_batch(p, spec, labels), reps) for g in (False, True))
        out.append({"op": "encode_batch", "y_dim": y_dim, "resident_ms": res, "generic_ms": gen, "generic_over_resident": ratio(gen, res)})
    for y_dim in (1, 513):
        torch.manual_seed(1)
        clf = frozen(Classifier([513, [128, 128], y_dim]))
        res, gen = (windows(lambda p=C.ClassifierPack(clf, generic=g): C.classify_batch(p, spec), reps) for g in (False, True))
        out.append({"op": "classify_batch", "y_dim": y_dim, "resident_ms": res, "generic_ms": gen, "generic_over_resident": ratio(gen, res)})
    return out


def part_b(spec, reps):
    vae, labels = vae_of(1, 32, (256, 64)), labels_of(spec, 1)
    pack = E.pack_encoder(vae.encoder, 1)
    assert pack.generic
    gen = windows(lambda: E.encode_batch(pack, spec, labels), reps)
    X2 = (spec.frames.abs() ** 2).T.contiguous()                            # [513, N], as McemBatch holds it
    yc = labels.hard.T.contiguous()                                         # [1, N]

    def module_path():
        with torch.no_grad():
            return vae.encoder(torch.t(torch.cat([X2, yc], dim=0)))
    mod = windows(module_path, reps)
    mb = M.McemBatch(vae, niter=1)
    fused = timed_init(mb, spec, labels, fused_start=True, encoder_pack=pack)
    default = timed_init(mb, spec, labels)
    return {"geometry": "z 32, h (256, 64), y_dim 1", "generic_encode_ms": gen, "module_path_ms": mod, "generic_over_module_path": ratio(gen, mod),
            "init_fused_with_pack": fused, "init_default": default}


def part_c(spec, reps):
    frames = sum(spec.counts)
    vae, labels = vae_of(513, 128, (512, 512)), labels_of(spec, 513)
    enc = windows(lambda p=E.pack_encoder(vae.encoder, 513): E.encode_batch(p, spec, labels), reps)
    torch.manual_seed(1)
    clf = frozen(Classifier([513, [512, 512], 513]))
    cl = windows(lambda p=C.pack_classifier(clf): C.classify_batch(p, spec), reps)
    f_enc, f_clf = frames * 2 * (1026 * 512 + 512 * 512 + 512 * 256), frames * 2 * (513 * 512 + 512 * 512 + 512 * 513)
    return {"geometry": "z 128, h (512, 512), y_dim 513", "encode_ms": enc, "encode_mfma_fraction_of_157TFLOPs": round(f_enc / (enc["median"] * 1e-3) / PEAK_FLOPS, 4),
            "classify_ms": cl, "classify_mfma_fraction_of_157TFLOPs": round(f_clf / (cl["median"] * 1e-3) / PEAK_FLOPS, 4)}


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
        cases.append({"utterances": U, "frames": sum(spec.counts), "a": part_a(spec, a.reps), "b": part_b(spec, a.reps), "c": part_c(spec, a.reps)})
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "calls_per_window": INNER, "cases": cases}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

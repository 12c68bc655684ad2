"""Ragged-batch STFT / ISTFT against the single-signal calls, and the MCEM enhancement tail before / after, on the MI355X.

    python tools/bench_stft_batch.py [--out profiles/stft_batch.json] [--reps 15]

Batches of 25, 256 and 1024 utterances of 4-6 s (mixed lengths, float64, already on the device).  Per batch size, in alternation
(one round = one run of each variant, median of the rounds): stft_packed / istft_batch (one launch each), the loop of single-signal
calls over the same utterances (stft_device / istft_device per utterance), and the single-signal kernel on ONE signal of the same
total frame count.  Times are wall clock around the calls with the device synchronised (what a caller waits for); frames/s counts
the batch's frames.  MCEM tail (25 utterances x 300 frames): Wiener gains on the device -> both waveforms of every utterance on the
host, by the numpy path (gains to the host, WF * X in numpy, istft per utterance and estimate) and by McemBatch.enhance()."""
import argparse, importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.mcem")
from packages.processing import stft as ps

KW = dict(fs=16000, wlen_sec=64e-3, hop_percent=0.25)


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


def transforms(U, reps, rng, dev):
    lengths = rng.integers(4 * 16000, 6 * 16000, U).tolist()
    plan = H.plan_stft_batch(lengths, center=False, **KW)
    x = torch.randn(int(plan["padded"].sum()), dtype=torch.float64, device=dev)
    w = H.window_f64("hann", 1024, dev)
    T_total = int(plan["frame_off"][-1])
    sb = H.stft_packed(x, plan["frames"], plan["x0"], plan["padded"], lengths)
    nfr, lens, start = H.istft_plan(sb.counts, None, 1024, 256, False)
    xs = [x[int(a):int(a) + int(p)] for a, p in zip(plan["x0"], plan["padded"])]
    specs = [sb.spec(u) for u in range(U)]
    n_long = (T_total - 1) * 256 + 1024
    x_long = torch.randn(n_long, dtype=torch.float64, device=dev)
    S_long = H.stft_device(x_long, w, 1024, 256, T_total, 2).T
    f = plan["frames"].tolist()
    t = alternate({
        "stft_batch": lambda: H.stft_packed(x, plan["frames"], plan["x0"], plan["padded"], lengths),
        "stft_loop": lambda: [H.stft_device(xu, w, 1024, 256, fu, 2) for xu, fu in zip(xs, f)],
        "stft_one_signal": lambda: H.stft_device(x_long, w, 1024, 256, T_total, 2),
        "istft_batch": lambda: H.istft_batch(sb),
        "istft_loop": lambda: [H.istft_device(s, w, 1024, 256, n, start, ln) for s, n, ln in zip(specs, nfr, lens)],
        "istft_one_signal": lambda: H.istft_device(S_long, w, 1024, 256, T_total, 0, n_long),
    }, reps)
    out = {"utterances": U, "frames": T_total, "samples": int(sum(lengths))}
    for k, v in t.items():
        out[k + "_us"] = round(v * 1e6, 1)
        out[k + "_Mframes_s"] = round(T_total / v / 1e6, 1)
    for k in ("stft", "istft"):
        out[k + "_batch_over_one_signal"] = round(t[k + "_batch"] / t[k + "_one_signal"], 3)
        out[k + "_loop_over_batch"] = round(t[k + "_loop"] / t[k + "_batch"], 2)
    return out


def mcem_tail(reps, rng, dev):
    U, T = 25, 300
    n = (T - 1) * 256 + 1024 - 100                         # end-padded to exactly T frames
    xs = [rng.standard_normal(n) for _ in range(U)]
    sb = H.stft_batch(xs, center=False, **KW)
    assert all(c == T for c in sb.counts), sb.counts[:3]
    mb = M.McemBatch(None)
    mb.spec, mb.counts, mb.X_list = sb, list(sb.counts), None
    mb.starts, mb.ntot = mb._layout(mb.counts, dev)[:2]
    mb.WFs = torch.rand((513, mb.ntot), device=dev)
    mb.WFn = 1 - mb.WFs
    lens = [len(x) for x in xs]

    def host_path():                                       # McemBatch.run's numpy tail + examples/enhance_mcem.py's istft loop (before)
        mb._S_hat = mb._N_hat = None
        mb._estimates()
        return [(ps.istft(s, max_len=m, center=False, **KW), ps.istft(nz, max_len=m, center=False, **KW)) for s, nz, m in zip(mb.S_hat, mb.N_hat, lens)]

    def device_path():                                     # enhance(): one fused-gain launch, both waveforms to the host
        s, nz = mb.enhance(max_len=lens)
        return s.numpy(), nz.numpy()
    a, b = host_path(), device_path()
    assert all(np.array_equal(a[u][0], b[0][u]) and np.array_equal(a[u][1], b[1][u]) for u in range(U))
    t = alternate({"host_path": host_path, "enhance": device_path}, reps)
    return {"utterances": U, "frames_per_utterance": T, "host_path_ms": round(t["host_path"] * 1e3, 3), "enhance_ms": round(t["enhance"] * 1e3, 3),
            "speedup": round(t["host_path"] / t["enhance"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="25,256,1024")
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "batches": [transforms(int(U), a.reps, rng, dev) for U in a.sizes.split(",")],
           "mcem_tail": mcem_tail(a.reps, rng, dev)}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

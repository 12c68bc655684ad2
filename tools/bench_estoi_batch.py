"""McemBatch.estoi against the path it replaces (enhance().numpy() + a numpy STOI per utterance on the host), on the MI355X.

    python tools/bench_estoi_batch.py [--out profiles/estoi_batch.json] [--reps 5] [--utterances 25 256] [--kernel-stats 25=a.csv 256=b.csv] [--no-host]

Synthetic mixtures of 4-6 s at 16 kHz (float64 clean speech on the host, as soundfile returns it), a McemBatch brought to its Wiener
gains by one short EM iteration (the scores' values do not matter here, only the shapes).  In alternation (one round = one run of
each variant, warm-up round excluded, median of the rounds), wall clock with the device synchronised and the U scores on the host at
the end:
  estoi_host_refs    mb.estoi(s, max_len, trim=800).cpu()     clean references as host arrays: packed and uploaded on every call
  estoi_device_refs  the same with the references already packed on the device (WaveBatch)
  host               enhance() -> .numpy() -> tests/estoi_ref.stoi(s, s_hat, 16000, extended=True) per utterance, on 16 worker processes
  scorer_alone       metrics.estoi_batch on resident inputs
Device time of the scorer's six launches: the same script with --no-host --reps 1 --utterances U under `rocprofv3 --kernel-trace
--stats`, one run per batch size (a pass of its own; --no-host leaves the host variant and its worker processes out, so that the
profiler follows one process), whose kernel stats files are merged in with --kernel-stats U=file."""
import argparse, csv, importlib, json, multiprocessing, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import estoi_ref as R
TRIM = 800
HOST_PROCESSES = 16


def host_estoi(args):
    s, w = args
    return R.stoi(s[TRIM:-TRIM], w.astype(np.float64)[TRIM:-TRIM], 16000, True)


def wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def alternate(variants, reps, sync):
    """variants: name -> callable; every round runs each once (warm-up round first); median seconds per name."""
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(wall(fn, sync))
    return {k: statistics.median(v) for k, v in times.items()}


def speechlike(n, rng):
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n]
    return env * rng.standard_normal(n) * 0.3 * np.sin(2 * np.pi * 220 * np.arange(n) / 16000) + 0.003 * rng.standard_normal(n)


def one(U, reps, vae, pool):
    import torch
    H = importlib.import_module("disentangled-vae_amd.stft")
    M = importlib.import_module("disentangled-vae_amd.metrics")
    McemBatch = importlib.import_module("disentangled-vae_amd.mcem").McemBatch
    rng = np.random.default_rng(U)
    speech = [speechlike(int(n), rng) for n in rng.integers(4 * 16000, 6 * 16000, U)]
    lengths = [len(s) for s in speech]
    X = H.stft_batch([s + 0.1 * rng.standard_normal(len(s)) for s in speech], center=False, pad_at_end=True)
    mb = McemBatch(vae, niter=1, nsamples_E_step=2, burnin_E_step=2, nsamples_WF=2, burnin_WF=2)
    mb.init_parameters(X, [np.ones((1, T), np.float32) for T in X.counts])
    mb.run()
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    s_dev = H.WaveBatch(torch.from_numpy(np.concatenate(speech)).cuda(), offsets, lengths)

    def host():
        s_hat, _ = mb.enhance(max_len=lengths)
        return np.array(pool.map(host_estoi, list(zip(speech, s_hat.numpy())), chunksize=max(1, U // 64)))
    variants = {"estoi_host_refs": lambda: mb.estoi(speech, max_len=lengths, trim=TRIM).cpu().numpy(),
                "estoi_device_refs": lambda: mb.estoi(s_dev, max_len=lengths, trim=TRIM).cpu().numpy()}
    if pool is not None:
        variants["host"] = host
        want = host()
        for k in ("estoi_host_refs", "estoi_device_refs"):
            assert np.allclose(variants[k](), want, rtol=0, atol=1e-7), k
    t = alternate(variants, reps, torch.cuda.synchronize)
    s_hat, _ = mb.enhance(max_len=lengths)
    t["scorer_alone"] = alternate({"scorer_alone": lambda: M.estoi_batch(s_dev, s_hat, 16000, trim=TRIM).cpu()}, reps, torch.cuda.synchronize)["scorer_alone"]
    res = {"samples": int(sum(lengths))}
    res.update({k + "_ms": round(v * 1e3, 3) for k, v in t.items()})
    if pool is not None:
        res["host_processes"] = HOST_PROCESSES
        res["host_over_estoi_host_refs"] = round(t["host"] / t["estoi_host_refs"], 1)
        res["host_over_estoi_device_refs"] = round(t["host"] / t["estoi_device_refs"], 1)
    return res


def kernel_stats(path):
    """The es_* rows of a rocprofv3 kernel stats file: name -> calls / average / min / max in microseconds."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "dvae::es_" in row["Name"]:
                name = row["Name"].split("dvae::")[1].split("(")[0]
                out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--utterances", type=int, nargs="+", default=[25, 256])
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="U=CSV",
                    help="rocprofv3 --kernel-trace --stats csv of a `--reps 1 --utterances U` run of this script, per batch size")
    ap.add_argument("--no-host", action="store_true", help="leave the host variant (and its worker processes) out: for traced runs")
    a = ap.parse_args()
    # the host path's workers start before the GPU is opened and never touch it (numpy only)
    pool = None if a.no_host else multiprocessing.get_context("spawn").Pool(HOST_PROCESSES)
    import torch
    from packages.models.models import DeepGenerativeModel
    torch.manual_seed(0)
    vae = DeepGenerativeModel([513, 1, 16, [128, 128]], None).cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False
    res = {"device": torch.cuda.get_device_name(0), "trim": TRIM, "reps": a.reps}
    for U in a.utterances:
        res[f"utterances_{U}"] = one(U, a.reps, vae, pool)
    if pool is not None:
        pool.close()
        pool.join()
    for item in a.kernel_stats:
        U, path = item.split("=", 1)
        res.setdefault(f"utterances_{U}", {})["kernel_trace_us"] = kernel_stats(path)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""McemBatch.score against the path it replaces (enhance().numpy() + packages.metrics.energy_ratios per utterance), on the MI355X.

    python tools/bench_metrics_batch.py [--out profiles/metrics_batch.json] [--reps 10] [--utterances 25 256] [--kernel-stats 25=a.csv 256=b.csv]

Synthetic mixtures of 4-6 s (speech + noise, float64 on the host as soundfile returns the clean references), a McemBatch brought to
its Wiener gains by one short EM iteration (the scores' values do not matter here, only the shapes).  In alternation (one round = one
run of each variant, median of the rounds), wall clock with the device synchronised and the three scores of every utterance on the
host at the end:
  score_host_refs    mb.score(s, n, max_len, trim=800).cpu()   clean references as host arrays: packed and uploaded on every call
  score_device_refs  the same with the references already packed on the device (WaveBatch): what an evaluation loop keeps resident
  host               enhance() -> .numpy() -> energy_ratios(s_hat[800:-800], ...) per utterance in numpy
All three agree within the test suite's bounds (checked first, loosely).  Device time of the scorer's three launches: the same
script with --reps 1 --utterances U under `rocprofv3 --kernel-trace --stats`, one run per batch size, whose kernel stats files are
merged in with --kernel-stats U=file."""
import argparse, csv, importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from packages import metrics as PM
from packages.models.models import DeepGenerativeModel
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.metrics")
McemBatch = importlib.import_module("disentangled-vae_amd.mcem").McemBatch
TRIM = 800


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


def device_batch(arrays):
    lengths = [len(a) for a in arrays]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return H.WaveBatch(torch.from_numpy(np.concatenate(arrays)).cuda(), offsets, lengths)


def one(U, reps, vae):
    rng = np.random.default_rng(U)
    speech = [speechlike(int(n), rng) for n in rng.integers(4 * 16000, 6 * 16000, U)]
    noise = [0.1 * rng.standard_normal(len(s)) for s in speech]
    lengths = [len(s) for s in speech]
    X = H.stft_batch([a + b for a, b in zip(speech, noise)], center=False, pad_at_end=True)
    mb = McemBatch(vae, niter=1, nsamples_E_step=2, burnin_E_step=2, nsamples_WF=2, burnin_WF=2)
    mb.init_parameters(X, [np.ones((1, T), np.float32) for T in X.counts])
    mb.run()
    s_dev, n_dev = device_batch(speech), device_batch(noise)

    def host():
        s_hat, _ = mb.enhance(max_len=lengths)
        return np.array([PM.energy_ratios(w.astype(np.float64)[TRIM:-TRIM], s[TRIM:-TRIM], n[TRIM:-TRIM])
                         for w, s, n in zip(s_hat.numpy(), speech, noise)])
    variants = {"score_host_refs": lambda: mb.score(speech, noise, max_len=lengths, trim=TRIM).cpu().numpy(),
                "score_device_refs": lambda: mb.score(s_dev, n_dev, max_len=lengths, trim=TRIM).cpu().numpy(),
                "host": host}
    want = host()
    for k in ("score_host_refs", "score_device_refs"):
        assert np.allclose(variants[k](), want, rtol=0, atol=1e-6), k
    t = alternate(variants, reps)
    # the scorer alone, inputs resident: what the three launches and the [U, 3] read-back cost next to enhance()
    s_hat, _ = mb.enhance(max_len=lengths)
    t["scorer_alone"] = alternate({"scorer_alone": lambda: M.energy_ratios_batch(s_hat, s_dev, n_dev, trim=TRIM).cpu()}, reps)["scorer_alone"]
    res = {"samples": int(sum(lengths))}
    res.update({k + "_ms": round(v * 1e3, 3) for k, v in t.items()})
    res["host_over_score_host_refs"] = round(t["host"] / t["score_host_refs"], 1)
    res["host_over_score_device_refs"] = round(t["host"] / t["score_device_refs"], 1)
    return res


def kernel_stats(path):
    """The si_* rows of a rocprofv3 kernel stats file: name -> calls / average / min / max in microseconds."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "dvae::si_" in row["Name"]:
                name = row["Name"].split("dvae::")[1].split("(")[0]
                out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--utterances", type=int, nargs="+", default=[25, 256])
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="U=CSV",
                    help="rocprofv3 --kernel-trace --stats csv of a `--reps 1 --utterances U` run of this script, per batch size")
    a = ap.parse_args()
    torch.manual_seed(0)
    vae = DeepGenerativeModel([513, 1, 16, [128, 128]], None).cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False
    res = {"device": torch.cuda.get_device_name(0), "trim": TRIM, "reps": a.reps}
    for U in a.utterances:
        res[f"utterances_{U}"] = one(U, a.reps, vae)
    for item in a.kernel_stats:
        U, path = item.split("=", 1)
        # every launch of the traced run (warm-up, check and one round of each variant), all with n
        res.setdefault(f"utterances_{U}", {})["kernel_trace_us"] = kernel_stats(path)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""dvae_resample_batch on the MI355X: device time of the three cases of DESIGN section 8, against what the arithmetic and the data need.

    python tools/bench_resample_batch.py [--out profiles/resample_batch.json] [--reps 20] [--minutes 10] [--kernel-stats a.csv]

  a  512 signals x 5 s, 16 kHz -> 10 kHz (5 / 8, 117 taps per output): the job of es_resample_kernel inside stoi_batch, which
     resamples two signals per utterance -- the same sample count as stoi_batch of 256 x 5 s, which this script also runs once so
     that a `rocprofv3 --kernel-trace --stats` run of it (a run of its own, --reps 1) holds both kernels; --kernel-stats merges the
     es_resample_kernel and rs_resample_kernel rows of that run's csv into the result
  b  4 recordings x `--minutes` min, 48 kHz -> 16 kHz (1 / 3, 219 taps per output)
  c  4 recordings x `--minutes` min, 44.1 kHz -> 16 kHz (160 / 441, 200 taps per output, the per-lane walk of the phase-major taps)
  device_ms      one dvae_resample_batch call (resample_packed: table upload, one launch) from events around 10 calls in a row, the
                 median over `--reps` such windows after a warm-up window; float32 inputs resident on the device, float64 outputs
  fma_fraction   outputs x taps per output over the device time, as a fraction of the vector-FP64 peak (256 CUs x 64 fma / clock x
                 2.4 GHz = 39.3e12 fma / s)
  hbm_fraction   bytes (input once + output once) over the device time, as a fraction of 8 TB/s
Also the worst |device - restatement| in units of the derived bound (tests/estoi_bounds.py) over one short signal per case."""
import argparse, csv, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import estoi_bounds as EB
import estoi_ref as ER
RS = importlib.import_module("disentangled-vae_amd.resample")
M = importlib.import_module("disentangled-vae_amd.metrics")
R = importlib.import_module("disentangled-vae_amd.ragged")
INNER, PEAK_BYTES_PER_S, PEAK_FMA_PER_S = 10, 8e12, 256 * 64 * 2.4e9


def device_ms(buf, t, taps, p, q, reps):
    out = None

    def window():
        nonlocal out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            out = RS.resample_packed(buf, t["table"], taps, p, q, n_out=t["n_out"], out=out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER
    window()
    return [window() for _ in range(reps)]


def one_case(name, fs_in, fs_out, count, samples, reps, rng):
    taps, p, q, L = RS.resample_taps(fs_in, fs_out)
    dev = R.device()
    buf = (0.1 * torch.randn(count * samples, dtype=torch.float32, device=dev))
    t = RS.resample_tables((np.arange(count) * samples, [samples] * count, buf.numel()), p, q, L)
    ms = device_ms(buf, t, taps, p, q, reps)
    d = statistics.median(ms)
    outputs, nt = int(t["out_len"].sum()), 2 * L // p + 1
    x = rng.standard_normal(3001)
    got = RS.resample_batch([x], fs_in, fs_out).numpy()[0]
    worst = float(np.max(np.abs(got - ER.resample(x, None, (taps, p, q, L))) / EB.resample_bound(x, (taps, p, q, L))))
    nbytes = count * samples * 4 + outputs * 8
    return {"case": name, "fs_in": fs_in, "fs_out": fs_out, "p": p, "q": q, "L": L, "taps_per_output": nt, "run": t["run"],
            "signals": count, "samples_per_signal": samples, "outputs": outputs, "work_items": t["n_items"],
            "device_ms": round(d, 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
            "fma": outputs * nt, "fma_fraction_of_fp64_peak": round(outputs * nt / (d * 1e-3) / PEAK_FMA_PER_S, 4),
            "bytes": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (d * 1e-3) / PEAK_BYTES_PER_S, 5),
            "worst_error_in_units_of_bound": round(worst, 4)}


def kernel_stats(path):
    """The resampler rows of a rocprofv3 kernel stats file: name -> calls / average / min / max in microseconds."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "es_resample_kernel" in row["Name"] or "rs_resample_kernel" in row["Name"]:
                name = row["Name"].split("dvae::")[-1].split("(")[0]
                out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--minutes", type=float, default=10.0, help="length of each of the four recordings of cases b and c")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="rocprofv3 --kernel-trace --stats csv of a `--reps 1` run of this script")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    cases = [one_case("a", 16000, 10000, 512, 5 * 16000, a.reps, rng),
             one_case("b", 48000, 16000, 4, int(a.minutes * 60 * 48000), a.reps, rng),
             one_case("c", 44100, 16000, 4, int(a.minutes * 60 * 44100), a.reps, rng)]
    # the parent's only device resampler, on the sample count of case a: two signals of 256 utterances of 5 s (a kernel trace times it)
    xy = [0.1 * torch.randn(256 * 5 * 16000, dtype=torch.float32, device="cuda") for _ in range(2)]
    t = M.stoi_tables([(np.arange(256) * 80000, [80000] * 256)] * 2, [xy[0].numel()] * 2, 16000)
    M.stoi_packed(xy, t, True)
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "calls_per_window": INNER, "cases": cases}
    if a.kernel_stats:
        res["kernel_trace_us"] = kernel_stats(a.kernel_stats)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

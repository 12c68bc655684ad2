"""mix_at_snr_batch against the path it replaces (the mixing of scripts/create_test_set.py per utterance in numpy on 16 processes, then
the upload of its three outputs), on the MI355X.

    python tools/bench_mix_batch.py [--out profiles/mix_batch.json] [--reps 20] [--utterances 32] [--seconds 5] [--kernel-stats a.csv]

The batch: `--utterances` speech-like signals of `--seconds` under 2 noise banks x 4 SNRs (condition_grid: 256 mixtures of 5 s by
default, every utterance's speech read by 8 of them), float32 inputs resident on the device, float64 outputs.
  device_ms      the device time of one dvae_mix_snr_batch call (mix_packed: table upload, five launches), from events around 20 calls
                 in a row, the median over `--reps` such windows after a warm-up window
  wall_ms        the wall clock of mix_at_snr_batch from host lists (packing, upload, call, synchronise), median of the rounds
  host_ms        tests/mix_ref.mix_one per mixture on a pool of 16 processes (forked before the GPU is opened; they never open it), the
                 three outputs of every mixture packed and uploaded; same rounds, alternating with wall_ms
  bytes          what the algorithm needs: every mixture's speech and noise read once, three outputs written once
  hbm_fraction   bytes / device time over 8 TB/s.  The kernels read the inputs once per pass (four passes), so 1 is not reachable.
Also the worst |device - reference| over the cases of tests/golden/mix_golden.npz in units of the derived bound (tests/mix_bounds.py).
Kernel times: the same script with --reps 1 under `rocprofv3 --kernel-trace --stats`, merged in with --kernel-stats."""
import argparse, csv, importlib, json, multiprocessing, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import mix_bounds as XB
import mix_ref as XR
X = importlib.import_module("disentangled-vae_amd.mix")
R = importlib.import_module("disentangled-vae_amd.ragged")
SNRS, INNER, PROCS, PEAK_BYTES_PER_S = [-10.0, -5.0, 0.0, 5.0], 20, 16, 8e12
DATA = {}


def speechlike(n, rng):
    env = np.repeat((rng.random(n // 1600 + 1) > 0.4).astype(np.float64), 1600)[:n]
    return (env * rng.standard_normal(n) * 0.3 + 0.003 * rng.standard_normal(n)).astype(np.float32)


def host_one(c):
    r = XR.mix_one(DATA["grid"][c], DATA["banks"][DATA["index"][c]], DATA["starts"][c], DATA["snr"][c])
    return r["speech"], r["noise"], r["mixture"]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def golden_worst():
    gold = XR.load_golden(os.path.join(ROOT, "tests", "golden", "mix_golden.npz"))
    names = sorted(gold)
    cases = [gold[n] for n in names]
    mb = X.mix_at_snr_batch([c["speech"] for c in cases], [c["bank"] for c in cases], list(range(len(cases))), [c["start"] for c in cases],
                            [c["snr_db"] for c in cases])
    parts, stats = [b.numpy() for b in (mb.speech, mb.noise, mb.mixture)], mb.stats.cpu().numpy()
    out = {}
    for u, (name, c) in enumerate(zip(names, cases)):
        ref = XR.mix_one(c["speech"], c["bank"], c["start"], c["snr_db"])
        got = dict(speech=parts[0][u], noise=parts[1][u], mixture=parts[2][u], k=stats[u, 3], norm=stats[u, 4])
        out[name] = {k: round(v, 5) for k, v in XB.worst(got, ref).items()}
        out[name]["achieved_minus_requested_db"] = float(stats[u, 5] - c["snr_db"])
        out[name]["bound_noise"] = XB.bounds(len(c["speech"]))["noise"]
    return out


def kernel_stats(path):
    """The mix_* rows of a rocprofv3 kernel stats file: name -> calls / average / min / max in microseconds."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "dvae::mix_" in row["Name"]:
                name = row["Name"].split("dvae::")[1].split("(")[0]
                out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="rocprofv3 --kernel-trace --stats csv of a `--reps 1` run of this script")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n = int(16000 * a.seconds)
    speech = [speechlike(n, rng) for _ in range(a.utterances)]
    banks = [(0.1 * rng.standard_normal(60 * 16000)).astype(np.float32) for _ in range(2)]
    si, index, snr = X.condition_grid(a.utterances, len(banks), SNRS)
    grid = [speech[u] for u in si]
    starts = X.draw_noise_starts(np.random.default_rng(1), [len(b) for b in banks], index, [len(g) for g in grid])
    DATA.update(grid=grid, banks=banks, index=index, starts=starts, snr=snr)
    pool = multiprocessing.get_context("fork").Pool(PROCS)              # before the first GPU call: the workers never open the device
    U = len(grid)

    # device time: inputs resident, the table and the factors made once on the host
    s_view, b_view = R.view(grid, dedupe=True), R.view(banks, dedupe=True)
    tab = X.mix_tables(s_view[:2], (b_view[0], b_view[1], index), starts, None, (s_view[2], b_view[2]))
    factors = X.snr_factors(snr)
    dev = R.device()
    s_buf, b_buf = (R.pack(x, f"mix_at_snr_batch: {name}", dev, R.ENTRY, dedupe=True) for x, name in ((grid, "speech"), (banks, "noise_banks")))
    outs = None

    def window():
        nonlocal outs
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            outs = X.mix_packed(s_buf, b_buf, tab, factors, outputs=outs[:3] if outs else None)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / INNER
    window()
    device = [window() for _ in range(a.reps)]

    def batch():
        return X.mix_at_snr_batch(grid, banks, index, starts, snr)

    def host():
        res = pool.map(host_one, range(U), chunksize=max(1, U // (4 * PROCS)))
        for k in range(3):
            buf = torch.empty(U * n, dtype=torch.float64, pin_memory=True)
            h = buf.numpy()
            for c, r in enumerate(res):
                h[c * n:(c + 1) * n] = r[k]
            buf.to(dev, non_blocking=True)
        return res
    want, got = host(), batch()
    worst = 0.0
    for c in (0, U // 2, U - 1):                                         # loosely: the two paths make the same mixtures
        worst = max(worst, float(np.max(np.abs(got.mixture.numpy()[c] - want[c][2]))))
    assert worst < 1e-9, worst
    times = {"wall": [], "host": []}
    for _ in range(max(3, a.reps // 4)):
        times["wall"].append(wall(batch))
        times["host"].append(wall(host))
    pool.close()
    pool.join()

    nbytes = U * n * (4 + 4 + 3 * 8)
    d = statistics.median(device)
    res = {"device": torch.cuda.get_device_name(0), "mixtures": U, "utterances": a.utterances, "noise_banks": len(banks), "snrs": SNRS,
           "samples_per_mixture": n, "reps": a.reps, "calls_per_window": INNER,
           "launches_per_call": 5, "work_items": int(tab[U]),
           "device_ms": round(d, 4), "device_ms_min": round(min(device), 4), "device_ms_max": round(max(device), 4),
           "bytes": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (d * 1e-3) / PEAK_BYTES_PER_S, 4),
           "wall_ms": round(statistics.median(times["wall"]) * 1e3, 3), "host_ms": round(statistics.median(times["host"]) * 1e3, 3),
           "host_processes": PROCS, "host_over_wall": round(statistics.median(times["host"]) / statistics.median(times["wall"]), 1),
           "golden_worst_in_units_of_bound": golden_worst()}
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

"""The generic Metropolis-Hastings chain (csrc/mcem_generic.hip) measured on the MI355X:

  (a) at the reference's decoder ([16+1]-128-128-513), the generic chain beside the hand-tuned fp32 chain on the same inputs:
      one utterance and 25 utterances of 300 frames, 40 chain steps, device time per chain step (the two kernels alternating, median of --rounds windows of --reps launches);
  (b) a z 32 / h (256, 64) / y 1 model through McemBatch.run at the reference's settings (niter 100, 10 + 30, 25 + 75, rank 10),
      1 and 25 utterances of 300 frames;
  (c) the same model's host path (ATen on the CPU, the drop-in class), extrapolated from --cpu-iters EM iterations.

Prints one JSON line.  --skip a b c leaves parts out."""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import golden_util as gu, mcem_cases as mc
from impl_modules import build_model

mcem_dev = importlib.import_module("disentangled-vae_amd.mcem")
NIT, BURNIN, FRAMES = 40, 30, 300


def model_of(z_dim, h_dim, device, y_dim=1, seed=3):
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=z_dim, h_dim=tuple(h_dim))
    m = build_model("M2", dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in gu.make_params("M2", dims, seed).items()})
    m.eval().to(device)
    for p in m.parameters():
        p.requires_grad = False
    return m, dims


def device_time_us(fn, reps):
    """Mean device time of fn() in microseconds over `reps` calls after two warm-up calls (events around the whole run)."""
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def part_a(reps, rounds):
    m, _ = model_of(16, (128, 128), "cuda")
    out = {}
    for U in (1, 25):
        n = U * FRAMES
        gen = torch.Generator(device="cuda"); gen.manual_seed(U)
        X2 = torch.randn(513, n, device="cuda", generator=gen).square_().add_(1e-4)
        Vb = torch.rand(513, 10, device="cuda", generator=gen) @ torch.rand(10, n, device="cuda", generator=gen)
        y = (torch.rand(1, n, device="cuda", generator=gen) > 0.5).float()
        Z = torch.randn(16, n, device="cuda", generator=gen)
        g = torch.ones(n, device="cuda")
        noise = torch.randn(NIT, 16, n, device="cuda", generator=gen)
        logu = torch.rand(NIT, n, device="cuda", generator=gen).log_()
        packs = {name: mcem_dev.DecoderPack(m.decoder, 1, "fp32", generic=generic) for name, generic in (("specialised", False), ("generic", True))}
        runs = {name: [] for name in packs}
        for _ in range(rounds):                                     # the two kernels alternate: other work shares the host
            for name, pack in packs.items():
                runs[name].append(device_time_us(lambda: pack.sample(Z, y, g, Vb, X2, noise, logu, BURNIN, want_vs=False), reps) / NIT)
        for name, v in runs.items():
            out[f"{name}_u{U}_us_per_chain_step"] = dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))
    return out


def utterances(U, dims, seed=5):
    mc.DIMS["bench_generic"] = dims
    X, Y = [], []
    for u in range(U):
        x, _, y = mc.make_utterance(dict(seed=seed + u, N=FRAMES, model="bench_generic"))
        X.append(x); Y.append(y)
    return X, Y


def part_b(rounds):
    m, dims = model_of(32, (256, 64), "cuda")
    out = {}
    for U in (1, 25):
        X, Y = utterances(U, dims)
        times = []
        for r in range(rounds + 1):                                 # the first run warms up (code objects, allocator) and is dropped
            mb = mcem_dev.McemBatch(m, niter=100)
            torch.manual_seed(r)
            mb.init_parameters(X, Y)
            assert mb._pack.generic
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cost = mb.run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            assert np.isfinite(cost).all()
        times = times[1:]
        out[f"batch_u{U}_s"] = dict(median=round(float(np.median(times)), 4), min=round(min(times), 4), max=round(max(times), 4))
        out[f"batch_u{U}_utt_per_s"] = round(U / float(np.median(times)), 2)
    return out


def part_c(iters):
    from packages.models import mcem
    m, dims = model_of(32, (256, 64), "cpu")
    X, Y = utterances(1, dims)
    mc.DIMS["bench_generic"] = dims
    _, S, _ = mc.make_utterance(dict(seed=5, N=FRAMES, model="bench_generic"))
    em = mcem.MCEM_M2(niter=iters, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75)
    torch.manual_seed(0)
    em.init_parameters(X=X[0], S=S, y=torch.from_numpy(Y[0]), vae=m, nmf_rank=10, eps=mc.EPS, device="cpu")
    t0 = time.perf_counter()
    em.run()
    dt = time.perf_counter() - t0
    # an EM iteration runs 2 * 40 + 10 decoder passes per frame, the final Wiener chain 2 * 100 + 25: `iters` iterations and the
    # tail were timed together, 100 iterations are extrapolated by decoder passes
    unit = dt / (iters * 90 + 225)
    return dict(cpu_iters=iters, cpu_s=round(dt, 3), cpu_100_iterations_s=round(unit * (100 * 90 + 225), 2), cpu_threads=torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="chain launches per timed window of (a)")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per kernel in (a), timed runs per batch size in (b)")
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["a", "b", "c"])
    a = ap.parse_args()
    res = {}
    if "a" not in a.skip:
        res.update(part_a(a.reps, a.rounds))
    if "b" not in a.skip:
        res.update(part_b(a.rounds))
    if "c" not in a.skip:
        res.update(part_c(a.cpu_iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The batched M-step and the fused EM iteration (McemBatch) against the float64 oracle, at the shapes the batch path runs:
every frames-per-workgroup variant of the register-resident frames kernel (4 / 8 / 16, forced and as selected), the W update's
straight-line form and its double-buffered loop, the three-pass kernels (R > 10 kept samples, ranks other than 10), ragged
batches with padding, the lazy and the three-launch iteration.  The EM iteration runs on the weight-stationary chain, which writes
the final state itself (every model, the 513-row labels included), and -- the "-stream" cases, DVAE_MCEM_CHAIN=stream -- on the streaming
chain of csrc/mcem.hip, where last_sample_kernel writes Z over the chain's own initial state."""
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import golden_util as gu
from impl_modules import build_model
from oracle import mcem_oracle as mo

pytestmark = pytest.mark.gpu
mcem_dev = importlib.import_module("disentangled-vae_amd.mcem")
native = importlib.import_module("disentangled-vae_amd.native")

F = 513
# the segment lengths where the kernels branch: one frame, either side of a 16- and a 32-frame tile, the W update's straight-line
# limit (5 steps of 64 = 320 frames) and its loop with an even (321, 640) and an odd (641) step count, a long utterance
EDGE_COUNTS = [1, 15, 16, 17, 31, 32, 33, 320, 321, 640, 641, 1500]
LAYOUTS = {
    "u1": [1500],                                               # (no tables: m_step_, unpadded)
    "u1n1": [1],
    "u1n17": [17],
    "u1tab": [641],
    "u3": [33, 1537, 16],
    "u25mixed": EDGE_COUNTS + [47, 300, 299, 128, 96, 250, 181, 64, 200, 77, 310, 5, 150],
    "u48": [int(c) for c in np.random.default_rng(48).integers(40, 300, 48)],
    "u25x300": [300] * 25,                                      # the benchmarked batch: 8000 padded frames
    "t1024": [256] * 4,                                         # padded totals on either side of the 4 -> 8 -> 16 frame switch
    "t1056": [256, 256, 256, 257],
    "t2048": [512] * 4,
    "t2080": [512, 512, 512, 513],
}


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def layout(counts):
    """McemBatch's frame axis: every utterance starts on a multiple of 32 frames; one segment-table entry per 32 frames."""
    starts, pos = [], 0
    for c in counts:
        starts.append(pos)
        pos += (c + 31) // 32 * 32
    tile_seg = np.concatenate([np.full((c + 31) // 32, u, np.int32) for u, c in enumerate(counts)])
    return starts, pos, tile_seg


def default_frames(n):
    """What mstep::frames_per_workgroup selects without DVAE_MSTEP_FRAMES (csrc/mcem_mstep.hip)."""
    return 4 if (n + 3) // 4 <= 256 else (8 if (n + 7) // 8 <= 256 else 16)


def mixture_stft(n_frames, seed, level=0.05):
    """Complex STFT (513, n_frames) of a synthetic mixture: voiced bursts (harmonics of a random f0, 50 ms on / off) over a white-noise
    floor, Hann window 1024, hop 256, no centring.  The noise floor keeps every frame away from zero (the reference's own updates give 0/0
    on an all-zero frame); |X|^2 spans about ten decades, from the harmonic peaks to the deepest noise bins.  level: peak amplitude of
    the waveform.  At 0.05 the loudest bins are of the order of the test decoders' variances (a trained prior tracks the spectrum), and
    the geometric mean of |X|^2 sits far from 1 / e, so no utterance's cost -- a mean of log Vx + X2 / Vx -- is near zero, where a
    relative bound on it would only measure cancellation."""
    rng = np.random.default_rng(seed)
    n = 1024 + 256 * (n_frames - 1)
    tt = np.arange(n) / 16000.0
    f0 = 100.0 + 120.0 * rng.random()
    env = np.repeat(rng.random(n // 800 + 1) > 0.4, 800)[:n]
    s = sum((0.3 / h) * np.sin(2 * np.pi * h * f0 * tt + 6.283 * rng.random()) for h in range(1, 13)) * env
    x = level * (s + 0.02 * rng.standard_normal(n))
    frames = np.lib.stride_tricks.sliding_window_view(x, 1024)[::256] * np.hanning(1024)
    return np.fft.rfft(frames, axis=1).T.astype(np.complex64)


def power(X):
    return (np.abs(X) ** 2).astype(np.float32)                 # McemBatch.init_parameters' |X|^2


# ------------------------------------------------------------------------------------------------------------------------------
# 1. batched M-step vs the float64 oracle, per utterance

def mstep_inputs(counts, R, K, seed, kind, tables):
    rng = np.random.default_rng(seed)
    if tables:
        starts, n, tile_seg = layout(counts)
    else:
        starts, n, tile_seg = [0], counts[0], None
    U = len(counts)
    live = np.zeros(n, bool)
    # padding columns: X2 = 1 as McemBatch lays it out; H, g, Vb hold values of their own, which the M-step must leave alone
    X2 = np.ones((F, n), np.float32)
    Vs = rng.random((R, F, n), np.float32) + np.float32(0.5)
    H = (rng.random((K, n)) + 2.0).astype(np.float32)
    g = (rng.random(n) + 2.0).astype(np.float32)
    Vb = (rng.random((F, n)) + 2.0).astype(np.float32)
    W = np.maximum(rng.random((U, F, K)), 1e-6).astype(np.float32)
    for u, (s, c) in enumerate(zip(starts, counts)):
        sl = slice(s, s + c)
        live[sl] = True
        if kind == "stft":
            x2 = power(mixture_stft(c, 1000 * seed + u))
            vs = x2 * (rng.random((R, F, c), np.float32) * np.float32(1.9) + np.float32(0.1))          # variances that follow the spectrum
        else:                                                                          # iid log-normal
            x2 = np.exp(2.5 * rng.standard_normal((F, c)) - 1.0)
            vs = np.exp(np.float32(2.5) * rng.standard_normal((R, F, c), np.float32) - np.float32(1.0))
        X2[:, sl] = x2
        Vs[:, :, sl] = vs
        H[:, sl] = np.maximum(rng.random((K, c)), 1e-6)
        g[sl] = np.exp(0.3 * rng.standard_normal(c))
        Vb[:, sl] = W[u] @ H[:, sl]
    if kind == "stft" and live.sum() >= 64:
        assert X2[:, live].min() > 0 and X2[:, live].max() / X2[:, live].min() > 1e8
    return dict(starts=starts, counts=counts, n=n, tile_seg=tile_seg, live=live, X2=X2, Vs=Vs, W=W, H=H, g=g, Vb=Vb)


def oracle_m_steps(inp):
    """mcem_oracle.m_step in float64 on every utterance's own columns (numpy releases the GIL: one utterance per thread)."""
    X2, Vs = inp["X2"], inp["Vs"]

    def one(u):
        sl = slice(inp["starts"][u], inp["starts"][u] + inp["counts"][u])
        return mo.m_step(X2[:, sl], Vs[:, :, sl], inp["W"][u], inp["H"][:, sl], inp["g"][sl], inp["Vb"][:, sl], dtype=np.float64)
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, range(len(inp["counts"]))))


def check_m_step(inp, W, H, g, Vb, cost, err=""):
    """Device M-step outputs (numpy) against the float64 oracle per utterance; padding columns untouched.  cost None: checked by the
    caller (a lazy iteration forms it later).  Returns the oracle's costs."""
    ref = oracle_m_steps(inp)
    for u, (s, c) in enumerate(zip(inp["starts"], inp["counts"])):
        sl = slice(s, s + c)
        Wo, Ho, go, Vbo, _, co = ref[u]
        msg = f"{err} utterance {u} ({c} frames)"
        np.testing.assert_allclose(W[u], Wo, rtol=1e-4, atol=1e-9, err_msg="W " + msg)
        np.testing.assert_allclose(H[:, sl], Ho, rtol=1e-4, atol=1e-9, err_msg="H " + msg)
        np.testing.assert_allclose(g[sl], go, rtol=1e-4, err_msg="g " + msg)
        np.testing.assert_allclose(Vb[:, sl], Vbo, rtol=1e-4, atol=1e-9, err_msg="Vb " + msg)
        if cost is not None:
            np.testing.assert_allclose(cost[u], co, rtol=1e-5, err_msg="cost " + msg)
    pad = ~inp["live"]
    np.testing.assert_array_equal(H[:, pad], inp["H"][:, pad], err_msg="H padding " + err)
    np.testing.assert_array_equal(g[pad], inp["g"][pad], err_msg="g padding " + err)
    np.testing.assert_array_equal(Vb[:, pad], inp["Vb"][:, pad], err_msg="Vb padding " + err)
    return np.array([r[5] for r in ref])


def run_m_step(inp, tables):
    dW, dH, dg, dVb = t(inp["W"]), t(inp["H"]), t(inp["g"]), t(inp["Vb"])
    if tables:
        i32 = lambda a: torch.tensor(np.asarray(a, np.int32), device="cuda")
        cost = mcem_dev.m_step_batch_(t(inp["X2"]), t(inp["Vs"]), dW, dH, dg, dVb, i32(inp["starts"]), i32(inp["counts"]), i32(inp["tile_seg"]))
    else:
        dW1 = dW[0].contiguous()
        cost = mcem_dev.m_step_(t(inp["X2"]), t(inp["Vs"]), dW1, dH, dg, dVb)
        dW = dW1[None]
    return dW.cpu().numpy(), dH.cpu().numpy(), dg.cpu().numpy(), dVb.cpu().numpy(), cost.cpu().numpy()


def _mcase(layout_name, R, K, frames=None, mstep=None, kind="stft"):
    """frames: DVAE_MSTEP_FRAMES (None: the default selection); mstep: DVAE_MSTEP."""
    counts = LAYOUTS[layout_name]
    tables = layout_name not in ("u1", "u1n1", "u1n17")
    n = layout(counts)[1] if tables else counts[0]
    reg = R <= 10 and K == 10 and mstep != "3pass"
    if not reg:
        form = "3pass" + ("-forced" if mstep == "3pass" else "")
    else:
        form = f"fpw{frames or default_frames(n)}" + ("" if frames else "-default")
    if form.startswith("fpw16") and ((n + 15) // 16) % 16:
        form += "-tail"                                         # a last group of fewer than 16 workgroups: not remapped in XCD pairs
    loop = any(c > 320 for c in counts)
    pid = f"{form}-{layout_name}-N{n}-R{R}-K{K}-{kind}" + ("-wregloop" if loop and reg else "")
    return pytest.param(layout_name, R, K, frames, mstep, kind, id=pid)


MSTEP_CASES = [
    # register form (R <= 10, rank 10): frames per workgroup forced, on the batch with every edge length
    _mcase("u25mixed", 10, 10, frames=4), _mcase("u25mixed", 10, 10, frames=8), _mcase("u25mixed", 10, 10, frames=16),
    _mcase("u25mixed", 3, 10, frames=8), _mcase("u3", 1, 10, frames=16), _mcase("u3", 3, 10, frames=4),
    _mcase("u1tab", 10, 10, frames=16), _mcase("u1", 10, 10, frames=16),
    # and as selected: padded totals either side of 1024 and 2048 frames, the benchmarked 8000, 16-frame grids with an un-remapped tail
    _mcase("t1024", 10, 10), _mcase("t1056", 10, 10), _mcase("t2048", 10, 10), _mcase("t2080", 10, 10),
    _mcase("u25x300", 10, 10), _mcase("u48", 10, 10), _mcase("u3", 10, 10),
    _mcase("u1", 10, 10), _mcase("u1n1", 10, 10), _mcase("u1tab", 1, 10),
    _mcase("u25mixed", 10, 10, frames=16, kind="lognormal"),
    # three-pass kernels: more than 10 kept samples, ranks other than 10, and DVAE_MSTEP=3pass
    _mcase("u3", 11, 10), _mcase("u25mixed", 30, 10), _mcase("u1tab", 30, 10), _mcase("u1n17", 30, 10),
    _mcase("u25mixed", 10, 4), _mcase("u3", 3, 16), _mcase("u1", 10, 16),
    _mcase("u25mixed", 10, 10, mstep="3pass"), _mcase("u1tab", 1, 10, mstep="3pass"),
]


@pytest.mark.parametrize("layout_name,R,K,frames,mstep,kind", MSTEP_CASES)
def test_batched_m_step_matches_float64_oracle(layout_name, R, K, frames, mstep, kind, monkeypatch):
    if frames is None:
        monkeypatch.delenv("DVAE_MSTEP_FRAMES", raising=False)
    else:
        monkeypatch.setenv("DVAE_MSTEP_FRAMES", str(frames))
    if mstep is None:
        monkeypatch.delenv("DVAE_MSTEP", raising=False)
    else:
        monkeypatch.setenv("DVAE_MSTEP", mstep)
    tables = layout_name not in ("u1", "u1n1", "u1n17")
    seed = sum(map(ord, layout_name)) + 7 * R + K
    inp = mstep_inputs(LAYOUTS[layout_name], R, K, seed, kind, tables)
    check_m_step(inp, *run_m_step(inp, tables))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the fused EM iteration (dvae_mcem_em_iteration / _lazy), one iteration at a time, vs the oracle

EM_COUNTS = [300, 17, 641, 1, 333, 160, 500, 64]                  # 2144 padded frames, the W update's loop, half-tiles of padding
EM_MODELS = {
    # name: (model, y_dim, McemBatch flags)
    "M1": ("M1", 0, dict(label_in_encoder=False, label_in_decoder=False)),
    "M2_y1": ("M2", 1, dict()),
    "M2_y513": ("M2", 513, dict()),                               # 513-row labels (528 padded rows in the chain's label image)
    "M2_info": ("M2_info", 1, dict(label_in_encoder=False)),
}


def em_setup(name, precision, seed=31):
    model, y_dim, flags = EM_MODELS[name]
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, seed)
    m = build_model(model, dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.cuda().eval()
    vae = m.enc_dec_clf if model == "M2_info" else m
    prefix = "enc_dec_clf.decoder." if model == "M2_info" else "decoder."
    rng = np.random.default_rng(seed)
    X = [mixture_stft(c, seed * 100 + u) for u, c in enumerate(EM_COUNTS)]
    Y = [(rng.random((y_dim, c)) > 0.5).astype(np.float32) for c in EM_COUNTS] if y_dim else None
    # the reference's settings: 10 kept samples after 30 of burn-in (MCEM_M1: 30 after 30, reference_m1_counts), rank 10
    mb = mcem_dev.McemBatch(vae, niter=2, nsamples_E_step=10, burnin_E_step=30, precision=precision, **flags)
    torch.manual_seed(seed)
    mb.init_parameters(X, Y)
    return mb, params, prefix


def subset_frames(mb, count=288):
    """Live frames spread over every utterance (first and last of each included): the chain is per frame, so the oracle on these columns is exact."""
    live = np.concatenate([np.arange(s, s + c) for s, c in zip(mb.starts, mb.counts)])
    pick = set(live[np.linspace(0, len(live) - 1, count).astype(int)].tolist())
    for s, c in zip(mb.starts, mb.counts):
        pick.update((s, s + c - 1))
    return np.array(sorted(pick))


def np_(a):
    return None if a is None else a.detach().cpu().numpy().copy()


# MCEM_M1 keeps 30 samples: the three-pass M-step, which has no lazy form (McemBatch.run takes the eager iteration there)
# chain None: the weight-stationary chain as selected; "stream": DVAE_MCEM_CHAIN=stream -- mcem_mh_kernel, then last_sample_kernel with Zlast
# aliasing Z0 (check (a) below)
EM_CASES = [pytest.param(name, precision, mode, chain, id=f"{name}-{precision}-{mode}" + (f"-{chain}" if chain else ""))
            for chain in (None, "stream") for name in EM_MODELS for precision in ("fp32", "bf16x3") for mode in ("eager", "lazy")
            if not (name == "M1" and mode == "lazy") and not (chain == "stream" and name == "M2_info")]


@pytest.mark.parametrize("name,precision,mode,chain", EM_CASES)
def test_em_iteration_matches_oracle(name, precision, mode, chain, monkeypatch):
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    if chain is None:
        monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
    else:
        monkeypatch.setenv("DVAE_MCEM_CHAIN", chain)
    mb, params, prefix = em_setup(name, precision)
    lazy = mode == "lazy"
    U, ntot, R, nit = len(mb.counts), mb.ntot, mb.n_e, mb.n_e + mb.b_e
    assert ntot >= 2048 and mb.K == 10
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    cost = torch.full((mb.niter, U), float("nan"), dtype=torch.float32, device="cuda")
    X2 = np_(mb.X2)
    y = np_(mb.y)
    sub = subset_frames(mb)
    live = np.zeros(ntot, bool)
    for s, c in zip(mb.starts, mb.counts):
        live[s:s + c] = True
    cost_o = np.zeros((mb.niter, U))
    for it in range(mb.niter):
        noise = torch.randn(nit, 16, ntot, device="cuda", generator=gen)
        logu = torch.log(torch.rand(nit, ntot, device="cuda", generator=gen))
        pre = {k: getattr(mb, k).clone() for k in ("Z", "g", "Vb", "W", "H")}
        cptr = (cost[it - 1].data_ptr() if it else None) if lazy else cost[it].data_ptr()
        mb._iteration(noise.data_ptr(), logu.data_ptr(), cptr, lazy)
        Zs_d, Vs_d, _ = mb._loop_buffers()
        Zs, Vs = np_(Zs_d), np_(Vs_d)
        # the same chain again from the same state with its trace: same kernels, same bits, plus the log ratios and decisions
        Zs_t, Vs_t, accp, accd = mb._pack.sample(pre["Z"], mb.y, pre["g"], pre["Vb"], mb.X2, noise, logu, mb.b_e, var_rw=float(mb.var_RW), trace=True)
        np.testing.assert_array_equal(np_(Zs_t), Zs)
        np.testing.assert_array_equal(np_(Vs_t), Vs)
        accp, accd = np_(accp), np_(accd).astype(bool)
        # (a) Z is the last kept sample, bit for bit (every column, padding included)
        np.testing.assert_array_equal(np_(mb.Z), Zs[:, -1, :].T)
        # (b) the M-step on the device's own variances, from the device's own state before the iteration
        inp = dict(starts=mb.starts, counts=mb.counts, live=live, X2=X2, Vs=Vs, W=np_(pre["W"]), H=np_(pre["H"]), g=np_(pre["g"]), Vb=np_(pre["Vb"]))
        cost_o[it] = check_m_step(inp, np_(mb.W), np_(mb.H), np_(mb.g), np_(mb.Vb), None, err=f"iteration {it}")
        # (c) the kept samples' variances are the decoder's
        ys = None if y is None else y[:, sub]
        Vs_o = mo.compute_vs(params, prefix, Zs[sub], ys)
        np.testing.assert_allclose(Vs[:, :, sub], Vs_o, rtol=1e-4, atol=1e-9)
        # (d) the chain: log acceptance ratios while the device and the oracle are in the same state, >= 97 % of the frames agree throughout
        Zs_o, tp, ta = mo.sample_posterior(params, prefix, np_(pre["Z"])[:, sub], ys, np_(pre["g"])[sub], np_(pre["Vb"])[:, sub], X2[:, sub],
                                           np_(noise)[:, :, sub], np_(logu)[:, sub], mb.b_e, var_rw=mb.var_RW, return_trace=True)
        diff = accd[:, sub] != ta
        first = np.where(diff.any(axis=0), diff.argmax(axis=0), nit)
        for j in range(len(sub)):
            k = min(first[j] + 1, nit)
            np.testing.assert_allclose(accp[:k, sub[j]], tp[:k, j], rtol=2e-4, atol=2e-3)
        same = first == nit
        assert same.mean() >= 0.97, same.mean()
        np.testing.assert_allclose(Zs[sub][same], Zs_o[same], rtol=1e-5, atol=1e-6)
        assert 0.02 < accd[:, sub].mean() < 0.98
    if lazy:
        lib = mb._pack.lib
        native.check(lib.dvae_mcem_cost_flush(R, ntot, mb.K, U, native.ptr(mb.seg_start), native.ptr(mb.seg_count), cost[-1].data_ptr(),
                                              native.ptr(mb._loop_buffers()[2]), native.stream()), "dvae_mcem_cost_flush")
    np.testing.assert_allclose(cost.cpu().numpy(), cost_o, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. lazy (two M-step launches, cost deferred) == three-launch iteration, bit for bit, at batch scale

@pytest.mark.parametrize("frames", ["4", "8", "16"])
def test_lazy_run_equals_three_launch_run_at_batch_scale(frames, monkeypatch):
    monkeypatch.setenv("DVAE_MSTEP_FRAMES", frames)
    monkeypatch.delenv("DVAE_MSTEP", raising=False)
    counts = [int(c) for c in np.random.default_rng(3).integers(20, 400, 28)]
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 23)
    m = build_model("M2", dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.cuda().eval()
    rng = np.random.default_rng(4)
    X = [mixture_stft(c, 700 + u) for u, c in enumerate(counts)]
    Y = [(rng.random((1, c)) > 0.5).astype(np.float32) for c in counts]
    res = {}
    for lazy in ("0", "1"):
        monkeypatch.setenv("DVAE_MCEM_LAZY", lazy)
        mb = mcem_dev.McemBatch(m, niter=4, nsamples_E_step=3, burnin_E_step=4, nsamples_WF=4, burnin_WF=3)
        torch.manual_seed(1)
        mb.init_parameters(X, Y)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2)
        draws = [(torch.randn(7, 16, mb.ntot, device="cuda", generator=gen), torch.log(torch.rand(7, mb.ntot, device="cuda", generator=gen)))
                 for _ in range(mb.niter + 1)]
        cost = mb.run(draws)
        res[lazy] = [cost] + [np_(a) for a in (mb.W, mb.H, mb.g, mb.Z, mb.WFs, mb.WFn)]
    assert np.isfinite(res["1"][0]).all()
    for nm, a, b in zip(("cost", "W", "H", "g", "Z", "WFs", "WFn"), res["0"], res["1"]):
        np.testing.assert_array_equal(a, b, err_msg=nm)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. Wiener gains at the final chain's 25 kept samples over a batch-sized frame axis

def test_wiener_gains_at_batch_scale():
    R, n = 25, 8032
    rng = np.random.default_rng(25)
    X2 = power(mixture_stft(n, 9))
    Vs = (X2 * np.exp(0.7 * rng.standard_normal((R, F, n)) - 0.7)).astype(np.float32)
    g = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    Vb = (np.maximum(rng.random((F, 10)), 1e-6) @ np.maximum(rng.random((10, n)), 1e-6)).astype(np.float32)
    WFs, WFn = mcem_dev.wiener(t(Vs), t(g), t(Vb))
    WFs, WFn = WFs.cpu().numpy(), WFn.cpu().numpy()
    for c0 in range(0, n, 1024):                                # the oracle in float64, 1024 frames at a time
        sl = slice(c0, min(n, c0 + 1024))
        WFs_o, WFn_o = mo.wiener(Vs[:, :, sl].astype(np.float64), g[sl].astype(np.float64), Vb[:, sl].astype(np.float64))
        np.testing.assert_allclose(WFs[:, sl], WFs_o, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(WFn[:, sl], WFn_o, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(WFs + WFn, 1.0, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. an utterance without frames has no columns to lay out: refused, not a NaN W

def test_zero_frame_utterance_is_refused():
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    m = build_model("M2", dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in gu.make_params("M2", dims, 3).items()})
    m.cuda().eval()
    X = [mixture_stft(40, 1), np.zeros((F, 0), np.complex64), mixture_stft(9, 2)]
    Y = [np.ones((1, x.shape[1]), np.float32) for x in X]
    mb = mcem_dev.McemBatch(m, niter=1)
    with pytest.raises(ValueError, match="utterance 1"):
        mb.init_parameters(X, Y)

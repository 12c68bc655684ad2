"""The streaming Metropolis-Hastings chain of csrc/mcem.hip (mcem_mh_kernel<P, YP, RES> + last_sample_kernel) where the library
selects it BY ITSELF: calls whose (513, N) matrices or whose noise array reach 2 GiB, which the weight-stationary chain refuses.
No environment variable is set for the large calls; inputs are built on the device from a seeded generator and only the compared
columns come back.  Frames are independent given g and Vb, so the float64 oracle on a subset of the columns is exact for them.

Which test reaches which instantiation by an oracle comparison (tests elsewhere select the kernel with DVAE_MCEM_CHAIN=stream,
which the library reads on every call):

  mcem_mh_kernel<PolF32Lean, 0, 0>    test_gpu_mcem.py::test_sample_posterior_matches_oracle[M1-0-45-fp32-stream],
                                      test_gpu_mcem_batch.py::test_em_iteration_matches_oracle[M1-fp32-eager-stream]
  mcem_mh_kernel<PolF32Lean, 16, 0>   test_large_frame_count_takes_the_streaming_chain[fp32] (here, automatic dispatch);
                                      test_gpu_mcem.py::test_sample_posterior_matches_oracle[M2-{1,2,7,15,16}-*-fp32-stream] and the soft cases,
                                      ::test_chain_on_tiny_and_ragged_frame_counts[*-fp32-stream]
  mcem_mh_kernel<PolF32Lean, 528, 0>  test_gpu_mcem.py::test_sample_posterior_matches_oracle[M2-513-33-fp32-stream], [M2-513-45-soft-fp32-stream]
  mcem_mh_kernel<PolX3M<0>, 0, 0>     test_gpu_mcem.py::test_sample_posterior_matches_oracle[M1-0-45-bf16x3-stream]
  mcem_mh_kernel<PolX3M<16>, 16, 0>   test_large_frame_count_takes_the_streaming_chain[bf16x3], test_long_chain_takes_the_streaming_chain,
                                      test_dispatch_boundary_of_the_frame_count (here); the bf16x3-stream cases of test_gpu_mcem.py
  mcem_mh_kernel<PolX3M<528>, 528, 0> test_gpu_mcem.py::test_sample_posterior_matches_oracle[M2-513-33-bf16x3-stream], [M2-513-45-soft-bf16x3-stream]
  mcem_mh_kernel<PolBF16, 16, 1>      test_gpu_mcem.py::test_bf16_chain_is_statistically_close[stream] (bf16 noise bounds: the policy rounds to 8 bits)
  mcem_mh_kernel<PolBF16, 0, 1>, <PolBF16, 528, 1>
                                      test_bf16_streaming_chain_without_and_with_513_label_rows (here, the same bf16 noise bounds)
  last_sample_kernel                  test_gpu_mcem_batch.py::test_em_iteration_matches_oracle[*-stream], check (a): Z is the last kept sample bit for bit
                                      with Zlast aliasing Z0
"""
import importlib
import time

import numpy as np
import pytest
import torch

import golden_util as gu
from impl_modules import build_model
from oracle import mcem_oracle as mo

pytestmark = pytest.mark.gpu
mcem_dev = importlib.import_module("disentangled-vae_amd.mcem")

F = 513
TWO_GIB = 1 << 31
GUARD = 1 << 16


def make_pack(model, y_dim, precision, seed=5):
    dims = dict(x_dim=F, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, seed)
    m = build_model(model, dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.cuda()
    return params, mcem_dev.DecoderPack(m.decoder, y_dim, precision)


def device_inputs(N, y_dim, seed):
    """The chain's per-frame inputs on the device (the distributions of test_gpu_mcem.setup); nothing of size N touches the host."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    ru = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    X2 = rn(F, N)
    X2.square_().mul_(torch.exp(rn(F, 1) - 1)).add_(1e-4)
    W = ru(F, 10).clamp_min_(1e-6)
    H = ru(10, N).clamp_min_(1e-6)
    Vb = torch.mm(W, H)
    del H
    y = (ru(y_dim, N) > 0.5).float() if y_dim else None
    Z = rn(16, N)
    g = torch.exp(0.2 * rn(N))
    return dict(N=N, X2=X2, Vb=Vb, y=y, Z=Z, g=g, gen=gen)


def tile_columns(N, tiles):
    """Columns of the given 32-frame tiles in ascending order; the ragged last tile may only come last, so that in a launch on these
    columns alone every frame sits in the lane it had in the large launch."""
    tiles = sorted(set(tiles))
    cols = np.concatenate([np.arange(32 * k, min(32 * k + 32, N)) for k in tiles])
    assert all(32 * k + 32 <= N for k in tiles[:-1])
    return cols


def take(a, cols_dev, dim):
    return None if a is None else a.index_select(dim, cols_dev).contiguous()


def guarded(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD:GUARD + n].view(dtype).view(*shape)


def guards_intact(raw):
    return bool((raw[:GUARD] == 0xA5).all()) and bool((raw[-GUARD:] == 0xA5).all())


def bar_units(got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if got.size else 0.0


def check_chain(what, params, sub, Zs, accp, accd, burnin, Vs=None):
    """The chain bars of test_gpu_mcem.py against the float64 oracle on the columns `sub` (a dict of host arrays): log ratios within rtol 2e-4 /
    atol 2e-3 while device and oracle are in the same state, >= 97 % of the frames agreeing over the whole chain, kept samples within rtol 1e-5 /
    atol 1e-6, Vs within rtol 1e-4 of the decoder."""
    nit = sub["noise"].shape[0]
    Zs_o, tp, ta = mo.sample_posterior(params, "decoder.", sub["Z"], sub["y"], sub["g"], sub["Vb"], sub["X2"], sub["noise"], sub["logu"], burnin,
                                       dtype=np.float64, return_trace=True)
    diff = accd.astype(bool) != ta
    first = np.where(diff.any(axis=0), diff.argmax(axis=0), nit)
    in_state = np.arange(nit)[:, None] <= first[None, :]
    same = first == nit
    msg = (f"{what}: worst error in units of the bar: log ratio {bar_units(accp[in_state], tp[in_state], 2e-4, 2e-3):.3f}, "
           f"kept samples {bar_units(Zs[same], Zs_o[same], 1e-5, 1e-6):.3f}")
    if Vs is not None:
        Vs_o = mo.compute_vs(params, "decoder.", Zs, sub["y"], dtype=np.float64)
        msg += f", Vs {bar_units(Vs, Vs_o, 1e-4, 1e-9):.3f} (row 512: {bar_units(Vs[:, 512], Vs_o[:, 512], 1e-4, 1e-9):.3f})"
    print(msg + f"; same decisions {same.mean():.3f}, acceptance {accd.mean():.3f}")
    np.testing.assert_allclose(accp[in_state], tp[in_state], rtol=2e-4, atol=2e-3)
    assert same.mean() >= 0.97, same.mean()
    np.testing.assert_allclose(Zs[same], Zs_o[same], rtol=1e-5, atol=1e-6)
    assert 0.02 < accd.mean() < 0.98
    if Vs is not None:
        np.testing.assert_allclose(Vs[:, 512], Vs_o[:, 512], rtol=1e-4, atol=1e-9)          # the row whose offsets lie wholly past 2^31 bytes
        np.testing.assert_allclose(Vs, Vs_o, rtol=1e-4, atol=1e-9)


def host(sub_dev):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in sub_dev.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# 1. (513, N) matrices past 2 GiB: N >= 1 046 532

N_BIG = (1 << 20) + 37


@pytest.fixture(scope="module")
def big():
    """Inputs of the N = 2^20 + 37 calls, built once (about 4.5 GB on the device) and left unchanged by the tests."""
    inp = device_inputs(N_BIG, 1, 1234)
    nit = 2
    inp["noise"] = torch.randn(nit, 16, N_BIG, device="cuda", generator=inp["gen"])
    inp["logu"] = torch.log(torch.rand(nit, N_BIG, device="cuda", generator=inp["gen"]))
    yield inp
    inp.clear()
    torch.cuda.empty_cache()


def big_tiles(N):
    """The first tile, the ragged last one and its whole neighbour, the tile in which row 511's byte offset crosses 2^31 (row 512 lies wholly
    past it), and tiles in between."""
    last = (N - 1) // 32
    n_cross = (TWO_GIB - 511 * N * 4) // 4
    assert 0 < n_cross < N and 512 * N * 4 >= TWO_GIB and N % 32 != 0
    return [0, 1000, 8192, 12345, 16385, 20000, 24577, 30000, n_cross // 32, last - 1, last]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_large_frame_count_takes_the_streaming_chain(big, precision, monkeypatch):
    """N = 2^20 + 37 frames, M2 with one label row: decode at R = 1 and a 2-step chain with its trace, on 11 tiles (325 frames) against the float64
    oracle; guard bands around every output; and the same tiles alone under DVAE_MCEM_CHAIN=stream give the same bits, i.e. the large call ran
    the streaming kernel and its 64-bit indexing moved nothing."""
    monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    import ctypes
    Nn = importlib.import_module("disentangled-vae_amd.native")
    N, nit, burnin, R = N_BIG, 2, 1, 1
    assert F * N * 4 >= TWO_GIB
    params, pack = make_pack("M2", 1, precision)
    cols = tile_columns(N, big_tiles(N))
    cd = torch.from_numpy(cols).cuda()
    raws, outs = zip(*(guarded(s, d) for s, d in (((N, R, 16), torch.float32), ((R, F, N), torch.float32), ((nit, N), torch.float32), ((nit, N), torch.uint8))))
    Zs, Vs, accp, accd = outs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Nn.check(pack.lib.dvae_mcem_sample(ctypes.byref(pack.plan), Nn.ptr(pack.weights), Nn.ptr(big["Z"]), Nn.ptr(big["y"]), Nn.ptr(big["g"]), Nn.ptr(big["Vb"]),
                                       Nn.ptr(big["X2"]), Nn.ptr(big["noise"]), Nn.ptr(big["logu"]), nit, burnin, 0.01, N, Nn.ptr(Zs), Nn.ptr(Vs), Nn.ptr(accp),
                                       Nn.ptr(accd), Nn.stream()), "dvae_mcem_sample")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    Vs2 = pack.decode(Zs, big["y"])
    torch.cuda.synchronize()
    print(f"N = {N} {precision}: chain of {nit} steps + Vs {t1 - t0:.3f} s, decode {time.perf_counter() - t1:.3f} s")
    for nm, raw in zip(("Zs", "Vs", "accp", "accd"), raws):
        assert guards_intact(raw), f"{nm}: guard band overwritten"
    assert torch.equal(Vs2, Vs)                                  # decode alone == the launch's Vs, all 513 x N of it
    del Vs2
    assert bool(torch.isfinite(Vs[0, 512]).all()) and bool((Vs[0, 512] > 0).all())
    sub_dev = dict(X2=take(big["X2"], cd, 1), Vb=take(big["Vb"], cd, 1), y=take(big["y"], cd, 1), Z=take(big["Z"], cd, 1), g=take(big["g"], cd, 0),
                   noise=take(big["noise"], cd, 2), logu=take(big["logu"], cd, 1))
    got = [a.cpu().numpy() for a in (take(Zs, cd, 0), take(Vs, cd, 2), take(accp, cd, 1), take(accd, cd, 1))]
    check_chain(f"N = {N} {precision}", params, host(sub_dev), got[0], got[2], got[3], burnin, Vs=got[1])
    # the same tiles alone on the streaming kernel: the same bits
    monkeypatch.setenv("DVAE_MCEM_CHAIN", "stream")
    alone = pack.sample(sub_dev["Z"], sub_dev["y"], sub_dev["g"], sub_dev["Vb"], sub_dev["X2"], sub_dev["noise"], sub_dev["logu"], burnin, trace=True)
    for nm, a, b in zip(("Zs", "Vs", "accp", "accd"), got, alone):
        np.testing.assert_array_equal(a, b.cpu().numpy(), err_msg=nm)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. a noise array past 2 GiB: nit * 16 * N * 4 >= 2^31

def test_long_chain_takes_the_streaming_chain(monkeypatch):
    """N = 2^18 + 5 frames, 129 steps (128 of burn-in), bf16x3, no Vs, no trace: the noise array is just over 2 GiB (the last burn-in step's
    feature 15 crosses 2^31 bytes, the kept step lies wholly past it).  The large call returns no decisions, so: its kept sample equals, bit
    for bit, that of the same tiles alone under DVAE_MCEM_CHAIN=stream with the trace on, and THAT launch's log ratios, decisions (the last
    step's among them) and kept sample meet the chain bars against the float64 oracle.
    Measured on MI355X: the large call takes 0.04 s (8193 tiles, 130 decoder passes each)."""
    monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    N, nit, burnin = (1 << 18) + 5, 129, 128
    assert nit * 16 * N * 4 >= TWO_GIB and F * N * 4 < TWO_GIB
    params, pack = make_pack("M2", 1, "bf16x3")
    inp = device_inputs(N, 1, 4321)
    noise = torch.randn(nit, 16, N, device="cuda", generator=inp["gen"])
    logu = torch.log(torch.rand(nit, N, device="cuda", generator=inp["gen"]))
    last = (N - 1) // 32
    e_cross = TWO_GIB // 4 - (127 * 16 + 15) * N                 # frame at which (step 127, feature 15) crosses 2^31 bytes
    assert 0 < e_cross < N
    cols = tile_columns(N, [0, 1, 1000, 2731, 4096, 6000, e_cross // 32, last - 1, last])
    cd = torch.from_numpy(cols).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Zs, Vs = pack.sample(inp["Z"], inp["y"], inp["g"], inp["Vb"], inp["X2"], noise, logu, burnin, want_vs=False)
    torch.cuda.synchronize()
    print(f"N = {N}, {nit} steps, bf16x3: {time.perf_counter() - t0:.3f} s")
    assert Vs is None and bool(torch.isfinite(Zs).all())
    sub_dev = dict(X2=take(inp["X2"], cd, 1), Vb=take(inp["Vb"], cd, 1), y=take(inp["y"], cd, 1), Z=take(inp["Z"], cd, 1), g=take(inp["g"], cd, 0),
                   noise=take(noise, cd, 2), logu=take(logu, cd, 1))
    Zs_sub = take(Zs, cd, 0).cpu().numpy()
    monkeypatch.setenv("DVAE_MCEM_CHAIN", "stream")
    Zs_a, _, accp, accd = pack.sample(sub_dev["Z"], sub_dev["y"], sub_dev["g"], sub_dev["Vb"], sub_dev["X2"], sub_dev["noise"], sub_dev["logu"], burnin,
                                      want_vs=False, trace=True)
    np.testing.assert_array_equal(Zs_sub, Zs_a.cpu().numpy())
    check_chain(f"N = {N}, {nit} steps", params, host(sub_dev), Zs_sub, accp.cpu().numpy(), accd.cpu().numpy(), burnin)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the boundary: 513 * N * 4 < 2^31 takes the weight-stationary chain, >= 2^31 the streaming one

@pytest.mark.parametrize("N,chain", [(1046531, "resident"), (1046532, "stream")])
def test_dispatch_boundary_of_the_frame_count(big, N, chain, monkeypatch):
    """Seen from the results (bf16x3, where the two chains differ in their bits): the last N the weight-stationary chain addresses equals
    a DVAE_MCEM_TILE=32 run of the same tiles, the first N past it a DVAE_MCEM_CHAIN=stream run of them."""
    monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    assert F * 1046531 * 4 < TWO_GIB <= F * 1046532 * 4
    params, pack = make_pack("M2", 1, "bf16x3")
    burnin = 1
    inp = {k: (big[k][..., :N].contiguous()) for k in ("X2", "Vb", "y", "Z", "g", "noise", "logu")}
    last = (N - 1) // 32
    cols = tile_columns(N, [0, 9000, 17000, 25000, last - 1, last])
    cd = torch.from_numpy(cols).cuda()
    Zs, Vs, accp, accd = pack.sample(inp["Z"], inp["y"], inp["g"], inp["Vb"], inp["X2"], inp["noise"], inp["logu"], burnin, trace=True)
    got = [a.cpu().numpy() for a in (take(Zs, cd, 0), take(Vs, cd, 2), take(accp, cd, 1), take(accd, cd, 1))]
    del Zs, Vs, accp, accd
    sub = dict(X2=take(inp["X2"], cd, 1), Vb=take(inp["Vb"], cd, 1), y=take(inp["y"], cd, 1), Z=take(inp["Z"], cd, 1), g=take(inp["g"], cd, 0),
               noise=take(inp["noise"], cd, 2), logu=take(inp["logu"], cd, 1))
    del inp
    alone = {}
    for which, var, val in (("resident", "DVAE_MCEM_TILE", "32"), ("stream", "DVAE_MCEM_CHAIN", "stream")):
        monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
        monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
        monkeypatch.setenv(var, val)
        alone[which] = [a.cpu().numpy() for a in pack.sample(sub["Z"], sub["y"], sub["g"], sub["Vb"], sub["X2"], sub["noise"], sub["logu"], burnin, trace=True)]
    # the check can tell the two chains apart on these columns
    assert not np.array_equal(alone["resident"][2], alone["stream"][2])
    for nm, a, b in zip(("Zs", "Vs", "accp", "accd"), got, alone[chain]):
        np.testing.assert_array_equal(a, b, err_msg=f"{nm}: N = {N} did not take the {chain} chain")
    check_chain(f"N = {N} ({chain})", params, host(sub), got[0], got[2], got[3], burnin, Vs=got[1])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the bf16 policy of the streaming chain (decoder layers 1-2 in registers) without labels and with 513 label rows

@pytest.mark.parametrize("model,y_dim", [("M1", 0), ("M2", 513)])
def test_bf16_streaming_chain_without_and_with_513_label_rows(model, y_dim, monkeypatch):
    """The bounds of test_gpu_mcem.py::test_bf16_chain_is_statistically_close (bf16 operands round to 8 bits: first-step log ratios within bf16
    noise of the oracle, the same acceptance rate to a few percent), on the two label widths that test does not run."""
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    monkeypatch.setenv("DVAE_MCEM_CHAIN", "stream")
    N, nit, burnin = 256, 20, 10
    params, pack = make_pack(model, y_dim, "bf16", seed=9)
    inp = device_inputs(N, y_dim, 99)
    noise = torch.randn(nit, 16, N, device="cuda", generator=inp["gen"])
    logu = torch.log(torch.rand(nit, N, device="cuda", generator=inp["gen"]))
    Zs, Vs, accp, accd = pack.sample(inp["Z"], inp["y"], inp["g"], inp["Vb"], inp["X2"], noise, logu, burnin, trace=True)
    h = host(dict(X2=inp["X2"], Vb=inp["Vb"], y=inp["y"], Z=inp["Z"], g=inp["g"], noise=noise, logu=logu))
    _, tp, ta = mo.sample_posterior(params, "decoder.", h["Z"], h["y"], h["g"], h["Vb"], h["X2"], h["noise"], h["logu"], burnin, dtype=np.float64,
                                    return_trace=True)
    accp, accd = accp.cpu().numpy(), accd.cpu().numpy().astype(bool)
    err = np.abs(accp[0] - tp[0])
    print(f"{model} y_dim {y_dim} bf16 stream: first-step log ratio error median {np.median(err):.4f}, max {err.max():.4f}; acceptance {accd.mean():.3f} / {ta.mean():.3f}")
    assert np.median(err) < 0.15 and err.max() < 2.0, (np.median(err), err.max())
    assert abs(accd.mean() - ta.mean()) < 0.05
    assert torch.isfinite(Vs).all()

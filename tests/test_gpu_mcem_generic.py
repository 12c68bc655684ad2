"""The generic Metropolis-Hastings chain (csrc/mcem_generic.hip, plans of dvae_mcem_plan_dims) against the float64 oracle, from the
kernel up to the drop-in classes: every geometry case of mcem_generic_cases.py and a single frame of each, the decode job, the
reference's decoder on both kernels, composition (a frame alone = the same frame in a larger launch, bit for bit), guard bands, one
EM iteration of a McemBatch in both forms, MCEM_M2.run / McemBatch.run on a decoder the hand-tuned kernels do not cover, refusals.
Bars: test_gpu_mcem_stream.check_chain (log ratios rtol 2e-4 / atol 2e-3 in the same state, >= 97 % of the frames with the same
decisions, kept samples rtol 1e-5 / atol 1e-6, Vs rtol 1e-4 / atol 1e-9, acceptance inside (0.02, 0.98))."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import golden_util as gu
import mcem_generic_cases as gc
from impl_modules import build_model
from oracle import mcem_oracle as mo
from test_gpu_mcem_batch import check_m_step, mixture_stft, np_
from test_gpu_mcem_stream import check_chain, guarded, guards_intact

pytestmark = pytest.mark.gpu
mcem_dev = importlib.import_module("disentangled-vae_amd.mcem")
native = importlib.import_module("disentangled-vae_amd.native")

F = 513
EM_DIMS = ("M2", 1, 32, (256, 64))                                # the model of the EM-iteration and surface tests


def t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def make_model(model, y_dim, z_dim, h_dim, seed=gc.SEED):
    dims = gc.dims_of(y_dim, z_dim, h_dim)
    params = gu.make_params(model, dims, seed)
    m = build_model(model, dims)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.cuda().eval()
    for p in m.parameters():
        p.requires_grad = False
    return params, m


_packs = {}


def pack_of(model, y_dim, z_dim, h_dim, generic=False):
    key = (model, y_dim, z_dim, tuple(h_dim), generic)
    if key not in _packs:
        _, m = make_model(model, y_dim, z_dim, h_dim)
        _packs[key] = mcem_dev.DecoderPack(m.decoder, y_dim, "fp32", generic=generic)
    return _packs[key]


def run_chain(pack, inp, trace=True):
    out = pack.sample(t(inp["Z"]), t(inp["y"]), t(inp["g"]), t(inp["Vb"]), t(inp["X2"]), t(inp["noise"]), t(inp["logu"]), gc.BURNIN, trace=trace)
    return [a.cpu().numpy() for a in out]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. every geometry case, and one frame of it alone

@pytest.mark.parametrize("single", [False, True], ids=["all", "N1"])
@pytest.mark.parametrize("model,y_dim,z_dim,h_dim,N", gc.CASES, ids=gc.IDS)
def test_chain_matches_float64_oracle(model, y_dim, z_dim, h_dim, N, single):
    inp = gc.chain_inputs(model, y_dim, z_dim, h_dim, N)
    if single:
        inp = gc.columns(inp, [N // 2])
    pack = pack_of(model, y_dim, z_dim, h_dim, generic=True)
    assert pack.plan.h2_dim == h_dim[0] and pack.plan.h_dim == h_dim[1] and pack.plan.z_dim == z_dim and pack.z_dim == z_dim
    Zs, Vs, accp, accd = run_chain(pack, inp)
    assert Zs.shape == (inp["Z"].shape[1], gc.NIT - gc.BURNIN, z_dim)
    check_chain(f"{model} y{y_dim} z{z_dim} h{h_dim} N{inp['Z'].shape[1]}", inp["params"], inp, Zs, accp, accd, gc.BURNIN, Vs=Vs)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the decode job

@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("model,y_dim,z_dim,h_dim,N", gc.CASES, ids=gc.IDS)
def test_decode_matches_float64_decoder(model, y_dim, z_dim, h_dim, N, R):
    inp = gc.chain_inputs(model, y_dim, z_dim, h_dim, N)
    Zs = np.random.default_rng(R).standard_normal((N, R, z_dim)).astype(np.float32)
    Vs = pack_of(model, y_dim, z_dim, h_dim, generic=True).decode(t(Zs), t(inp["y"])).cpu().numpy()
    assert Vs.shape == (R, F, N)
    np.testing.assert_allclose(Vs, mo.compute_vs(inp["params"], "decoder.", Zs, inp["y"], dtype=np.float64), rtol=1e-4, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the reference's decoder on both kernels, the same draws

def test_reference_decoder_on_both_kernels(monkeypatch):
    monkeypatch.delenv("DVAE_MCEM_CHAIN", raising=False)
    monkeypatch.delenv("DVAE_MCEM_TILE", raising=False)
    case = gc.CASES[-1]
    assert case[2:4] == (16, (128, 128))
    inp = gc.chain_inputs(*case)
    res = {}
    for generic in (True, False):
        pack = pack_of(*case[:4], generic=generic)
        assert (pack.plan.h2_dim != 0) == generic and pack.generic == generic
        res[generic] = run_chain(pack, inp)
        check_chain(f"reference decoder, generic={generic}", inp["params"], inp, res[generic][0], res[generic][2], res[generic][3], gc.BURNIN, Vs=res[generic][1])
    same = (res[True][3] == res[False][3]).all(axis=0)
    assert same.mean() >= 0.97, same.mean()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. composition

def test_a_frame_alone_equals_the_frame_in_a_launch_bit_for_bit():
    case = gc.CASES[5]
    assert case[4] == 70
    inp = gc.chain_inputs(*case)
    pack = pack_of(*case[:4], generic=True)
    full = run_chain(pack, inp)
    again = run_chain(pack, inp)
    for nm, a, b in zip(("Zs", "Vs", "accp", "accd"), full, again):
        np.testing.assert_array_equal(a, b, err_msg=f"{nm}: two runs of one launch")
    for j in (0, 15, 16, 37, 63, 64, 69):                           # first / last columns of whole tiles, the ragged last tile
        Zs, Vs, accp, accd = run_chain(pack, gc.columns(inp, [j]))
        np.testing.assert_array_equal(Zs[0], full[0][j], err_msg=f"Zs, column {j}")
        np.testing.assert_array_equal(Vs[:, :, 0], full[1][:, :, j], err_msg=f"Vs, column {j}")
        np.testing.assert_array_equal(accp[:, 0], full[2][:, j], err_msg=f"log ratios, column {j}")
        np.testing.assert_array_equal(accd[:, 0], full[3][:, j], err_msg=f"decisions, column {j}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. guard bands

@pytest.mark.parametrize("N", [1, 17])
def test_outputs_stay_inside_their_buffers(N):
    case = gc.CASES[5]
    model, y_dim, z_dim, h_dim, n_all = case
    inp = gc.columns(gc.chain_inputs(*case), np.arange(N) + 20)
    pack = pack_of(*case[:4], generic=True)
    R = gc.NIT - gc.BURNIN
    raws, outs = zip(*(guarded(s, d) for s, d in (((N, R, z_dim), torch.float32), ((R, F, N), torch.float32), ((gc.NIT, N), torch.float32),
                                                  ((gc.NIT, N), torch.uint8))))
    Zs, Vs, accp, accd = outs
    d = {k: t(inp[k]) for k in ("Z", "y", "g", "Vb", "X2", "noise", "logu")}
    native.check(pack.lib.dvae_mcem_sample(ctypes.byref(pack.plan), native.ptr(pack.weights), native.ptr(d["Z"]), native.ptr(d["y"]), native.ptr(d["g"]),
                                           native.ptr(d["Vb"]), native.ptr(d["X2"]), native.ptr(d["noise"]), native.ptr(d["logu"]), gc.NIT, gc.BURNIN, 0.01, N,
                                           native.ptr(Zs), native.ptr(Vs), native.ptr(accp), native.ptr(accd), native.stream()), "dvae_mcem_sample")
    Vs2_raw, Vs2 = guarded((R, F, N), torch.float32)
    native.check(pack.lib.dvae_mcem_decode(ctypes.byref(pack.plan), native.ptr(pack.weights), native.ptr(Zs), native.ptr(d["y"]), R, N, native.ptr(Vs2),
                                           native.stream()), "dvae_mcem_decode")
    torch.cuda.synchronize()
    for nm, raw in zip(("Zs", "Vs", "accp", "accd", "decode's Vs"), raws + (Vs2_raw,)):
        assert guards_intact(raw), f"{nm}: guard band overwritten"
    assert torch.equal(Vs, Vs2)
    ref = run_chain(pack, inp)
    for nm, a, b in zip(("Zs", "Vs", "accp", "accd"), (Zs, Vs, accp, accd), ref):
        np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=nm)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. one EM iteration of a batch (dvae_mcem_em_iteration and the lazy form)

EM_COUNTS = [33, 70, 16]


def em_batch(niter=2, seed=31):
    model, y_dim, z_dim, h_dim = EM_DIMS
    params, m = make_model(model, y_dim, z_dim, h_dim, seed)
    rng = np.random.default_rng(seed)
    X = [mixture_stft(c, seed * 100 + u) for u, c in enumerate(EM_COUNTS)]
    Y = [(rng.random((y_dim, c)) > 0.5).astype(np.float32) for c in EM_COUNTS]
    mb = mcem_dev.McemBatch(m, niter=niter, nsamples_E_step=10, burnin_E_step=30)
    torch.manual_seed(seed)
    mb.init_parameters(X, Y)
    return mb, params, m


@pytest.mark.parametrize("mode", ["eager", "lazy"])
def test_em_iteration_matches_oracle(mode, monkeypatch):
    monkeypatch.delenv("DVAE_MSTEP", raising=False)
    monkeypatch.delenv("DVAE_MSTEP_FRAMES", raising=False)
    mb, params, _ = em_batch()
    z_dim = EM_DIMS[2]
    lazy = mode == "lazy"
    U, ntot, R, nit = len(mb.counts), mb.ntot, mb.n_e, mb.n_e + mb.b_e
    assert mb._pack.generic and mb._pack.z_dim == z_dim and mb.Z.shape == (z_dim, ntot) and ntot == 192 and mb.K == 10
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    cost = torch.full((mb.niter, U), float("nan"), dtype=torch.float32, device="cuda")
    X2, y = np_(mb.X2), np_(mb.y)
    live = np.zeros(ntot, bool)
    for s, c in zip(mb.starts, mb.counts):
        live[s:s + c] = True
    sub = np.flatnonzero(live)
    cost_o = np.zeros((mb.niter, U))
    for it in range(mb.niter):
        noise = torch.randn(nit, z_dim, ntot, device="cuda", generator=gen)
        logu = torch.log(torch.rand(nit, ntot, device="cuda", generator=gen))
        pre = {k: getattr(mb, k).clone() for k in ("Z", "g", "Vb", "W", "H")}
        cptr = (cost[it - 1].data_ptr() if it else None) if lazy else cost[it].data_ptr()
        mb._iteration(noise.data_ptr(), logu.data_ptr(), cptr, lazy)
        Zs_d, Vs_d, _ = mb._loop_buffers()
        Zs, Vs = np_(Zs_d), np_(Vs_d)
        assert Zs.shape == (ntot, R, z_dim)
        # the same chain again from the same state with its trace: the same bits, plus log ratios and decisions
        Zs_t, Vs_t, accp, accd = mb._pack.sample(pre["Z"], mb.y, pre["g"], pre["Vb"], mb.X2, noise, logu, mb.b_e, var_rw=float(mb.var_RW), trace=True)
        np.testing.assert_array_equal(np_(Zs_t), Zs)
        np.testing.assert_array_equal(np_(Vs_t), Vs)
        assert np.isfinite(Zs).all() and np.isfinite(Vs).all()                       # padding frames (X2 = Vb = g = 1) included
        # Z is the last kept sample, bit for bit (every column, padding included)
        np.testing.assert_array_equal(np_(mb.Z), Zs[:, -1, :].T)
        # the M-step on the device's own variances: W / H / g / Vb within rtol 1e-4, padding columns untouched
        inp = dict(starts=mb.starts, counts=mb.counts, live=live, X2=X2, Vs=Vs, W=np_(pre["W"]), H=np_(pre["H"]), g=np_(pre["g"]), Vb=np_(pre["Vb"]))
        cost_o[it] = check_m_step(inp, np_(mb.W), np_(mb.H), np_(mb.g), np_(mb.Vb), None, err=f"iteration {it}")
        # the chain and the kept samples' variances on every live frame
        h = dict(Z=np_(pre["Z"])[:, sub], y=y[:, sub], g=np_(pre["g"])[sub], Vb=np_(pre["Vb"])[:, sub], X2=X2[:, sub], noise=np_(noise)[:, :, sub],
                 logu=np_(logu)[:, sub])
        check_chain(f"iteration {it}", params, h, Zs[sub], np_(accp)[:, sub], np_(accd)[:, sub], mb.b_e, Vs=Vs[:, :, sub])
    if lazy:
        native.check(mb._pack.lib.dvae_mcem_cost_flush(R, ntot, mb.K, U, native.ptr(mb.seg_start), native.ptr(mb.seg_count), cost[-1].data_ptr(),
                                                       native.ptr(mb._loop_buffers()[2]), native.stream()), "dvae_mcem_cost_flush")
    np.testing.assert_allclose(cost.cpu().numpy(), cost_o, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the surface: the drop-in class and McemBatch.run on a decoder the hand-tuned kernels do not cover

def test_dropin_run_on_a_generic_decoder_equals_the_stepwise_loop(monkeypatch):
    from packages.models import mcem
    model, y_dim, z_dim, h_dim = EM_DIMS
    _, m = make_model(model, y_dim, z_dim, h_dim, 31)
    assert mcem_dev.chain_kind(m.decoder, y_dim) == "generic"
    rng = np.random.default_rng(8)
    N = 45
    X, S = mixture_stft(N, 3), mixture_stft(N, 4)
    y = torch.from_numpy((rng.random((y_dim, N)) > 0.4).astype(np.float32)).cuda()
    res = {}
    for mode in ("fused", "steps"):
        monkeypatch.setenv("DVAE_MCEM_RUN", mode)
        em = mcem.MCEM_M2(niter=3, nsamples_E_step=3, burnin_E_step=4, nsamples_WF=4, burnin_WF=3)
        em.precision = "fp32"
        torch.manual_seed(7)
        em.init_parameters(X=X, S=S, y=y, vae=m, nmf_rank=10, eps=np.finfo(float).eps, device="cuda")
        cost = em.run()
        assert em._pack is not None and em._pack.generic and em.Z.shape == (z_dim, N)
        res[mode] = (np.asarray(cost, np.float64), em.W.cpu().numpy(), em.H.cpu().numpy(), em.g.cpu().numpy(), em.Z.cpu().numpy(), em.S_hat, em.N_hat)
    assert res["fused"][0].shape == (3,) and np.all(np.isfinite(res["fused"][0]))
    for nm, a, b in zip(("cost", "W", "H", "g", "Z", "S_hat", "N_hat"), res["fused"], res["steps"]):
        np.testing.assert_array_equal(a, b, err_msg=nm)
    assert np.isfinite(res["fused"][5]).all() and res["fused"][5].shape == X.shape


def test_batch_run_on_a_generic_decoder():
    mb, _, _ = em_batch(niter=3)
    mb.n_wf, mb.b_wf = 4, 3
    cost = mb.run()
    assert cost.shape == (3, len(EM_COUNTS)) and np.isfinite(cost).all()
    WFs, WFn = mb.WFs.cpu().numpy(), mb.WFn.cpu().numpy()
    assert WFs.shape == (F, mb.ntot) and np.isfinite(WFs).all() and np.isfinite(WFn).all()
    np.testing.assert_allclose(WFs + WFn, 1.0, rtol=1e-5)
    assert all(s.shape == (F, c) for s, c in zip(mb.S_hat, EM_COUNTS))


# ------------------------------------------------------------------------------------------------------------------------------
# 8. refusals

def test_refusals():
    from packages.models import mcem
    STFT = importlib.import_module("disentangled-vae_amd.stft")
    model, y_dim, z_dim, h_dim = EM_DIMS
    _, m = make_model(model, y_dim, z_dim, h_dim, 31)
    # a precision the generic chain does not have: refused, naming fp32 -- by the pack, by the drop-in class (no silent fallback)
    with pytest.raises(RuntimeError, match="fp32"):
        mcem_dev.DecoderPack(m.decoder, y_dim, "bf16x3")
    _, ref = make_model("M2", 1, 16, (128, 128))
    with pytest.raises(RuntimeError, match="fp32"):
        mcem_dev.DecoderPack(ref.decoder, 1, "bf16x3", generic=True)
    N = 20
    em = mcem.MCEM_M2(niter=1, nsamples_E_step=3, burnin_E_step=4, nsamples_WF=4, burnin_WF=3)
    em.precision = "bf16x3"
    em.init_parameters(X=mixture_stft(N, 3), S=mixture_stft(N, 4), y=torch.ones(y_dim, N, device="cuda"), vae=m, nmf_rank=10, eps=np.finfo(float).eps,
                       device="cuda")
    with pytest.raises(RuntimeError, match="fp32"):
        em.run()
    # the library itself
    plan = mcem_dev.McemPlan()
    lib = native.load()
    assert lib.dvae_mcem_plan_dims(129, 128, 128, 0, 0, ctypes.byref(plan)) == 1001            # DVAE_E_BADARG
    with pytest.raises(Exception, match="128"):
        native.check(lib.dvae_mcem_plan_dims(129, 128, 128, 0, 0, ctypes.byref(plan)), "dvae_mcem_plan_dims")
    assert lib.dvae_mcem_plan_dims(16, 513, 128, 0, 0, ctypes.byref(plan)) == 1001
    assert lib.dvae_mcem_plan_dims(16, 128, 128, 514, 0, ctypes.byref(plan)) == 1001
    assert lib.dvae_mcem_plan_dims(32, 64, 256, 1, 2, ctypes.byref(plan)) == 1003              # DVAE_E_UNSUPPORTED: bf16x3
    assert lib.dvae_mcem_plan_dims(32, 64, 256, 1, 0, ctypes.byref(plan)) == 0
    assert (plan.x_dim, plan.z_dim, plan.h_dim, plan.h2_dim, plan.y_dim, plan.precision) == (513, 32, 64, 256, 1, 0) and plan.weights_bytes > 0
    assert lib.dvae_mcem_plan(1, 0, ctypes.byref(plan)) == 0 and (plan.z_dim, plan.h_dim, plan.h2_dim) == (16, 128, 0)      # unchanged
    # the fused start needs the encoder kernel's geometry
    frames = np.concatenate([mixture_stft(c, 50 + u).T for u, c in enumerate(EM_COUNTS)]).astype(np.complex64)
    spec = STFT.SpecBatch(t(frames), EM_COUNTS, [1024 + 256 * (c - 1) for c in EM_COUNTS], 1024, 256, False, 2)
    Y = [np.ones((y_dim, c), np.float32) for c in EM_COUNTS]
    mb = mcem_dev.McemBatch(m, niter=1)
    with pytest.raises(ValueError, match="fused_start"):
        mb.init_parameters(spec, Y, fused_start=True)
    mb.init_parameters(spec, Y)                                                                 # the default start runs vae.encoder at any size
    assert mb.Z.shape == (z_dim, mb.ntot) and mb._pack.generic

"""The batched encoder, the NMF start and the fused MCEM start on the MI355X (dvae_encode_batch, dvae_mcem_nmf_start;
disentangled-vae_amd/encode.py, McemBatch.init_parameters(fused_start=True)): the fixture cases within the bars of
tests/encode_ref.py, bit identity over sources, tile edges, batches and runs with untouched rows around the utterances, the column
output, refusals through the C ABI, the NMF start against float64, the fused start against the default path, reconstruct_batch
against DecoderPack.decode and a float64 decoder, and the enhancement example's --fused-start.

Bars (encode_ref.py): mu and log_var within 8 c_ref u M of the float64 network, c_ref per head measured on the reference's own
float32 CPU run and recorded in the fixture (mu / log_var: 0.115 / 0.095 for M1, 0.166 / 0.150 for M2 y_dim 1, 0.098 / 0.100 for M2
y_dim 513; bars of 5e-6 .. 2e-4 on outputs up to 3.3); z within bar_mu + |eps| exp(lv / 2) (bar_lv / 2 + 4 u) + u |z|.  Every test
prints its worst error in units of the bars before it asserts.

Measured on an MI355X (complex frames, power rows, power rows at a leading dimension of 520 and both label strides give the same
figures, worst error in bars of mu / log_var / z):
  M1 (y_dim 0):    0.118 / 0.165 / 0.091
  M2, y_dim 1:     0.184 / 0.164 / 0.172
  M2, y_dim 513:   0.104 / 0.088 / 0.092
The fused start's Z came out bit-equal to the default path's (0.000 bars apart; the bound is 2), 0.118 (M1, M2v3) and 0.184 (M2) bars
from float64; Vb of the NMF start at 0.38 (K = 10) and 0.76 (K = 3) of gamma_K |W||H|; reconstruct_batch's variance at 0.008 of the
decoder bound.
"""
import gc
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import encode_ref as ER
from test_encode_cpu import FRAMES, GOLD, labels_of, rebuild

pytestmark = pytest.mark.gpu
E = importlib.import_module("disentangled-vae_amd.encode")
C = importlib.import_module("disentangled-vae_amd.classify")
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.mcem")
N = importlib.import_module("disentangled-vae_amd.native")
from packages.models import models as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
COUNTS = [33, 65, 20]
EDGES = [1, 31, 32, 33, 63, 64, 65, 130]
U32 = ER.U32


def spec_of(frames, counts):
    return H.SpecBatch(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), counts, [1024 + 256 * (int(c) - 1) for c in counts], 1024, 256, False, 2)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


_case = {}


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """As in tests/test_gpu_classify.py: every device allocation of this module comes from a private pool of the caching allocator,
    emptied when the module is done, so that the default pool keeps exactly the cached blocks it had (tests/test_gpu_module_path.py
    holds torch.cuda.memory_allocated() flat to within 1 MiB); a BLAS workspace that the first matmul of the process allocated inside
    the pool is dropped with it."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _case.clear()
        gc.collect()
        torch.cuda.synchronize()
        if any(s["segment_type"] == "large" and any(b["state"].startswith("active") for b in s["blocks"]) for s in pool.snapshot()):
            torch._C._cuda_clearCublasWorkspaces()
    del pool


def case(name):
    """(pack, model on the device, encoder weights, [x | y] float32, c_ref mu, c_ref log_var) of a fixture case, made once."""
    if name not in _case:
        model, w = rebuild(name)
        model = model.to(DEV).eval()
        for p in model.parameters():
            p.requires_grad = False
        c_mu, c_lv = (float(c) for c in GOLD[name + "/c_ref"])
        _case[name] = (E.EncoderPack(model.encoder, ER.CASES[name]), model, w, ER.inputs(ER.power(FRAMES), labels_of(name)), c_mu, c_lv)
    return _case[name]


def wide(t, extra, fill=float("nan")):
    """The same rows at a row stride of `extra` more, the gap filled with NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, device=t.device, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    v = buf[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + extra
    return v


# ---- 1: the fixture cases within the bars -----------------------------------------------------------------------------------------------

FIXTURE_RUNS = [(c, s, l) for c in ER.CASES for s in ("complex", "rows", "rows_ld520") for l in (("packed", "wide") if ER.CASES[c] else ("none",))]


@pytest.mark.parametrize("name,source,label_stride", FIXTURE_RUNS, ids=["-".join(r) for r in FIXTURE_RUNS])
def test_fixture_case_within_the_bars(name, source, label_stride):
    pack, _, w, V, c_mu, c_lv = case(name)
    k = name + "/"
    y = dev(labels_of(name))
    if label_stride == "wide":
        y = wide(y, 2)
    eps = dev(GOLD[k + "eps"])
    if source == "complex":
        lat = E.encode_batch(pack, spec_of(FRAMES, COUNTS), y, eps=eps)
    else:
        P = dev(ER.power(FRAMES))
        lat = E.encode_batch(pack, wide(P, 7) if source == "rows_ld520" else P, y, COUNTS, eps=eps)
    assert lat.mu.shape == (118, 16) and lat.frame_off.tolist() == [0, 33, 98, 118] and lat.view(1, "z").shape == (16, 65)
    mu, lv, z = (t.cpu().numpy() for t in (lat.mu, lat.log_var, lat.z))
    ER.check(f"device {name} {source} labels {label_stride}", mu, lv, z, V, w, c_mu, c_lv, GOLD[k + "eps"])
    print(f"against the reference's recorded float32 outputs: mu {np.abs(mu - GOLD[k + 'mu']).max():.2e}, log_var "
          f"{np.abs(lv - GOLD[k + 'log_var']).max():.2e}, z {np.abs(z - GOLD[k + 'z']).max():.2e}")
    assert [a.shape for a in lat.numpy("log_var")] == [(16, c) for c in COUNTS]


@pytest.mark.parametrize("name", list(ER.CASES))
def test_sources_give_the_same_bits(name):
    """The power formed in the kernel is numpy's float32 power, so complex frames, power rows and strided rows give the same latents."""
    pack = case(name)[0]
    y, eps = dev(labels_of(name)), dev(GOLD[name + "/eps"])
    P = dev(ER.power(FRAMES))
    a = E.encode_batch(pack, spec_of(FRAMES, COUNTS), y, eps=eps)
    b = E.encode_batch(pack, P, y, COUNTS, eps=eps)
    c = E.encode_batch(pack, wide(P, 7), None if y is None else wide(y, 2), COUNTS, eps=eps)
    d = E.encode_batch(pack, H.SpecBatch(P, COUNTS, [0, 0, 0], 1024, 256, False, 1), y, eps=eps)
    for other in (b, c, d):
        for which in ("mu", "log_var", "z"):
            assert torch.equal(getattr(a, which), getattr(other, which)), which


# ---- 2: tile edges, batches, runs, untouched rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_tile_edges_alone_in_the_batch_and_twice(name):
    pack = case(name)[0]
    y_dim = ER.CASES[name]
    rng = np.random.default_rng(3)
    total, first, tail = sum(EDGES), 5, 70
    rows = first + total + tail
    frames = (rng.standard_normal((rows, 513)) + 1j * rng.standard_normal((rows, 513))).astype(np.complex64) * rng.random((rows, 1)).astype(np.float32) * 0.7
    src = dev(frames)
    y = dev((rng.random((rows, y_dim)) > 0.5).astype(np.float32)) if y_dim else None
    eps = dev(rng.standard_normal((rows, 16)).astype(np.float32))
    off = C.frame_table("test", EDGES, rows, first=first)

    def run(src, y, eps, off):
        outs = [torch.full((src.shape[0], 16), float("nan"), device=DEV) for _ in range(3)]
        E.encode_rows(pack, src, off, y, eps, *outs)
        return [o.cpu().numpy() for o in outs]

    batch, again = run(src, y, eps, off), run(src, y, eps, off)
    for a, b in zip(batch, again):
        assert np.array_equal(bits(a), bits(b))
    inside = np.zeros(rows, bool)
    inside[first:first + total] = True
    for nm, o in zip(("mu", "log_var", "z"), batch):
        assert np.all(np.isnan(o[~inside])), f"{nm}: rows outside the utterances were written"
        assert np.all(np.isfinite(o[inside])), f"{nm}: rows inside the utterances were left out"
    assert np.std(batch[0][inside]) > 0.05
    for u, c in enumerate(EDGES):
        a, b = int(off[u]), int(off[u + 1])
        alone = run(src[a:b].contiguous(), None if y is None else y[a:b].contiguous(), eps[a:b].contiguous(), np.array([0, c], np.int64))
        for nm, o, full in zip(("mu", "log_var", "z"), alone, batch):
            assert np.array_equal(bits(o), bits(full[a:b])), f"utterance {u} ({c} frames): {nm} differs alone and in the batch"
    print(f"{name}: {len(EDGES)} utterances of {EDGES} frames from row {first}: bit-identical alone, in the batch and twice; {first} + {tail} outer rows untouched")


# ---- 3: the column output ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_column_output_is_mu_transposed_and_leaves_the_pads(name):
    pack = case(name)[0]
    spec, y = spec_of(FRAMES, COUNTS), dev(labels_of(name))
    starts, ntot, *_ = M.McemBatch(None)._layout(COUNTS, torch.device(DEV))
    assert starts == [0, 64, 160] and ntot == 192
    lat = E.encode_batch(pack, spec, y)
    Z = torch.full((16, ntot), -7.5, device=DEV)
    E.encode_rows(pack, spec.frames, spec.frame_off, y, Z=Z, cols=starts)
    real = np.zeros(ntot, bool)
    for s, c in zip(starts, COUNTS):
        real[s:s + c] = True
    Zh = Z.cpu().numpy()
    assert np.all(Zh[:, ~real] == -7.5), "pad columns were written"
    assert np.array_equal(bits(Zh[:, real]), bits(lat.mu.cpu().numpy().T))
    # together with the row outputs, and at other columns
    mu = torch.empty((118, 16), device=DEV)
    Z2 = torch.full((16, 200), -7.5, device=DEV)
    E.encode_rows(pack, spec.frames, spec.frame_off, y, mu=mu, Z=Z2, cols=[3, 40, 180])
    assert torch.equal(mu, lat.mu)
    Z2h = Z2.cpu().numpy()
    assert np.array_equal(bits(np.concatenate([Z2h[:, 3:36], Z2h[:, 40:105], Z2h[:, 180:200]], axis=1)), bits(lat.mu.cpu().numpy().T))
    assert np.all(Z2h[:, :3] == -7.5) and np.all(Z2h[:, 36:40] == -7.5) and np.all(Z2h[:, 105:180] == -7.5)


# ---- 4: refusals through the C ABI ------------------------------------------------------------------------------------------------------

def test_bad_arguments_return_an_error_and_launch_nothing():
    lib = N.load()
    pack0, pack1 = case("m1")[0], case("m2_y1")[0]
    n, ntot = 40, 64
    src = torch.zeros((n, 513), device=DEV)
    y = torch.zeros((n, 1), device=DEV)
    eps = torch.zeros((n, 16), device=DEV)
    outs = [torch.full((n, 16), -7.5, device=DEV) for _ in range(3)]
    Z = torch.full((16, ntot), -7.5, device=DEV)
    table = lambda *v: np.asarray(v, np.int64)
    good, cols = table(0, 10, 40), table(0, 32)
    tab_dev = dev(np.concatenate([good, cols]))

    def call(src_p=N.ptr(src), cplx=0, ld=513, y_p=None, ldy=0, rows=n, U=2, off=good, pack=pack0, y_dim=0, eps_p=N.ptr(eps), mu=N.ptr(outs[0]),
             lv=N.ptr(outs[1]), z=N.ptr(outs[2]), Z_p=None, nt=0, col=None, tab=None):
        return lib.dvae_encode_batch(src_p, cplx, ld, y_p, ldy, rows, U, off.ctypes.data if off is not None else None, N.ptr(pack.weights), y_dim, eps_p,
                                     mu, lv, z, Z_p, nt, col.ctypes.data if col is not None else None, tab, N.stream())

    withZ = dict(Z_p=N.ptr(Z), nt=ntot, col=cols, tab=N.ptr(tab_dev))
    refused = {"all outputs null": lambda: call(mu=None, lv=None, z=None), "z without eps": lambda: call(eps_p=None),
               "y with y_dim 0": lambda: call(y_p=N.ptr(y), ldy=1), "y_dim 1 without y": lambda: call(pack=pack1, y_dim=1),
               "y_dim 7": lambda: call(y_p=N.ptr(y), ldy=7, y_dim=7), "null source": lambda: call(src_p=None), "null table": lambda: call(off=None),
               "ld 512": lambda: call(ld=512), "complex ld": lambda: call(cplx=1, ld=520), "no rows": lambda: call(rows=0),
               "label ld below y_dim": lambda: call(pack=pack1, y_dim=1, y_p=N.ptr(y), ldy=0),
               "decreasing table": lambda: call(off=table(0, 30, 20)), "negative start": lambda: call(off=table(-1, 10, 40)),
               "table past the rows": lambda: call(off=table(0, 10, 41)),
               "columns past ntot": lambda: call(**{**withZ, "col": table(0, 35)}), "columns going back": lambda: call(**{**withZ, "col": table(0, 9)}),
               "Z without the device table": lambda: call(**{**withZ, "tab": None}), "Z without columns": lambda: call(**{**withZ, "col": None})}
    for name, fn in refused.items():
        rc = fn()
        msg = lib.dvae_last_error().decode()
        print(f"{name}: code {rc}: {msg}")
        assert rc != 0 and "encode_batch" in msg, name
    assert lib.dvae_encode_weights_floats(7) == 0 and lib.dvae_encode_weights_floats(0) == pack0.weights.numel()
    assert lib.dvae_encode_weights_floats(1) == pack1.weights.numel() == pack0.weights.numel() + 128
    assert "utterance 1" in (call(off=table(0, 30, 20)), lib.dvae_last_error().decode())[1]
    assert "utterance 1" in (call(**{**withZ, "col": table(0, 35)}), lib.dvae_last_error().decode())[1]
    torch.cuda.synchronize()
    assert all(bool((o == -7.5).all()) for o in outs + [Z])
    assert call(**withZ) == 0
    torch.cuda.synchronize()
    assert not any(bool((o == -7.5).any()) for o in outs)
    Zh = Z.cpu().numpy()
    assert np.all(Zh[:, 10:32] == -7.5) and np.all(Zh[:, 62:] == -7.5) and not np.any(Zh[:, :10] == -7.5) and not np.any(Zh[:, 32:62] == -7.5)
    # the Python layer names the utterance before the library is asked
    with pytest.raises(ValueError, match="utterance 2"):
        E.encode_batch(pack0, src, counts=[10, 20, 11])
    with pytest.raises(ValueError, match="labels are needed exactly"):
        E.encode_batch(pack1, src, counts=[40])
    with pytest.raises(TypeError, match="Classifier"):
        E.encode_batch(PM.Classifier([513, [128, 128], 16]).to(DEV), src)


# ---- 5: the NMF start -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [10, 3])
def test_nmf_start_clamps_and_multiplies(K):
    eps = 2.220446049250313e-16
    starts, ntot, *_ = M.McemBatch(None)._layout(COUNTS, torch.device(DEV))
    U = len(COUNTS)
    torch.manual_seed(K)
    W0 = torch.rand((U, 513, K), device=DEV)
    H0 = torch.rand((K, ntot), device=DEV)
    W0[0, 0, 0] = 0.0; W0[2, 512, K - 1] = 0.0; H0[0, 0] = 0.0; H0[K - 1, starts[2] + 19] = 0.0      # a draw of exactly zero meets the clamp
    W, Hm = W0.clone(), H0.clone()
    Vb = torch.full((513, ntot), float("nan"), device=DEV)
    tab = dev(np.concatenate([np.concatenate([[0], np.cumsum(COUNTS)]), starts]).astype(np.int64))
    N.check(N.load().dvae_mcem_nmf_start(N.ptr(W), N.ptr(Hm), N.ptr(Vb), ntot, K, U, N.ptr(tab), eps, N.stream()), "dvae_mcem_nmf_start")
    Wh, Hh, Vh = W.cpu().numpy(), Hm.cpu().numpy(), Vb.cpu().numpy()
    real = np.zeros(ntot, bool)
    for s, c in zip(starts, COUNTS):
        real[s:s + c] = True
    e32 = np.float32(eps)
    assert np.array_equal(Wh, np.maximum(W0.cpu().numpy(), e32)) and Wh.min() == e32 and Wh.max() < 1
    assert np.array_equal(Hh[:, real], np.maximum(H0.cpu().numpy()[:, real], e32)) and Hh[:, real].min() == e32 and Hh[:, real].max() < 1
    assert np.all(Hh[:, ~real] == 1) and np.all(Vh[:, ~real] == 1)
    gamma = K * U32 / (1 - K * U32)
    worst = 0.0
    for u, (s, c) in enumerate(zip(starts, COUNTS)):
        want = Wh[u].astype(np.float64) @ Hh[:, s:s + c].astype(np.float64)
        err = np.abs(Vh[:, s:s + c].astype(np.float64) - want) / (gamma * want)          # W, H > 0: |W||H| = W H
        worst = max(worst, float(err.max()))
    print(f"K {K}: worst |Vb - W H| = {worst:.3f} gamma_K |W||H|")
    assert worst <= 1.0
    # and it is the chain as written: fma from 0 with k ascending
    # float64 holds a product of two float32 exactly; its sum with the chain is rounded once more than an fma's, which can change the
    # float32 result only where the sum lies within that rounding of a float32 midpoint: such elements (and what follows them in
    # their chain) are set aside, the others must be equal
    s0, c0 = starts[1], 65
    chain = np.zeros((513, c0), np.float64)
    unsure = np.zeros((513, c0), bool)
    for k in range(K):
        t = Wh[1][:, k:k + 1].astype(np.float64) * Hh[k:k + 1, s0:s0 + c0].astype(np.float64) + chain
        r = t.astype(np.float32)
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            mid = (r.astype(np.float64) + np.nextafter(r, side).astype(np.float64)) / 2
            unsure |= np.abs(t - mid) <= 4 * np.spacing(np.abs(t))
        chain = r.astype(np.float64)
    assert unsure.mean() < 1e-3
    assert np.array_equal(chain.astype(np.float32)[~unsure], Vh[:, s0:s0 + c0][~unsure])


# ---- 6: the fused start of McemBatch ----------------------------------------------------------------------------------------------------

def _v3_model():
    torch.manual_seed(7)
    m = PM.DeepGenerativeModel_v5([513, 1, 16, [128, 128]])
    with torch.no_grad():
        for l in m.modules():
            if isinstance(l, torch.nn.Linear):
                l.bias.normal_(0.0, 0.05)
    return m.to(DEV).eval().enc_dec_clf


@pytest.mark.parametrize("variant", ["M1", "M2", "M2v3"])
def test_fused_start_against_the_default_path(variant):
    spec = spec_of(FRAMES, COUNTS)
    y1 = dev(labels_of("m2_y1"))
    lb = C.LabelBatch(y1, y1, COUNTS)
    if variant == "M1":
        vae, labels, kw, c_name, enc_labels = case("m1")[1], None, dict(label_in_encoder=False, label_in_decoder=False), "m1", None
    elif variant == "M2":
        vae, labels, kw, c_name, enc_labels = case("m2_y1")[1], lb, dict(label_in_encoder=True, label_in_decoder=True), "m2_y1", lb
    else:
        vae, labels, kw, c_name, enc_labels = _v3_model(), lb, dict(label_in_encoder=False, label_in_decoder=True), "m1", None
    for p in vae.parameters():
        p.requires_grad = False
    mk = lambda: M.McemBatch(vae, niter=2, nsamples_E_step=4, burnin_E_step=3, nsamples_WF=3, burnin_WF=3, reference_m1_counts=False, **kw)
    base, fused, again = mk(), mk(), mk()
    torch.manual_seed(11); base.init_parameters(spec, labels)
    torch.manual_seed(11); fused.init_parameters(spec, labels, fused_start=True)
    torch.manual_seed(11); again.init_parameters(spec, labels, fused_start=True)
    assert np.array_equal(bits(fused.X2), bits(base.X2))
    assert (fused.y is None) == (base.y is None) == (variant == "M1")
    if base.y is not None:
        assert fused.y.shape == base.y.shape and np.array_equal(bits(fused.y), bits(base.y))
    for nm in ("Z", "W", "H", "Vb", "g"):
        assert getattr(fused, nm).shape == getattr(base, nm).shape and getattr(fused, nm).is_contiguous()
        assert np.array_equal(bits(getattr(fused, nm)), bits(getattr(again, nm))), f"{nm} is not reproducible under the same seed"
    real = np.zeros(fused.ntot, bool)
    for s, c in zip(fused.starts, COUNTS):
        real[s:s + c] = True
    lat = E.encode_batch(vae.encoder, spec, enc_labels)
    Zf, Zb = fused.Z.cpu().numpy(), base.Z.cpu().numpy()
    assert np.array_equal(bits(Zf[:, real]), bits(lat.mu.cpu().numpy().T)) and np.all(Zf[:, ~real] == 0)
    w = ER.encoder_weights(vae.encoder)
    V = ER.inputs(ER.power(FRAMES), labels_of("m2_y1") if variant == "M2" else None)
    c_mu, c_lv = (float(c) for c in GOLD[c_name + "/c_ref"])
    bar_mu = ER.bars(*ER.masses(V, w), c_mu, c_lv)[0]
    mu64 = ER.forward64(V, w)[0]
    between = float(np.max(np.abs(Zf[:, real].astype(np.float64) - Zb[:, real]) / bar_mu.T))
    print(f"{variant}: fused Z at {ER.worst(Zf[:, real].T, mu64, bar_mu):.3f} bars of float64, the default path's at {ER.worst(Zb[:, real].T, mu64, bar_mu):.3f}; "
          f"apart by {between:.3f} bars")
    assert between <= 2.0
    Wh, Hh = fused.W.cpu().numpy(), fused.H.cpu().numpy()
    assert Wh.min() > 0 and Wh.max() < 1 and Hh[:, real].max() < 1 and np.all(Hh[:, ~real] == 1) and np.all(fused.Vb.cpu().numpy()[:, ~real] == 1)
    assert bool((fused.g == 1).all())
    cost = fused.run()
    assert cost.shape == (2, 3) and np.all(np.isfinite(cost))
    s_hat, n_hat = fused.enhance()
    for wb in (s_hat, n_hat):
        assert wb.lengths == spec.lengths and all(np.all(np.isfinite(a)) and np.any(a != 0) for a in wb.numpy())
    with pytest.raises(TypeError, match="fused_start needs a SpecBatch"):
        mk().init_parameters(spec.numpy(), None if labels is None else labels.numpy(), fused_start=True)


# ---- 7: reconstruct_batch ---------------------------------------------------------------------------------------------------------------

def _decode_bound():
    """(rtol, atol) that tests/test_gpu_mcem.py holds dvae_mcem_decode's variances to against its oracle, read from that test."""
    import test_gpu_mcem
    m = re.search(r"assert_allclose\(Vs, Vs_o, rtol=([0-9.e+-]+), atol=([0-9.e+-]+)\)", inspect.getsource(test_gpu_mcem.test_sample_posterior_matches_oracle))
    assert m, "tests/test_gpu_mcem.py no longer states the bound of the decoder variances"
    return float(m.group(1)), float(m.group(2))


def _decoder64(decoder, rows):
    l3, l4, l5 = ([t.detach().cpu().numpy().astype(np.float64) for t in (l.weight, l.bias)] for l in (*decoder.hidden, decoder.reconstruction))
    h = np.tanh(np.tanh(rows @ l3[0].T + l3[1]) @ l4[0].T + l4[1])
    return np.exp(h @ l5[0].T + l5[1])


@pytest.mark.parametrize("name,with_eps", [("m1", True), ("m2_y1", False), ("m2_y1", True), ("m2_y513", True)])
def test_reconstruct_batch(name, with_eps):
    _, model, *_ = case(name)
    y_dim = ER.CASES[name]
    spec, y = spec_of(FRAMES, COUNTS), dev(labels_of(name))
    eps = dev(GOLD[name + "/eps"]) if with_eps else None
    var, lat = E.reconstruct_batch(model, spec, y, eps)
    assert var.shape == (513, 118) and var.is_contiguous() and lat.counts == COUNTS
    zrows = lat.z if with_eps else lat.mu
    assert (lat.z is None) == (not with_eps)
    pack = M.DecoderPack(model.decoder, y_dim)
    yc = y.T.contiguous() if y_dim else None
    assert torch.equal(var, pack.decode(zrows[:, None, :].contiguous(), yc)[0])
    z64 = zrows.cpu().numpy().astype(np.float64)
    want = _decoder64(model.decoder, z64 if not y_dim else np.concatenate([z64, labels_of(name).astype(np.float64)], axis=1)).T
    rtol, atol = _decode_bound()
    got = var.cpu().numpy().astype(np.float64)
    print(f"{name}: variance against float64 exp(decoder): worst {float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))):.3f} of the bound (rtol {rtol}, atol {atol})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)
    if y_dim == 1:                                           # the disentanglement analysis: the same latents under all-ones and all-zeros
        ones, _ = E.reconstruct_batch(model, spec, y, eps, decode_labels=torch.ones_like(y))
        zeros, _ = E.reconstruct_batch(model, spec, y, eps, decode_labels=torch.zeros_like(y))
        assert torch.equal(ones[:, (y[:, 0] == 1)], var[:, (y[:, 0] == 1)]) and torch.equal(zeros[:, (y[:, 0] == 0)], var[:, (y[:, 0] == 0)])
        assert not torch.equal(ones, zeros)


# ---- 8: the enhancement example ---------------------------------------------------------------------------------------------------------

def test_enhance_mcem_example_with_the_fused_start(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "enhance_mcem.py"), "--synthetic", "2", "--niter", "2", "--fused-start",
                        "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr, sep="\n")
    assert r.returncode == 0
    assert len(list(tmp_path.glob("*_s_est.wav"))) == 2

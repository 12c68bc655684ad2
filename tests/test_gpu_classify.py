"""The batched classifier and the batched F1 score on the MI355X (dvae_classify_batch, dvae_label_counts_batch;
disentangled-vae_amd/classify.py): the fixture cases within the bars of tests/classify_ref.py, bit identity over tile edges, batches
and runs with untouched rows around the utterances, the in-kernel power against McemBatch's, exact confusion counts, f1_loss's bits,
the device-to-device hand-over to McemBatch, refusals through the C ABI and the enhancement example's classifier path.

Bars (classify_ref.py): logits within 8 c_ref u M of the float64 network, c_ref measured on the reference's own float32 CPU run and
recorded in the fixture (0.0065 at y_dim 1, 0.0204 at y_dim 513); soft within a quarter of that plus 4 u; hard equal to the float64
decision outside |logit64| <= 2 bars + 4 u, a set that may hold at most 0.1 % of a case.  Every test prints its worst error in units
of the bars and the excluded share before it asserts.

A frame prefix table has no rows between two utterances; the rows that must stay untouched are those before the first utterance
and after the last one, and the tile-edge test places sentinels in both.

Measured on an MI355X (complex frames, power rows and power rows at a leading dimension of 520 give the same figures):
  y_dim 1:    worst logit error 0.144 bars, worst soft error 0.162 bars, excluded share 0,       no hard label off, all equal to the reference's
  y_dim 513:  worst logit error 0.136 bars, worst soft error 0.201 bars, excluded share 1.65e-5, no hard label off, all equal to the reference's
"""
import gc
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_ref as CR
from test_classify_cpu import GOLD, rebuild, same_bits

pytestmark = pytest.mark.gpu
C = importlib.import_module("disentangled-vae_amd.classify")
H = importlib.import_module("disentangled-vae_amd.stft")
M = importlib.import_module("disentangled-vae_amd.mcem")
N = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.target")
from packages.models import models as PM
from packages.models import utils as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EDGES = [1, 31, 32, 33, 63, 64, 65, 130]
SENTINEL = -7.5


def spec_of(frames, counts):
    return H.SpecBatch(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), counts, [1024 + 256 * (int(c) - 1) for c in counts], 1024, 256, False, 2)


_case = {}


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """Every device allocation of this module comes from a private pool of the caching allocator, which is emptied when the module is
    done: the default pool keeps exactly the cached blocks it had.  test_gpu_module_path.py holds torch.cuda.memory_allocated() flat to
    within 1 MiB, and that figure counts the unsplit remainder (up to 1 MiB) of every cached block a large request is served from, so
    it depends on the blocks that the modules before it left behind; torch.cuda.empty_cache() here would change them as well.  A BLAS
    workspace that the first matmul of the process allocated inside the pool (the only block above 1 MiB that outlives the tests) is
    dropped with it, so that the next matmul allocates it from the default pool as it would have without this module."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _case.clear()
        gc.collect()
        torch.cuda.synchronize()
        if any(s["segment_type"] == "large" and any(b["state"].startswith("active") for b in s["blocks"]) for s in pool.snapshot()):
            torch._C._cuda_clearCublasWorkspaces()
    del pool


def case(y_dim):
    """(pack, float64 logits, mass, c_ref) of a fixture case, computed once."""
    if y_dim not in _case:
        clf, w = rebuild(GOLD, y_dim)
        P = CR.power(GOLD["frames"])
        _case[y_dim] = (C.ClassifierPack(clf.to(DEV)), CR.logits64(P, w), CR.mass(P, w), float(GOLD[f"y{y_dim}/c_ref"]))
    return _case[y_dim]


# ---- 1: the fixture cases within the bars -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["complex", "rows", "rows_ld520"])
@pytest.mark.parametrize("y_dim", [1, 513])
def test_fixture_case_within_the_bars(y_dim, source):
    pack, z64, mass, c_ref = case(y_dim)
    counts = GOLD["counts"].tolist()
    if source == "complex":
        lb = C.classify_batch(pack, spec_of(GOLD["frames"], counts), want_logits=True)
    else:
        P = torch.from_numpy(CR.power(GOLD["frames"])).to(DEV)
        if source == "rows_ld520":
            wide = torch.full((P.shape[0], 520), float("nan"), device=DEV)
            wide[:, :513] = P
            P = wide[:, :513]
            assert P.stride(0) == 520
        lb = C.classify_batch(pack, P, counts, want_logits=True)
    assert lb.soft.shape == (sum(counts), y_dim) and lb.frame_off.tolist() == [0, 33, 98, 118] and lb[1].shape == (y_dim, 65)
    logit, soft, hard = (t.cpu().numpy() for t in (lb.logits, lb.soft, lb.hard))
    CR.check(f"device y_dim {y_dim} {source}", logit, soft, hard, z64, mass, c_ref)
    assert np.array_equal(hard, (soft > 0.5).astype(np.float32))                        # decided from the kernel's own soft
    agree = float(np.mean(hard == GOLD[f"y{y_dim}/hard"]))
    print(f"hard labels equal to the reference's recorded ones: {agree:.6f}")
    assert [a.shape for a in lb.numpy()] == [(y_dim, c) for c in counts]


def test_sources_give_the_same_bits():
    """The power formed in the kernel is the host's float32 power, so complex frames and power rows give the same labels."""
    pack = case(513)[0]
    counts = GOLD["counts"].tolist()
    a = C.classify_batch(pack, spec_of(GOLD["frames"], counts), want_logits=True)
    b = C.classify_batch(pack, torch.from_numpy(CR.power(GOLD["frames"])).to(DEV), counts, want_logits=True)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.soft, b.soft) and torch.equal(a.hard, b.hard)


# ---- 2: tile edges, batches, runs, untouched rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("y_dim", [1, 513])
def test_tile_edges_alone_in_the_batch_and_twice(y_dim):
    pack = case(y_dim)[0]
    rng = np.random.default_rng(3)
    total, first, tail = sum(EDGES), 5, 70
    rows = first + total + tail
    frames = (rng.standard_normal((rows, 513)) + 1j * rng.standard_normal((rows, 513))).astype(np.complex64) * rng.random((rows, 1)).astype(np.float32) * 30
    src = torch.from_numpy(frames).to(DEV)
    off = C.frame_table("test", EDGES, rows, first=first)

    def run(src, off):
        outs = [torch.full((src.shape[0], y_dim), SENTINEL, device=DEV) for _ in range(3)]
        C.classify_rows(pack, src, off, outs[0], outs[1], outs[2])
        return [o.cpu().numpy() for o in outs]

    batch, again = run(src, off), run(src, off)
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    inside = np.zeros(rows, bool)
    inside[first:first + total] = True
    for name, o in zip(("soft", "hard", "logits"), batch):
        assert np.all(o[~inside] == SENTINEL), f"{name}: rows outside the utterances were written"
        assert not np.any(o[inside] == SENTINEL), f"{name}: rows inside the utterances were left out"
    assert 0.02 < batch[1][inside].mean() < 0.98
    for u, c in enumerate(EDGES):
        a, b = int(off[u]), int(off[u + 1])
        alone = run(src[a:b].contiguous(), np.array([0, c], np.int64))
        for name, o, full in zip(("soft", "hard", "logits"), alone, batch):
            assert np.array_equal(o.view(np.uint32), full[a:b].view(np.uint32)), f"utterance {u} ({c} frames): {name} differs alone and in the batch"
    print(f"y_dim {y_dim}: {len(EDGES)} utterances of {EDGES} frames: bit-identical alone, in the batch and twice; {first} + {tail} outer rows untouched")


# ---- 3: the in-kernel power is McemBatch's ----------------------------------------------------------------------------------------------

def test_in_kernel_power_equals_mcem_x2():
    """An identity-like network reads the power back through the logits: W1 picks 128 bins (one 1 per row), W2 is the identity, W3
    copies hidden unit j to output j; every sum is then one exact product and zeros, and relu passes a power as it is."""
    counts = [33, 65, 20]
    frames = GOLD["frames"].copy()
    frames[0, :4] = [0, 1e-30 + 0j, 3e18j, 1 + 1j]
    frames[40, 512] = 5e-15 - 2e-15j
    spec = spec_of(frames, counts)
    starts, ntot, *_ = M.McemBatch(None)._layout(counts, torch.device(DEV))
    X2 = torch.ones((513, ntot), dtype=torch.float32, device=DEV)
    tab = torch.from_numpy(np.concatenate([spec.frame_off, np.asarray(starts, np.int64)])).to(DEV)
    N.check(N.load().dvae_mcem_spec_init(N.ptr(spec.frames), sum(counts), 3, N.ptr(tab), N.ptr(X2), ntot, N.stream()), "dvae_mcem_spec_init")
    want = torch.cat([X2[:, s:s + c] for s, c in zip(starts, counts)], dim=1).T.cpu().numpy()          # [frames, 513]
    assert np.array_equal(want, CR.power(frames))
    clf = PM.Classifier([513, [128, 128], 513])
    got = np.zeros_like(want)
    for p in range(5):
        bins = np.minimum(np.arange(128) + 128 * p, 512) if p < 4 else np.arange(385, 513)
        with torch.no_grad():
            for l in (*clf.hidden, clf.output_layer):
                l.weight.zero_(); l.bias.zero_()
            clf.hidden[0].weight[np.arange(128), bins] = 1.0
            clf.hidden[1].weight.copy_(torch.eye(128))
            clf.output_layer.weight[:128] = torch.eye(128)
        lb = C.classify_batch(C.ClassifierPack(clf.to(DEV)), spec, want_logits=True)
        clf = clf.cpu()
        logits = lb.logits.cpu().numpy()
        assert np.all(logits[:, 128:] == 0)
        got[:, bins] = logits[:, :128]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    print(f"in-kernel power equals McemBatch.X2 on all {want.size} bins (max {want.max():.3g}, zeros {int((want == 0).sum())})")


# ---- 4: counts and F1 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("y_dim,ld", [(1, 1), (1, 3), (7, 9), (513, 513)])
def test_label_counts_match_numpy(y_dim, ld):
    rng = np.random.default_rng(y_dim)
    counts = [1, 70, 4096 // y_dim + 3, 2, 129]
    n = sum(counts) + 11
    pred = (rng.random((n, ld)) > 0.6).astype(np.float32) * rng.choice([1.0, -2.0, 0.5], (n, ld)).astype(np.float32)
    truth = (rng.random((n, ld)) > 0.3).astype(np.float32)
    got = C.label_counts_batch(torch.from_numpy(pred).to(DEV)[:, :y_dim], torch.from_numpy(truth).to(DEV)[:, :y_dim], counts).cpu().numpy()
    off = np.concatenate([[0], np.cumsum(counts)])
    want = np.stack([CR.counts(pred[a:b, :y_dim], truth[a:b, :y_dim]) for a, b in zip(off[:-1], off[1:])])
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    assert np.array_equal(got.sum(axis=1), np.asarray(counts) * y_dim)


@pytest.mark.parametrize("y_dim", [1, 513])
def test_f1_batch_matches_the_recorded_f1_loss_bits(y_dim):
    k = f"y{y_dim}/"
    counts = GOLD["counts"].tolist()
    pred = torch.from_numpy(GOLD[k + "hard"].astype(np.float32)).to(DEV)
    truth = torch.from_numpy(GOLD[k + "truth"].astype(np.float32)).to(DEV)
    got = C.f1_batch(pred, truth, float(GOLD["epsilon"]), counts=counts)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (3, 4)
    print(got.cpu().numpy(), GOLD[k + "f1"])
    assert same_bits(got.cpu().numpy(), GOLD[k + "f1"])
    assert np.array_equal(C.label_counts_batch(pred, truth, counts).cpu().numpy(), GOLD[k + "counts"])
    # the drop-in form, and f1_loss itself on the device, utterance by utterance
    off = np.concatenate([[0], np.cumsum(counts)])
    many = PU.f1_loss_many([pred[a:b].reshape(-1) for a, b in zip(off[:-1], off[1:])], [truth[a:b].reshape(-1) for a, b in zip(off[:-1], off[1:])], 1e-8)
    assert same_bits(np.array([[v.item() for v in row] for row in many], np.float32), GOLD[k + "f1"])
    # a LabelBatch as the prediction
    lb = C.LabelBatch(pred, pred, counts)
    assert torch.equal(C.f1_batch(lb, truth, counts=counts), got)


def speechlike(n, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    return env * rng.standard_normal(n) * 0.1


def test_f1_of_classifier_labels_against_the_clean_speech_vad_on_the_device():
    """pred from classify_batch, truth the FrameBatch of the batched front end (the device form behind clean_speech_VAD_many), on the
    same utterances: the rows meet in the count kernel, only the [U, 4] result is downloaded."""
    pack = case(1)[0]
    fb = T.utterances_to_frames([speechlike(n, 20 + u) for u, n in enumerate((9000, 20000, 4096))], "vad_labels", device=DEV)
    lb = C.classify_batch(pack, fb)
    assert lb.counts == fb.counts and lb.hard.shape == fb.Y.shape
    got = C.f1_batch(lb, fb).cpu().numpy()
    hard, truth = lb.hard.cpu().numpy(), fb.Y.cpu().numpy()
    want = CR.f1_from_counts(np.stack([CR.counts(hard[a:b], truth[a:b]) for a, b in zip(fb.frame_off[:-1], fb.frame_off[1:])]))
    print(got)
    assert same_bits(got, want) and 0 < truth.mean() < 1
    with pytest.raises(ValueError, match="utterance 1"):
        C.f1_batch(lb, C.LabelBatch(fb.Y, fb.Y, [fb.counts[0], fb.counts[1] - 1, fb.counts[2] + 1]))


# ---- 5: the hand-over to McemBatch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use", ["hard", "soft"])
def test_mcem_takes_a_label_batch_device_to_device(use):
    torch.manual_seed(4)
    model = PM.DeepGenerativeModel_v5([513, 1, 16, [128, 128]]).to(DEV).eval()
    counts = GOLD["counts"].tolist()
    spec = spec_of(GOLD["frames"], counts)
    with torch.no_grad():
        model.enc_dec_clf.classifier.output_layer.bias.fill_(-0.05)        # xavier weights with zero biases sit on one side
    lb = C.classify_batch(model.enc_dec_clf.classifier, spec)
    ys = []
    for form in (lb, lb.numpy(use)):
        mb = M.McemBatch(model.enc_dec_clf, niter=1, label_in_encoder=False, label_in_decoder=True)
        torch.manual_seed(9)
        mb.init_parameters(spec, form, use=use) if form is lb else mb.init_parameters(spec, form)
        ys.append(mb.y.cpu().numpy())
    assert ys[0].shape == (1, mb.ntot) and np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32))
    got = np.concatenate([ys[0][:, s:s + c] for s, c in zip(mb.starts, counts)], axis=1)
    assert np.array_equal(got, getattr(lb, use).cpu().numpy().T)
    with pytest.raises(ValueError, match="utterance 2"):
        M.McemBatch(model.enc_dec_clf, label_in_encoder=False).init_parameters(spec, C.LabelBatch(lb.soft, lb.hard, [33, 65, 19]))


# ---- 6: refusals through the C ABI ------------------------------------------------------------------------------------------------------

def test_bad_arguments_return_an_error_and_launch_nothing():
    lib = N.load()
    pack = case(1)[0]
    n = 40
    src = torch.zeros((n, 513), device=DEV)
    outs = [torch.full((n, 1), SENTINEL, device=DEV) for _ in range(2)]
    cnt = torch.full((2, 4), -3, dtype=torch.int64, device=DEV)
    table = lambda *v: np.asarray(v, np.int64)
    good = table(0, 10, 40)
    good_dev = torch.from_numpy(good).to(DEV)

    def classify(src_p=N.ptr(src), cplx=0, ld=513, rows=n, U=2, off=good, w=N.ptr(pack.weights), y=1, soft=N.ptr(outs[0]), hard=N.ptr(outs[1])):
        return lib.dvae_classify_batch(src_p, cplx, ld, rows, U, off.ctypes.data if off is not None else None, w, y, soft, hard, None, N.stream())

    def count(p=N.ptr(outs[0]), t=N.ptr(outs[1]), off=good, off_dev=N.ptr(good_dev), out=N.ptr(cnt), y=1, ld=1):
        return lib.dvae_label_counts_batch(p, ld, t, ld, n, y, 2, off.ctypes.data if off is not None else None, off_dev, out, N.stream())

    refused = {"null source": lambda: classify(src_p=None), "null weights": lambda: classify(w=None), "null soft": lambda: classify(soft=None),
               "null table": lambda: classify(off=None), "y_dim 2": lambda: classify(y=2), "ld 512": lambda: classify(ld=512),
               "complex ld": lambda: classify(cplx=1, ld=520), "no rows": lambda: classify(rows=0),
               "decreasing table": lambda: classify(off=table(0, 30, 20)), "negative start": lambda: classify(off=table(-1, 10, 40)),
               "table past the rows": lambda: classify(off=table(0, 10, 41)),
               "counts: null pred": lambda: count(p=None), "counts: null device table": lambda: count(off_dev=None), "counts: null out": lambda: count(out=None),
               "counts: decreasing table": lambda: count(off=table(0, 30, 20)), "counts: ld below y_dim": lambda: count(y=2, ld=1)}
    for name, call in refused.items():
        rc = call()
        msg = lib.dvae_last_error().decode()
        print(f"{name}: code {rc}: {msg}")
        assert rc != 0 and ("classify_batch" in msg or "label_counts_batch" in msg), name
    assert "utterance 1" in (classify(off=table(0, 30, 20)), lib.dvae_last_error().decode())[1]
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs) and bool((cnt == -3).all())
    assert classify() == 0 and count() == 0
    torch.cuda.synchronize()
    assert not bool((outs[0] == SENTINEL).any()) and cnt.sum().item() == n


# ---- 7: the enhancement example ---------------------------------------------------------------------------------------------------------

def test_enhance_mcem_example_labels_with_the_classifier(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "enhance_mcem.py"), "--labels", "classifier", "--synthetic", "4", "--niter", "2",
                        "--score", "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr, sep="\n")
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    head = next(i for i, line in enumerate(lines) if "F1" in line and "utterance" in line)
    rows = [line.split() for line in lines[head + 1:] if line.startswith("synthetic_")]
    assert len(rows) == 4
    for row in rows:
        assert all(np.isfinite(float(v)) for v in row[1:]) and 0.0 <= float(row[-1]) <= 1.0, row
    assert len(list(tmp_path.glob("*_s_est.wav"))) == 4

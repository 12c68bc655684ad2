"""Batched training-set front end on the MI355X (dvae_peak_normalise_batch, dvae_vad_labels_batch, dvae_ibm_labels_batch and
utterances_to_frames / the *_many drop-ins): the reference's label files, and bit-identity per utterance to the single-signal calls
on ragged batches from one frame to 60 s and past 2 GiB of complex frames."""
import importlib
import os

import numpy as np
import pytest
import torch

from packages.processing import target as P
from packages.processing.stft import stft

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.target")
H = importlib.import_module("disentangled-vae_amd.stft")
DeviceFrames = importlib.import_module("disentangled-vae_amd.frames").DeviceFrames
FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "labels_fixture.npz"))
UTTS = ["08F_sa2", "01M_sa1", "08F_si519"]
KW = dict(fs=16000, wlen_sec=64e-3, hop_percent=0.25)


def unpack(key):
    shape = tuple(FIX[key + "_shape"])
    return np.unpackbits(FIX[key + "_bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)


def speechlike(n, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 1600 + 1) > 0.4).astype(np.float64), 1600)[:n]
    return amp * (env * rng.standard_normal(n) * 0.3 + 0.003 * rng.standard_normal(n))


def end_pad_lengths():
    """One length the end-pad rule leaves alone and one it pads (both multiples of the hop)."""
    plain = next(k * 256 for k in range(40, 400) if not H.needs_end_pad(k * 256, **KW))
    padded = next(k * 256 for k in range(40, 400) if H.needs_end_pad(k * 256, **KW))
    return plain, padded


def ragged_set():
    plain, padded = end_pad_lengths()
    zeros_run = speechlike(30000, 3)
    zeros_run[5000:9000] = 0.0                                        # a run of exact zeros longer than nfft: min energy 0
    return [speechlike(1024, 1),                                      # exactly one frame
            speechlike(plain, 2), speechlike(padded, 4), zeros_run,
            speechlike(80000, 5),                                     # 5 s
            speechlike(20000, 6, 1e-30), speechlike(20000, 7, 1e30),  # the peak normalisation's range
            speechlike(960000, 8),                                    # 60 s
            speechlike(1024 + 100, 9)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def check_against_single(speeches, fb, labels, which=None, **kw):
    for u in (range(len(speeches)) if which is None else which):
        X1, Y1 = T.utterance_to_frames(speeches[u], labels, **kw)
        X, Y = fb.frames(u)
        assert same(X, X1), (labels, u)
        assert same(Y, Y1), (labels, u)


def test_reference_label_files_in_one_batch():
    raws = [FIX[u + "_wav_i16"].astype(np.float64) / 32768.0 for u in UTTS]
    speeches = [raws[0], speechlike(40000, 11), raws[1], speechlike(1500, 12), raws[2]]
    at = {UTTS[0]: 0, UTTS[1]: 2, UTTS[2]: 4}
    fv = T.utterances_to_frames(speeches, "vad_labels")
    fi = T.utterances_to_frames(speeches, "ibm_labels")
    assert torch.equal(fv.X, fi.X)
    for utt, u in at.items():
        assert np.array_equal(fv.frames(u)[1].cpu().numpy(), unpack(utt + "_vad").T), utt
        ibm = fi.frames(u)[1].cpu().numpy().T
        ref = unpack(utt + "_ibm")
        assert ibm.shape == ref.shape
        mism = ibm != ref
        if mism.any():                         # as tests/test_gpu_target.py: only bins within 1e-4 dB of the threshold may differ
            sp = speeches[u] / np.max(np.abs(speeches[u]))
            S = stft(sp, win="hann", dtype="complex64", center=False, pad_mode="reflect", pad_at_end=True, **KW)
            db = 20 * np.log10(np.abs(S) + np.float32(1e-8))
            assert np.all(np.abs(db[mism] - (db.max() - 50)) < 1e-4), int(mism.sum())
        assert mism.mean() < 1e-5
    check_against_single(speeches, fv, "vad_labels")
    check_against_single(speeches, fi, "ibm_labels")


@pytest.mark.parametrize("labels", ["vad_labels", "ibm_labels"])
def test_ragged_batch_is_bit_identical_to_single_calls(labels):
    speeches = ragged_set()
    fb = T.utterances_to_frames(speeches, labels, vad_threshold=1.2)
    assert fb.X.shape == (sum(fb.counts), 513) and fb.Y.shape == (sum(fb.counts), 1 if labels == "vad_labels" else 513)
    assert fb.counts[0] == 1
    check_against_single(speeches, fb, labels, vad_threshold=1.2)
    if labels == "vad_labels":
        Y = fb.frames(3)[1]
        assert 0 < float(Y.mean()) < 1


def test_peak_normalise_matches_numpy_and_leaves_the_rest():
    speeches = ragged_set()
    n = [len(s) for s in speeches]
    x0 = np.concatenate([[7], 7 + np.cumsum(np.array(n) + 13)[:-1]]).astype(np.int64)    # 13 sentinel samples between utterances
    buf = np.full(int(x0[-1] + n[-1] + 5), -3.25)
    for s, a in zip(speeches, x0):
        buf[a:a + len(s)] = s
    x = torch.from_numpy(buf).cuda()
    peak = T.peak_normalise_batch(x, x0, n).cpu().numpy()
    got = x.cpu().numpy()
    want = buf.copy()
    for s, a in zip(speeches, x0):
        want[a:a + len(s)] = s / np.max(np.abs(s))
    assert np.array_equal(got, want)                                  # IEEE division, sentinels untouched
    assert np.array_equal(peak, [np.max(np.abs(s)) for s in speeches])


@pytest.mark.parametrize("center,wlen", [(True, 50e-3), (False, 64e-3)])
@pytest.mark.parametrize("thr", [1.70, 1.2])
def test_vad_many_equals_the_single_calls(center, wlen, thr):
    kw = dict(fs=16e3, wlen_sec=wlen, hop_percent=0.25, center=center, pad_mode="reflect", pad_at_end=True, vad_threshold=thr)
    sp = ragged_set()
    sp64 = [s for s in sp]
    sp32 = [s.astype(np.float32) for s in sp if np.max(np.abs(s)) < 1e20]     # 1e30 is not a float32
    mixed = [sp64[0], sp32[1], sp64[4], sp32[3]]
    for group in (sp64, sp32, mixed):
        got = P.clean_speech_VAD_many(group, **kw)
        assert len(got) == len(group)
        for g, s in zip(got, group):
            want = P.clean_speech_VAD(s, **kw)
            assert g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want)


def test_ibm_many_equals_the_single_calls_c_and_fortran_order():
    rng = np.random.default_rng(5)
    Ss = []
    for rows, cols in [(513, 1), (513, 200), (7, 33), (513, 3751)]:
        S = ((rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols))) * np.exp(3 * rng.standard_normal((rows, cols))))
        Ss.append(S.astype(np.complex64))
    sp = [speechlike(20000, 21), speechlike(80000, 22)]
    Ss += [stft(s, **dict(KW, center=False)) for s in sp]            # Fortran-ordered, as the drop-in stft returns it
    assert Ss[-1].flags.f_contiguous and not Ss[-1].flags.c_contiguous
    Ss += [np.asfortranarray(Ss[1]), np.ascontiguousarray(Ss[-1])]
    for eps, thr in [(1e-8, 50), (1e-6, 30)]:
        got = P.clean_speech_IBM_many(Ss, eps=eps, ibm_threshold=thr)
        for g, S in zip(got, Ss):
            want = P.clean_speech_IBM(S, eps=eps, ibm_threshold=thr)
            assert g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want)


@pytest.mark.parametrize("center,wlen", [(True, 50e-3), (False, 64e-3)])
def test_noise_robust_many_gates_in_the_kernel(center, wlen):
    kw = dict(fs=16e3, wlen_sec=wlen, hop_percent=0.25, center=center, pad_mode="reflect", pad_at_end=True)
    sp = [speechlike(n, 30 + n % 97) for n in (1500, 16000, 48000, 80123)]
    sp[2][:20000] = 0.0
    Ss = [stft(s, win="hann", **kw) for s in sp]
    Ss[1] = np.ascontiguousarray(Ss[1])
    got = P.noise_robust_clean_speech_IBM_many(sp, Ss, vad_threshold=1.5, eps=1e-8, ibm_threshold=40, **kw)
    for g, s, S in zip(got, sp, Ss):
        want = P.noise_robust_clean_speech_IBM(s, S, vad_threshold=1.5, eps=1e-8, ibm_threshold=40, **kw)
        assert g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want)
    # a direct gate of arbitrary values (not 0 / 1): the kernel's column index g0 + i % cols
    S = Ss[3]
    gate = np.random.default_rng(2).random(S.shape[1] + 9).astype(np.float32)
    m = T.ibm_labels_batch(torch.from_numpy(np.ascontiguousarray(S).ravel()), [0], [S.size], [S.shape[1]], 1e-8, 40,
                           torch.from_numpy(gate).cuda(), [9]).cpu().numpy().reshape(S.shape)
    assert np.array_equal(m, P.clean_speech_IBM(S, eps=1e-8, ibm_threshold=40) * gate[None, 9:])


@pytest.mark.parametrize("U", [1, 2, 256])
def test_scale(U):
    rng = np.random.default_rng(U)
    speeches = [speechlike(int(n), 100 + u) for u, n in enumerate(rng.integers(4 * 16000, 6 * 16000, U))]
    for labels in ("vad_labels", "ibm_labels"):
        fb = T.utterances_to_frames(speeches, labels)
        check_against_single(speeches, fb, labels)


def test_past_2_gib_of_complex_frames():
    U = 1700
    lengths = [80000 + 37 * (u % 7) for u in range(U)]
    base = np.random.default_rng(0).standard_normal(max(lengths) + U)
    speeches = [base[u:u + n] * (0.5 + (u % 5)) for u, n in enumerate(lengths)]
    fb = T.utterances_to_frames(speeches, "ibm_labels")
    assert sum(fb.counts) * 513 * 8 > 2 ** 31
    check = sorted(set([0, U - 1] + np.random.default_rng(1).choice(U, 30, replace=False).tolist()))
    assert len(check) >= 32 - 1
    check_against_single(speeches, fb, "ibm_labels", which=check)
    del fb
    torch.cuda.empty_cache()


def test_all_zero_utterance_is_named():
    sp = [speechlike(20000, 1), np.zeros(20000), speechlike(30000, 2), np.zeros(5000)]
    with pytest.raises(ValueError, match="utterance 1 is all zeros.*1 more"):
        T.utterances_to_frames(sp)


def test_deterministic_and_stream_independent():
    speeches = ragged_set()[:7]
    for labels in ("vad_labels", "ibm_labels"):
        a = T.utterances_to_frames(speeches, labels)
        b = T.utterances_to_frames(speeches, labels)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = T.utterances_to_frames(speeches, labels)
        s.synchronize()
        for o in (b, c):
            assert torch.equal(a.X, o.X) and torch.equal(a.Y, o.Y) and a.counts == o.counts


@pytest.mark.parametrize("labels", ["vad_labels", "ibm_labels"])
def test_device_frames_from_rows(labels):
    fb = T.utterances_to_frames(ragged_set()[:6], labels)
    d1 = DeviceFrames.from_rows(fb.X, fb.Y)
    d2 = DeviceFrames(fb.X.t(), fb.Y.t())
    assert d1.x.data_ptr() == fb.X.data_ptr()                         # adopted, not copied
    assert same(d1.x, d2.x) and same(d1.y, d2.y) and len(d1) == len(d2)
    g1 = torch.Generator(device="cuda").manual_seed(3)
    g2 = torch.Generator(device="cuda").manual_seed(3)
    for (x1, y1), (x2, y2) in zip(d1.batches(64, generator=g1), d2.batches(64, generator=g2)):
        assert same(x1, x2) and same(y1, y2)
    d3 = DeviceFrames.from_rows(fb.X)
    assert d3.y is None and same(d3.x, d2.x)
    with pytest.raises(ValueError):
        DeviceFrames.from_rows(fb.X, fb.Y[:-1])

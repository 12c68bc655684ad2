"""The batched intelligibility scorer on the MI355X (dvae_estoi_batch; metrics.stoi_batch / estoi_batch, McemBatch.estoi): every
utterance against the float64 restatement tests/estoi_ref.py -- the score, the three counts of `info` exactly, the third-octave
bands of the debug output per element (so that a failure names its stage) -- bit-identity across runs and batches, bad table
entries, sentinel-filled outputs, packed buffers past 2^31 bytes.

Bounds are derived, not tuned: tests/estoi_bounds.py states them and evaluates them on each utterance's own intermediates (for these
inputs 1e-12 ... 1e-9 on d; a wrong frame rule or band edge moves d by 1e-3).  The silent-frame mask is a discontinuity: every
comparison first asserts, from the restatement, that no non-zero frame of x lies within 1e-6 dB of the threshold.
Every check prints its figures before it asserts (got - expected, bound; the worst per batch).
"""
import importlib
import multiprocessing

import numpy as np
import pytest
import torch

import estoi_bounds as EB
import estoi_ref as R

pytestmark = pytest.mark.gpu
M = importlib.import_module("disentangled-vae_amd.metrics")
H = importlib.import_module("disentangled-vae_amd.stft")
N = importlib.import_module("disentangled-vae_amd.native")

_pool = None


def evaluate(cases, fs):
    """estoi_bounds.evaluate of every (x, y) in worker processes that never touch the GPU (numpy only)."""
    global _pool
    if len(cases) <= 2:
        return [EB.evaluate((x, y, fs)) for x, y in cases]
    if _pool is None:
        _pool = multiprocessing.get_context("spawn").Pool(14)
    return _pool.map(EB.evaluate, [(x, y, fs) for x, y in cases], chunksize=1)


def teardown_module(module):
    global _pool
    if _pool is not None:
        _pool.close()
        _pool.join()
        _pool = None


def speech(n, seed, fs=16000, on=0.6):
    """Speech-like: 50 ms on / off white noise times a 220 Hz sine, plus a weak floor so that pauses are quiet, not digital zero."""
    rng = np.random.default_rng(seed)
    hold = fs // 20
    env = np.repeat((rng.random(n // hold + 1) < on).astype(np.float64), hold)[:n]
    return 0.3 * env * rng.standard_normal(n) * np.sin(2 * np.pi * 220 * np.arange(n) / fs + rng.random()) + 1e-4 * rng.standard_normal(n)


def pair(n, seed, fs=16000, snr_db=5.0):
    """(clean float64, estimate float32 held as float64): the estimate is what a float32 device buffer holds."""
    s = speech(n, seed, fs)
    rng = np.random.default_rng(seed + 7919)
    y = 0.8 * s + rng.standard_normal(n) * np.sqrt(np.mean(s * s)) * 10 ** (-snr_db / 20)
    return s, y.astype(np.float32).astype(np.float64)


def special_cases(fs):
    """Long silences, a leading and a trailing all-zero stretch, a clipped loud estimate (STOI's min is active), an utterance under
    30 frames, and a plain one."""
    n = 2 * fs
    s, y = pair(n, 1, fs)
    gaps = s.copy()
    gaps[n // 5:2 * n // 5] *= 1e-4                                                           # 0.4 s some 80 dB down: removed
    gaps[3 * n // 5:7 * n // 10] = 0.0                                                        # 0.2 s of digital silence
    lead = s.copy(); lead[:n // 4] = 0.0
    trail = s.copy(); trail[-n // 3:] = 0.0
    loud = np.clip(6.0 * y, -0.5, 0.5).astype(np.float32).astype(np.float64)
    short_s, short_y = pair(fs * 3 // 10, 2, fs)
    return [(gaps, y), (lead, y), (trail, y), (s, loud), (short_s, short_y), pair(int(1.37 * fs), 3, fs)]


def score(cases, fs, extended, dtypes=(np.float64, np.float32), trim=0):
    """-> d, info, tob (numpy) and the tables, from packed NaN-guarded buffers at unaligned offsets."""
    rng = np.random.default_rng(len(cases))
    bufs, views = [], []
    for k, dt in enumerate(dtypes):
        offs, pos = [], int(rng.integers(1, 37))
        for c in cases:
            offs.append(pos)
            pos += len(c[k]) + int(rng.integers(1, 37))
        buf = np.full(pos, np.nan, dt)
        for c, o in zip(cases, offs):
            buf[o:o + len(c[k])] = c[k]
        bufs.append(torch.from_numpy(buf).cuda())
        views.append((offs, [len(c[k]) for c in cases]))
    t = M.stoi_tables(views, [b.numel() for b in bufs], fs, trim)
    d, info, tob = M.stoi_packed(bufs, t, extended, return_info=True, return_tob=True)
    return d.cpu().numpy(), info.cpu().numpy(), tob.cpu().numpy(), t


def check(cases, refs, got, extended, what=""):
    d, info, tob, t = got
    f0 = np.concatenate([[0], np.cumsum(t["frames"])])
    key = "estoi" if extended else "stoi"
    worst = 0.0
    for u, ev in enumerate(refs):
        assert ev["clearance_db"] > EB.MASK_CLEAR_DB, (what, u, "a frame at the silent-frame threshold: not a valid test input")
        assert tuple(int(v) for v in info[u]) == tuple(ev["info"]), (what, u, info[u], ev["info"])            # exactly
        Mf = ev["tob_x"].shape[0]
        for name, sig in (("tob_x", 0), ("tob_y", 1)):
            rows = tob[sig, f0[u]:f0[u] + Mf]
            err = np.abs(rows - ev[name])
            if Mf:
                print(what, u, name, "worst error / bound", float(np.max(err / ev["E_" + name])), "worst relative to the largest band", float(err.max() / ev[name].max()))
            assert np.all(err <= ev["E_" + name]), (what, u, name)
            assert np.isnan(tob[sig, f0[u] + Mf:f0[u + 1]]).all(), (what, u, "rows past the last spectral frame were written")
        print(what, u, key, "got - expected", d[u] - ev[key], "bound", ev[key + "_bound"], "value", ev[key])
        assert abs(d[u] - ev[key]) <= ev[key + "_bound"], (what, u, key)
        worst = max(worst, abs(d[u] - ev[key]))
    print(what, key, "worst |device - restatement|", worst)


# ---- every stage, at three sampling rates -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", [16000, 10000, 8000])
def test_special_signals_at_three_rates(fs):
    cases = special_cases(fs)
    refs = evaluate(cases, fs)
    assert refs[4]["info"][2] == 0 and refs[4]["estoi"] == 1e-5                                # the short one, among normal ones
    assert refs[0]["info"][1] < R.frames_silent(refs[0]["info"][0]) - 30                       # the silences are removed
    for extended in (True, False):
        check(cases, refs, score(cases, fs, extended), extended, f"fs {fs}")
    # both buffers float64, and both float32 (the clean speech rounded first)
    check(cases, refs, score(cases, fs, True, (np.float64, np.float64)), True, f"fs {fs} f64-f64")
    c32 = [(x.astype(np.float32).astype(np.float64), y) for x, y in cases]
    check(c32, evaluate(c32, fs), score(c32, fs, False, (np.float32, np.float32)), False, f"fs {fs} f32-f32")


def test_clipped_estimate_activates_the_clip():
    s, loud = special_cases(16000)[3]
    st = R.stages(s, loud, 16000)
    X, Y = st["tob_x"][:30].T, st["tob_y"][:30].T
    alpha = np.linalg.norm(X, axis=1, keepdims=True) / (np.linalg.norm(Y, axis=1, keepdims=True) + R.EPS)
    assert np.any(alpha * Y > X * R.CLIP)                                                       # min() picks the clipped branch somewhere


# ---- ragged batches of 4 - 6 s ---------------------------------------------------------------------------------------------------------

_batch = {}


def ragged(U):
    if U not in _batch:
        rng = np.random.default_rng(U)
        cases = [pair(int(n), 100 * U + i) for i, n in enumerate(rng.integers(4 * 16000, 6 * 16000, U))]
        _batch[U] = (cases, evaluate(cases, 16000))
    return _batch[U]


@pytest.mark.parametrize("U", [1, 25, 256])
def test_ragged_batches(U):
    cases, refs = ragged(U)
    check(cases, refs, score(cases, 16000, True), True, f"U {U}")                               # float64 references, float32 estimates
    check(cases, refs, score(cases, 16000, False), False, f"U {U}")
    # the public functions on lists: float64 clean speech, float32 estimates (mixed), on the host and on the device
    x = [c[0] for c in cases]
    y = [c[1].astype(np.float32) for c in cases]
    d, info = M.estoi_batch(x, y, 16000, return_info=True)
    assert d.shape == (U,) and d.dtype == torch.float64 and d.is_cuda and info.shape == (U, 3) and info.dtype == torch.int64
    d2 = M.stoi_batch([torch.from_numpy(a).cuda() for a in x], [torch.from_numpy(a).cuda() for a in y], 16000, extended=True)
    assert torch.equal(d, d2)
    for u, ev in enumerate(refs):
        assert abs(float(d[u]) - ev["estoi"]) <= ev["estoi_bound"] and tuple(info[u].tolist()) == tuple(ev["info"]), u
    st = M.stoi_batch(x, y, 16000).cpu().numpy()                                                # pystoi's default: STOI
    assert all(abs(st[u] - ev["stoi"]) <= ev["stoi_bound"] for u, ev in enumerate(refs))


def test_alone_and_inside_256_utterances_and_twice():
    cases, _ = ragged(256)
    x, y = [c[0] for c in cases], [c[1].astype(np.float32) for c in cases]
    for extended in (True, False):
        d1, i1 = M.stoi_batch(x, y, 16000, extended, return_info=True)
        d2, i2 = M.stoi_batch(x, y, 16000, extended, return_info=True)
        assert torch.equal(d1, d2) and torch.equal(i1, i2)
        for u in (0, 17, 100, 255):
            da, ia = M.stoi_batch([x[u]], [y[u]], 16000, extended, return_info=True)
            assert torch.equal(da[0], d1[u]) and torch.equal(ia[0], i1[u]), u


def test_trim_scores_the_inner_samples():
    cases = [pair(n, 50 + i) for i, n in enumerate((40000, 33333, 6500))]
    x, y = [c[0] for c in cases], [c[1].astype(np.float32) for c in cases]
    got, info = M.estoi_batch(x, y, 16000, trim=800, return_info=True)
    cut = [(c[0][800:-800], c[1][800:-800]) for c in cases]
    lists = M.estoi_batch([c[0] for c in cut], [c[1].astype(np.float32) for c in cut], 16000)
    assert torch.equal(got, lists)                                                              # offsets moved == arrays cut
    refs = evaluate(cut, 16000)
    for u, ev in enumerate(refs):
        assert ev["clearance_db"] > EB.MASK_CLEAR_DB
        print("trimmed", u, float(got[u]) - ev["estoi"], ev["estoi_bound"])
        assert abs(float(got[u]) - ev["estoi"]) <= ev["estoi_bound"] and tuple(info[u].tolist()) == tuple(ev["info"])
    assert refs[2]["info"][2] == 0 and float(got[2]) == 1e-5                                    # (6500 - 1600) 5 / 8 = 3063 samples: 22 frames


# ---- the table is rechecked on the device ---------------------------------------------------------------------------------------------

def packed(cases, fs=16000):
    xb = torch.from_numpy(np.concatenate([c[0] for c in cases])).cuda()
    yb = torch.from_numpy(np.concatenate([c[1] for c in cases]).astype(np.float32)).cuda()
    lens = [len(c[0]) for c in cases]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [xb, yb], M.stoi_tables([(offs, lens), (offs, lens)], [xb.numel(), yb.numel()], fs)


def test_a_bad_table_entry_leaves_nan_and_spares_the_others():
    cases = [pair(n, 70 + i) for i, n in enumerate((30000, 9000, 41000))]
    bufs, t = packed(cases)
    U, tab = 3, t["table"]
    good, ginfo = M.stoi_packed(bufs, t, True, return_info=True)
    assert torch.isfinite(good).all()
    x0, y0, ln, r0, f0 = (3 * (U + 1) + k * U for k in range(5))
    for entry, value, row in ((y0 + 1, bufs[1].numel() - 100, 1),        # utterance 1 of y: 9000 samples from 100 before the end
                              (x0 + 0, -1, 0),                            # a negative offset
                              (ln + 2, 41000 + 4096, 2),                  # a length that disagrees with the item counts (and leaves the buffer)
                              (r0 + 1, t["n_res"] - 10, 1),               # resampled samples past the workspace
                              (f0 + 2, t["n_frames"], 2),                 # frames past the workspace
                              (2 * (U + 1) + 1, int(tab[2 * (U + 1) + 1]) + 1, None)):   # a segment-item prefix off by one: utterances 0 and 1
        bad = tab.copy()
        bad[entry] = value
        d, info = M.stoi_packed(bufs, t, True, return_info=True, table=bad)
        rows = [row] if row is not None else [0, 1]
        keep = [u for u in range(U) if u not in rows]
        assert torch.isnan(d[rows]).all() and bool((info[rows] == -1).all()), (entry, d)
        assert torch.equal(d[keep], good[keep]) and torch.equal(info[keep], ginfo[keep]), (entry, d)


def test_into_poisoned_outputs_with_guard_rows():
    cases = [pair(n, 80 + i) for i, n in enumerate((20000, 4000, 26000))]
    bufs, t = packed(cases)
    U = 3
    want, winfo = M.stoi_packed(bufs, t, False, return_info=True)
    lib = N.load()
    n_items = [int(t["table"][c * (U + 1) + U]) for c in range(3)]
    d = torch.full((U + 2,), float("nan"), dtype=torch.float64, device="cuda")
    info = torch.full((U + 2, 3), -7, dtype=torch.int64, device="cuda")
    ws = torch.full((lib.dvae_estoi_workspace_bytes(t["n_res"], t["n_frames"], n_items[2], U) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    tab = torch.from_numpy(t["table"]).cuda()
    taps, window, bands = (torch.from_numpy(t[k]).cuda() for k in ("taps", "window", "bands"))
    N.check(lib.dvae_estoi_batch(N.ptr(bufs[0]), bufs[0].numel(), 1, N.ptr(bufs[1]), bufs[1].numel(), 0, U, N.ptr(tab), n_items[0], n_items[1],
                                 n_items[2], t["n_res"], t["n_frames"], N.ptr(taps), t["p"], t["q"], t["L"], N.ptr(window), N.ptr(bands), 0,
                                 N.ptr(d[1:]), N.ptr(info[1:]), None, N.ptr(ws), N.stream()), "dvae_estoi_batch")
    assert torch.isnan(d[0]) and torch.isnan(d[-1]) and bool((info[0] == -7).all()) and bool((info[-1] == -7).all())
    assert torch.equal(d[1:-1], want) and torch.equal(info[1:-1], winfo)                        # a NaN-filled workspace leaks nowhere


# ---- past 2^31 bytes -------------------------------------------------------------------------------------------------------------------

def test_packed_buffers_past_two_gib():
    U, L = 6800, 80000                                                                          # 6 800 x 5 s: 2.18e9 bytes per float32 buffer
    assert U * L * 4 > 2 ** 31
    base = [pair(L, 900 + i) for i in range(4)]
    xs = torch.stack([torch.from_numpy(c[0].astype(np.float32)) for c in base]).cuda()
    ys = torch.stack([torch.from_numpy(c[1].astype(np.float32)) for c in base]).cuda()
    x = xs.repeat(U // 4, 1).reshape(-1)                                                        # utterance u holds base pair u % 4
    y = ys.repeat(U // 4, 1).reshape(-1)
    offs, lens = [u * L for u in range(U)], [L] * U
    d, info = M.estoi_batch(H.WaveBatch(x, offs, lens), H.WaveBatch(y, offs, lens), 16000, return_info=True)
    assert bool(torch.isfinite(d).all())
    refs = evaluate([(c[0].astype(np.float32).astype(np.float64), c[1]) for c in base], 16000)
    mark = 2 ** 31 // (4 * L)                                                                   # the utterance that straddles the 2^31-byte mark
    for u in (0, mark - 1, mark, mark + 1, U - 1):
        ev = refs[u % 4]
        assert ev["clearance_db"] > EB.MASK_CLEAR_DB
        print(u, float(d[u]) - ev["estoi"], ev["estoi_bound"])
        assert abs(float(d[u]) - ev["estoi"]) <= ev["estoi_bound"] and tuple(info[u].tolist()) == tuple(ev["info"]), u
    assert torch.equal(d[4:8], d[:4]) and torch.equal(d[-4:], d[:4])                            # the same bits wherever the utterance lies


# ---- McemBatch.estoi -------------------------------------------------------------------------------------------------------------------

def test_mcem_batch_estoi_equals_the_scores_of_its_waveforms():
    from packages.models.models import DeepGenerativeModel
    McemBatch = importlib.import_module("disentangled-vae_amd.mcem").McemBatch
    torch.manual_seed(0)
    vae = DeepGenerativeModel([513, 1, 16, [128, 128]], None).cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False
    lengths = [32000, 40000, 24691]
    clean = [speech(n, 40 + i) for i, n in enumerate(lengths)]
    rng = np.random.default_rng(4)
    waves = [s + 0.05 * rng.standard_normal(s.size) for s in clean]
    X = H.stft_batch(waves, center=False, pad_at_end=True)
    mb = McemBatch(vae, niter=2, nsamples_E_step=2, burnin_E_step=2, nsamples_WF=2, burnin_WF=2)
    mb.init_parameters(X, [np.ones((1, T), np.float32) for T in X.counts])
    mb.run()
    got = mb.estoi(clean, max_len=lengths, trim=800)
    assert got.shape == (3,) and got.is_cuda and got.dtype == torch.float64
    s_hat, _ = mb.enhance(max_len=lengths)
    assert torch.equal(got, M.estoi_batch(clean, s_hat, 16000, trim=800))
    assert torch.equal(mb.estoi(clean, max_len=lengths, extended=False), M.stoi_batch(clean, s_hat, 16000))
    cut = [(s[800:-800], w.astype(np.float64)[800:-800]) for s, w in zip(clean, s_hat.numpy())]
    for u, ev in enumerate(evaluate(cut, 16000)):
        assert ev["clearance_db"] > EB.MASK_CLEAR_DB
        print("utterance", u, float(got[u]) - ev["estoi"], ev["estoi_bound"], ev["estoi"])
        assert abs(float(got[u]) - ev["estoi"]) <= ev["estoi_bound"], u

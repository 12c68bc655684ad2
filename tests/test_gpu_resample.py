"""The batched resampler on the MI355X (dvae_resample_batch; resample.resample_batch; packages/dataset/qut_database.py): every output
sample against the numpy restatement (tests/estoi_ref.py::resample) within the derived bound (tests/estoi_bounds.py::resample_bound:
2 (nt + 2) u p sum |h| |x| per output, from the arithmetic, not fitted), an impulse bit for bit, bit identity across batches,
offsets and runs, the float32 forms, the strided read of an interleaved recording, a bad table entry through the C ABI, and the
drop-in preprocess_noise.

Ratios: 48 kHz -> 16 kHz (p 1, q 3), 44.1 kHz -> 16 kHz (160 / 441, the per-lane walk of the phase-major taps), 16 kHz -> 10 kHz (5 / 8),
8 kHz -> 16 kHz and 16 kHz -> 48 kHz (upsampling).  Lengths: 1, 2, q - 1, q, q + 1; one shorter than L / p input samples, so that the
zero extension of both edges lies under every output; one output short of, exactly at and one past a work item's run; three items
and a remainder.  Every test prints its figures before it asserts.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import estoi_bounds as EB
import estoi_ref as ER

pytestmark = pytest.mark.gpu
RS = importlib.import_module("disentangled-vae_amd.resample")
X = importlib.import_module("disentangled-vae_amd.mix")
N = importlib.import_module("disentangled-vae_amd.native")
from packages.dataset import qut_database as Q

RATES = [(48000, 16000), (44100, 16000), (16000, 10000), (8000, 16000), (16000, 48000)]
IDS = [f"{a}to{b}" for a, b in RATES]


def shortest_with(n_out, p, q):
    """The shortest signal with at least n_out output samples: ceil(n p / q) >= n_out (equal when p < q)."""
    return (n_out - 1) * q // p + 1


def longest_with(n_out, p, q):
    """The longest signal with at most n_out output samples: ceil(n p / q) <= n_out."""
    return n_out * q // p


def run_lengths(run, p, q):
    """Signals that end just short of, exactly at and just past a work item's run, and one of three items and a remainder.  When
    upsampling the output lengths are multiples of p: the nearest ones on either side of the run (a multiple of 64 p) are taken."""
    return [longest_with(run - 1, p, q), longest_with(run, p, q), shortest_with(run + 1, p, q), shortest_with(3 * run + 37, p, q)]


@functools.lru_cache(maxsize=None)
def case(rates):
    """Taps, signals of the lengths of the module's docstring, the restatement and the bound of each: computed once per ratio."""
    taps = RS.resample_taps(*rates)
    h, p, q, L = taps
    run = RS.resample_run(p, q, L)
    lengths = [1, 2, max(q - 1, 1), q, q + 1, max(L // p - 1, 1)] + run_lengths(run, p, q)
    rng = np.random.default_rng(1000 + p * 7 + q)
    xs = [rng.standard_normal(n) for n in lengths]
    for x in xs:
        x.setflags(write=False)
    ref = [ER.resample(x, None, taps) for x in xs]
    bound = [EB.resample_bound(x, taps) for x in xs]
    return {"taps": taps, "run": run, "lengths": lengths, "x": xs, "ref": ref, "bound": bound}


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                                        b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


# ---- 1: against the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_every_sample_within_the_derived_bound_of_the_restatement(rates):
    c = case(rates)
    h, p, q, L = c["taps"]
    got = RS.resample_batch(c["x"], *rates).numpy()
    assert len(got) == len(c["x"])
    assert c["lengths"][-4:] == run_lengths(c["run"], p, q)
    for u, (g, ref, bound, n) in enumerate(zip(got, c["ref"], c["bound"], c["lengths"])):
        assert g.dtype == np.float64 and g.shape == ref.shape == (-(-n * p // q),), (u, n)
        err = np.abs(g - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
        print(f"{rates} n {n}: {g.size} outputs, max |err| {err.max():.3e}, max bound {bound.max():.3e}, worst err / bound {worst:.3f}")
        assert np.all(err <= bound), (u, n, float(err.max()))
    short, at, past, three = [g.size for g in got[-4:]]
    step = max(-(-p // q), 1)                                                       # output lengths come in steps of ceil(p / q)
    assert c["run"] - step <= short < c["run"] == at < past <= c["run"] + step and 3 * c["run"] + 37 <= three < 4 * c["run"]


# ---- 2: an impulse, bit for bit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", [(48000, 16000), (16000, 10000), (44100, 16000)], ids=["p1", "p5", "p160"])
def test_an_impulse_returns_the_taps_of_its_phase_exactly(rates):
    h, p, q, L = RS.resample_taps(*rates)
    assert p in (1, 5, 160)
    n = 3200
    places = [0, n - 1, n // 2 + 3]
    xs = []
    for i0 in places:
        x = np.zeros(n)
        x[i0] = 1.0
        xs.append(x)
    got = RS.resample_batch(xs, *rates).numpy()
    n_out = -(-n * p // q)
    assert n_out > 3 * RS.resample_run(p, q, L)                                     # more than three work items
    for i0, g in zip(places, got):
        j = np.arange(n_out, dtype=np.int64) * q - i0 * p + L
        inside = (j >= 0) & (j <= 2 * L)
        want = np.where(inside, p * h[np.clip(j, 0, 2 * L)], 0.0)
        print(f"{rates} impulse at {i0}: {int(inside.sum())} outputs under the filter, {int((g != want).sum())} differ")
        assert inside.any() and g.shape == want.shape and np.array_equal(g, want), i0


# ---- 3: bit identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_alone_in_a_batch_permuted_and_twice_the_same_bits(rates):
    c = case(rates)
    batch = RS.resample_batch(c["x"], *rates).numpy()
    again = RS.resample_batch(c["x"], *rates).numpy()
    order = [7, 0, 9, 3, 5, 1, 8, 2, 6, 4]
    perm = RS.resample_batch([c["x"][u] for u in order], *rates).numpy()
    for u in range(len(c["x"])):
        assert bits(batch[u], again[u]), u
        assert bits(batch[u], perm[order.index(u)]), u
    for u in (0, 4, 5, 7, 9):
        alone = RS.resample_batch([c["x"][u]], *rates).numpy()[0]
        assert bits(batch[u], alone), u


@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000), (16000, 48000)], ids=["p1", "p160", "up3"])
def test_odd_offsets_of_input_and_output_change_no_bit(rates):
    c = case(rates)
    h, p, q, L = c["taps"]
    pick = [9, 4, 8]
    xs = [c["x"][u] for u in pick]
    want = RS.resample_batch(xs, *rates).numpy()
    gaps = [3, 1, 7]
    x0, parts, o = [], [], 0
    for g, x in zip(gaps, xs):
        parts += [np.full(g, 1e30), x]
        x0.append(o + g)
        o += g + x.size
    buf = torch.from_numpy(np.concatenate(parts)).cuda()
    out_len = [w.size for w in want]
    y0 = [5, 5 + out_len[0] + 1, 5 + out_len[0] + 1 + out_len[1] + 11]
    n_y = y0[2] + out_len[2] + 9
    t = RS.resample_tables((x0, [x.size for x in xs], buf.numel()), p, q, L, out_layout=(y0, n_y))
    y = torch.full((n_y,), 7.0, dtype=torch.float64, device="cuda")
    RS.resample_packed(buf, t["table"], h, p, q, n_out=n_y, out=y)
    y = y.cpu().numpy()
    written = np.zeros(n_y, bool)
    for o, m, w in zip(y0, out_len, want):
        assert bits(y[o:o + m], w)
        written[o:o + m] = True
    assert np.all(y[~written] == 7.0)                                              # nothing outside the output ranges is touched


# ---- 4: dtypes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000), (8000, 16000)], ids=["p1", "p160", "up2"])
def test_float32_input_and_output(rates):
    c = case(rates)
    x32 = [x.astype(np.float32) for x in c["x"]]
    from32 = RS.resample_batch(x32, *rates).numpy()
    from64 = RS.resample_batch([x.astype(np.float64) for x in x32], *rates).numpy()
    out32 = RS.resample_batch(x32, *rates, out_dtype=torch.float32).numpy()
    for a, b, o in zip(from32, from64, out32):
        assert bits(a, b)                                                           # a float32 sample converts to double exactly
        assert o.dtype == np.float32 and bits(o, a.astype(np.float32))              # the double result rounded once
    dev = RS.resample_batch([torch.from_numpy(x).cuda() for x in x32], *rates).numpy()           # device tensors are taken as they are
    assert all(bits(a, b) for a, b in zip(dev, from32))


# ---- 5: stride ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000)], ids=["p1", "p160"])
def test_channels_of_an_interleaved_recording_equal_their_contiguous_copies(rates):
    c = case(rates)
    stereo = [np.stack([c["x"][u], c["x"][u][::-1]], axis=1) for u in (9, 4, 0)]
    for ch in (0, 1):
        got = RS.resample_batch(stereo, *rates, channel=ch).numpy()
        want = RS.resample_batch([np.ascontiguousarray(s[:, ch]) for s in stereo], *rates).numpy()
        assert all(bits(a, b) for a, b in zip(got, want)), ch
    f32 = RS.resample_batch([torch.from_numpy(s.astype(np.float32)).cuda() for s in stereo], *rates, channel=1).numpy()
    want = RS.resample_batch([np.ascontiguousarray(s[:, 1]).astype(np.float32) for s in stereo], *rates).numpy()
    assert all(bits(a, b) for a, b in zip(f32, want))


# ---- 6: a bad table entry, through the C ABI ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000)], ids=["p1", "p160"])
def test_a_bad_table_entry_drops_that_signal_and_nothing_else(rates):
    """The kernel rechecks the table: a signal whose entry leaves a buffer or disagrees with the item counts (the host check
    bypassed) is dropped; nothing out of range is read or written."""
    lib = N.load()
    c = case(rates)
    h, p, q, L = c["taps"]
    xs = [c["x"][9], c["x"][4], c["x"][8]]
    lengths = [x.size for x in xs]
    buf = torch.from_numpy(np.concatenate(xs)).cuda()
    x0 = [0, lengths[0], lengths[0] + lengths[1]]
    t = RS.resample_tables((x0, lengths, buf.numel()), p, q, L)
    tab, U, n_out, y0, m = t["table"], 3, t["n_out"], t["out0"], t["out_len"]
    taps_dev = torch.from_numpy(RS.phase_major(h, p).reshape(-1)).cuda()
    pad = 64

    def call(table, n_items=None, stride=1):
        y = torch.full((pad + n_out + pad,), 7.0, dtype=torch.float64, device="cuda")
        body = y[pad:pad + n_out]
        tab_dev = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        rc = lib.dvae_resample_batch(N.ptr(buf), buf.numel(), 1, stride, N.ptr(body), n_out, 1, U, N.ptr(tab_dev),
                                     int(table[U]) if n_items is None else n_items, N.ptr(taps_dev), p, q, L, N.stream())
        torch.cuda.synchronize()
        return rc, y.cpu().numpy()

    rc, good = call(tab)
    assert rc == 0 and np.all(good[:pad] == 7.0) and np.all(good[pad + n_out:] == 7.0)
    want = RS.resample_batch(xs, *rates).numpy()
    for u in range(U):
        assert bits(good[pad + y0[u]:pad + y0[u] + m[u]], want[u])
    one = slice(pad + int(y0[1]), pad + int(y0[1] + m[1]))
    entries = {"x0 past the buffer": (U + 1 + 1, buf.numel()), "x0 negative": (U + 1 + 1, -1),
               "a length that leaves the buffer": (2 * U + 1 + 1, buf.numel() - x0[1] + 1), "a length of zero": (2 * U + 1 + 1, 0),
               "a length with another item count": (2 * U + 1 + 1, lengths[1] + 2 * c["run"] * q // p),
               "y0 past the buffer": (3 * U + 1 + 1, n_out), "y0 that leaves the buffer": (3 * U + 1 + 1, n_out - int(m[1]) + 1),
               "y0 negative": (3 * U + 1 + 1, -3)}
    for name, (pos, value) in entries.items():
        bad = tab.copy()
        bad[pos] = value
        rc, y = call(bad)
        assert rc == 0, name
        assert np.all(y[one] == 7.0), name                                          # signal 1: dropped, its outputs unwritten
        keep = np.ones(y.size, bool)
        keep[one] = False
        assert np.array_equal(y[keep], good[keep]), name                            # the neighbours and the canaries as they were
    bad = tab.copy()                                                                # a wrong item count: signal 1 claims one item more
    bad[2:U + 1] += 1
    rc, y = call(bad, n_items=int(tab[U]))
    assert rc == 0 and np.all(y[one] == 7.0)
    assert np.all(y[:pad] == 7.0) and np.all(y[pad + n_out:] == 7.0) and bits(y[pad:pad + m[0]], want[0])
    # host-detectable misuse: refused by name, nothing launched
    for kw in (dict(n_items=0), dict(n_items=U - 1), dict(stride=0)):
        rc, y = call(tab, **kw)
        assert rc != 0 and b"resample_batch" in lib.dvae_last_error(), kw
        assert np.all(y == 7.0)
    rc = lib.dvae_resample_batch(N.ptr(buf), buf.numel(), 1, 1, None, n_out, 1, U, None, 1, N.ptr(taps_dev), p, q, L, N.stream())
    assert rc != 0 and b"resample_batch" in lib.dvae_last_error()
    rc = lib.dvae_resample_batch(N.ptr(buf), buf.numel(), 1, 1, N.ptr(buf), n_out, 1, U, None, 1, N.ptr(taps_dev), p, p, L, N.stream())
    assert rc != 0 and b"resample_batch" in lib.dvae_last_error()


# ---- 7: the drop-in surface -----------------------------------------------------------------------------------------------------------

def test_preprocess_noise_is_resample_batch_of_the_first_channel():
    rng = np.random.default_rng(11)
    audio = 0.1 * rng.standard_normal((9600, 2))                                   # 0.2 s, two channels, 48 kHz
    got = Q.preprocess_noise(audio, 'cafe', 48000, 16000)
    want = RS.resample_batch([np.ascontiguousarray(audio[:, 0])], 48000, 16000).numpy()[0]
    assert isinstance(got, np.ndarray) and got.shape == (3200,) and bits(got, want)
    assert np.array_equal(Q.preprocess_noise(audio, 'home', 16000, 16000), audio[:, 0])


def test_preprocess_noise_cuts_the_car_recording_as_the_reference():
    rng = np.random.default_rng(12)
    fs_noise, fs = 48, 16                                                           # the cut is in minutes: low rates keep 45 min small
    audio = rng.standard_normal((fs_noise * 2700, 2))
    whole = Q.preprocess_noise(audio, 'street', fs_noise, fs)
    car = Q.preprocess_noise(audio, 'car', fs_noise, fs)
    assert whole.size == 43200 and int(1.5 * 60 * fs) == 1440 and int(43 * 60 * fs) == 41280
    assert bits(car, whole[1440:41280])
    many = Q.preprocess_noise_many({"street": audio, "car": audio}, fs_noise, fs)
    assert many["car"].is_cuda and bits(many["car"].cpu().numpy(), car) and bits(many["street"].cpu().numpy(), whole)


def test_preprocess_noise_many_feeds_the_mixer():
    rng = np.random.default_rng(13)
    raw = {"cafe": 0.1 * rng.standard_normal((60000, 2)), "home": 0.1 * rng.standard_normal((48000, 2))}
    banks = Q.preprocess_noise_many(raw, 48000, 16000)
    assert list(banks) == ["cafe", "home"] and [int(b.numel()) for b in banks.values()] == [20000, 16000]
    for k in raw:
        assert bits(banks[k].cpu().numpy(), Q.preprocess_noise(raw[k], k, 48000, 16000))
    speech = [0.3 * rng.standard_normal(4000), 0.3 * rng.standard_normal(5000)]
    mb = X.mix_at_snr_batch(speech, list(banks.values()), [0, 1], [100, 200], [0.0, 5.0])
    stats = mb.stats.cpu().numpy()
    print("achieved SNR", stats[:, 5])
    assert np.allclose(stats[:, 5], [0.0, 5.0], atol=1e-9)
    host = X.mix_at_snr_batch(speech, [b.cpu().numpy() for b in banks.values()], [0, 1], [100, 200], [0.0, 5.0])
    assert all(bits(a, b) for a, b in zip(mb.mixture.numpy(), host.mixture.numpy()))

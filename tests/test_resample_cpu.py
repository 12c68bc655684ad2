"""Host side of the batched resampler (disentangled-vae_amd/resample.py, packages/dataset/qut_database.py), no GPU: the taps, the
lengths and tables, the phase-major tap layout, the run of a work item against the library's own, the restatement
(tests/estoi_ref.py::resample) against scipy's resample_poly within the derived bound (tests/estoi_bounds.py::resample_bound), the
numpy path of preprocess_noise, and the refusals."""
import importlib

import numpy as np
import pytest
import torch

import estoi_bounds as EB
import estoi_ref as ER

RS = importlib.import_module("disentangled-vae_amd.resample")
M = importlib.import_module("disentangled-vae_amd.metrics")
N = importlib.import_module("disentangled-vae_amd.native")
from packages.dataset import qut_database as Q

RATES = [(48000, 16000), (44100, 16000), (16000, 10000), (8000, 16000), (16000, 48000)]
WANT = {(48000, 16000): (1, 3, 109), (44100, 16000): (160, 441, 15973), (16000, 10000): (5, 8, 290)}


@pytest.mark.parametrize("fs", [16000, 8000, 48000])
def test_taps_at_10_khz_are_the_bits_of_stoi_taps(fs):
    h, p, q, L = RS.resample_taps(fs, 10000)
    g, gp, gq, gL = M.stoi_taps(fs)
    assert (p, q, L) == (gp, gq, gL) and h.dtype == np.float64 and np.array_equal(h, g)


@pytest.mark.parametrize("rates", RATES)
def test_taps_ratio_and_length(rates):
    h, p, q, L = RS.resample_taps(*rates)
    assert p * rates[0] == q * rates[1] and np.gcd(p, q) == 1 and h.size == 2 * L + 1
    assert abs(h.sum() - 1.0) < 1e-12 and np.array_equal(h, h[::-1])
    if rates in WANT:
        assert (p, q, L) == WANT[rates]


@pytest.mark.parametrize("rates", RATES)
def test_phase_major_rows_are_the_taps_of_each_phase(rates):
    h, p, q, L = RS.resample_taps(*rates)
    hp = RS.phase_major(h, p)
    assert hp.shape == (p, 2 * L // p + 1)
    for j0 in range(p):
        row = h[j0::p]
        assert row.size == (2 * L - j0) // p + 1
        assert np.array_equal(hp[j0, :row.size], row) and not hp[j0, row.size:].any()


def test_phase_major_of_fewer_taps_than_phases():
    hp = RS.phase_major(np.array([1.0, 2.0, 3.0]), 5)
    assert hp.shape == (5, 1) and np.array_equal(hp[:, 0], [1.0, 2.0, 3.0, 0.0, 0.0])


@pytest.mark.parametrize("rates", RATES)
def test_run_fits_the_tile_and_equals_the_librarys(rates):
    _, p, q, L = RS.resample_taps(*rates)
    run = RS.resample_run(p, q, L)
    nt = 2 * L // p + 1
    assert run > 0 and run % 64 == 0 and run <= max(RS.RESAMPLE_MAX_RUN, 64 * p)
    assert -(-(run - 1) * q // p) + 1 + nt <= RS.RESAMPLE_SPAN
    if p <= RS.UNIFORM_P:
        assert run % (64 * p) == 0
    assert N.load().dvae_resample_run(p, q, L) == run


def test_run_of_what_does_not_fit_is_zero_on_both_sides():
    lib = N.load()
    for p, q, L in ((1, 40, 100), (1, 2, 700), (3, 2, 3000), (7, 5, 20), (320, 147, 16000), (17, 19, 400)):
        assert lib.dvae_resample_run(p, q, L) == RS.resample_run(p, q, L), (p, q, L)
    assert RS.resample_run(1, 40, 100) == 0 and RS.resample_run(1, 2, 700) == 0
    with pytest.raises(ValueError, match="a tile holds"):
        RS.resample_tables(([0], [100], 100), 1, 40, 100)


@pytest.mark.parametrize("rates", RATES)
def test_lengths_and_tables(rates):
    _, p, q, L = RS.resample_taps(*rates)
    run = RS.resample_run(p, q, L)
    lengths = np.array([1, 2, q - 1 if q > 1 else 1, q, q + 1, 5000, 3 * run * q // p + 7])
    x0 = np.concatenate([[0], np.cumsum(lengths)[:-1]]) * 2 + 1
    t = RS.resample_tables((x0, lengths, int(2 * lengths.sum())), p, q, L, stride=2)
    U = lengths.size
    want = np.array([-(-int(n) * p // q) for n in lengths])
    assert t["U"] == U and t["run"] == run and np.array_equal(t["out_len"], want)
    assert np.array_equal([ER.resample(np.zeros(int(n)), None, (np.ones(2 * L + 1), p, q, L)).size for n in lengths[:6]], want[:6])
    tab = t["table"]
    assert tab.dtype == np.int64 and tab.size == 4 * U + 1
    assert np.array_equal(np.diff(tab[:U + 1]), -(-want // run)) and tab[0] == 0 and tab[U] == t["n_items"]
    assert np.array_equal(tab[U + 1:2 * U + 1], x0) and np.array_equal(tab[2 * U + 1:3 * U + 1], lengths)
    y0 = tab[3 * U + 1:]
    assert np.all(y0 % 64 == 0) and np.all(y0[1:] >= y0[:-1] + want[:-1]) and t["n_out"] == y0[-1] + want[-1]
    own = RS.resample_tables((x0, lengths, int(2 * lengths.sum())), p, q, L, stride=2, out_layout=(y0 + 3, t["n_out"] + 3))
    assert np.array_equal(own["table"][3 * U + 1:], y0 + 3) and own["n_out"] == t["n_out"] + 3


def test_table_refusals_name_the_signal():
    _, p, q, L = RS.resample_taps(48000, 16000)
    with pytest.raises(ValueError, match="signal 1 is empty"):
        RS.resample_tables(([0, 10], [10, 0], 20), p, q, L)
    with pytest.raises(ValueError, match="signal 0 has .* more than 2\\^31"):
        RS.resample_tables(([0], [(1 << 31) + 1], 1 << 40), p, q, L)
    with pytest.raises(ValueError, match="signal 1 .* leaves its buffer"):
        RS.resample_tables(([0, 10], [10, 11], 20), p, q, L)
    with pytest.raises(ValueError, match="signal 0 .* leaves its buffer"):
        RS.resample_tables(([2], [10], 20), p, q, L, stride=2)
    with pytest.raises(ValueError, match="stride 0"):
        RS.resample_tables(([0], [10], 20), p, q, L, stride=0)
    with pytest.raises(ValueError, match="signals 0 and 1 overlap"):
        RS.resample_tables(([0, 30], [30, 30], 60), p, q, L, out_layout=([0, 9], 100))
    with pytest.raises(ValueError, match="signal 1 of the output"):
        RS.resample_tables(([0, 30], [30, 30], 60), p, q, L, out_layout=([0, 95], 100))


def test_batch_refusals_come_before_any_device_work():
    x = np.zeros(100)
    with pytest.raises(ValueError, match="fs_in == fs_out"):
        RS.resample_batch([x], 16000, 16000)
    with pytest.raises(ValueError, match="fs_in == fs_out"):
        RS.resample_taps(8000, 8000)
    with pytest.raises(ValueError, match="positive integer"):
        RS.resample_batch([x], 16000.0, 8000)
    with pytest.raises(ValueError, match="signal 1 is empty"):
        RS.resample_batch([x, np.zeros(0)], 48000, 16000)
    with pytest.raises(ValueError, match="signal 0 has 2 dimensions"):
        RS.resample_batch([np.zeros((10, 2))], 48000, 16000)
    with pytest.raises(ValueError, match="signal 0 has 1 dimensions"):
        RS.resample_batch([x], 48000, 16000, channel=0)
    with pytest.raises(ValueError, match="no channel 2"):
        RS.resample_batch([np.zeros((10, 2))], 48000, 16000, channel=2)
    with pytest.raises(ValueError, match="signal 1 has 3 channels"):
        RS.resample_batch([np.zeros((10, 2)), np.zeros((10, 3))], 48000, 16000, channel=0)
    with pytest.raises(TypeError, match="not floating point"):
        RS.resample_batch([np.zeros(10, np.int16)], 48000, 16000)
    with pytest.raises(ValueError, match="odd length"):
        RS.resample_batch([x], 48000, 16000, taps=np.ones(4))
    with pytest.raises(ValueError, match="needs a .* resampler"):
        RS.resample_batch([x], 99991, 16000)


def test_host_detectable_misuse_of_the_c_abi_is_refused_by_name():
    """No launch happens: every refusal precedes it (and this machine may have no GPU at all)."""
    lib = N.load()
    one = 8                                           # any non-null address: nothing is dereferenced before the refusal
    for args in ((None, 10, 1, 1, one, 10, 1, 1, one, 1, one, 1, 3, 109),          # null input
                 (one, 10, 1, 0, one * 2, 10, 1, 1, one, 1, one, 1, 3, 109),       # stride 0
                 (one, 10, 1, 1, one * 2, 10, 1, 1, one, 1, one, 3, 3, 109),       # p == q
                 (one, 10, 1, 1, one * 2, 10, 1, 1, one, 1, one, 1, 3, 0),         # L 0
                 (one, 10, 1, 1, one * 2, 10, 1, 1, one, 1, one, 1, 40, 100),      # the span does not fit the tile
                 (one, 10, 1, 1, one * 2, 10, 1, 0, one, 1, one, 1, 3, 109),       # U 0
                 (one, 10, 1, 1, one * 2, 10, 1, 2, one, 1, one, 1, 3, 109),       # fewer items than signals
                 (one, 10, 1, 1, one, 10, 1, 1, one, 1, one, 1, 3, 109)):          # the output is the input
        rc = lib.dvae_resample_batch(*args, None)
        assert rc != 0 and b"resample_batch" in lib.dvae_last_error(), args


def test_restatement_against_scipy_resample_poly_within_the_bound():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    worst = 0.0
    for rates in RATES:
        taps = RS.resample_taps(*rates)
        h, p, q, L = taps
        for n in (1, 2, q + 1, 257, 5000):
            x = rng.standard_normal(n)
            want = sig.resample_poly(x, p, q, window=h)
            got, bound = ER.resample(x, None, taps), EB.resample_bound(x, taps)
            assert got.shape == want.shape == (-(-n * p // q),)
            err = np.abs(got - want)
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (rates, n, float(err.max()))
    print(f"worst |restatement - resample_poly| / bound = {worst:.3f}")


@pytest.mark.parametrize("rates", RATES)
def test_numpy_path_is_the_restatement_within_the_bound(rates):
    taps = RS.resample_taps(*rates)
    h, p, q, L = taps
    rng = np.random.default_rng(6)
    for n in (1, q, 700, 3001):
        x = rng.standard_normal(n)
        got = RS.resample_numpy(x, h, p, q, block=257)
        want, bound = ER.resample(x, None, taps), EB.resample_bound(x, taps)
        assert got.shape == want.shape and np.all(np.abs(got - want) <= bound), (rates, n)


def test_preprocess_noise_numpy_path_first_channel_and_car_cut(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # the path of a machine without a GPU, wherever this runs
    rng = np.random.default_rng(7)
    fs_noise, fs = 48, 16                             # the car cut is in minutes: low rates keep 45 min of "audio" small
    audio = rng.standard_normal((fs_noise * 2700, 2))
    taps, p, q, _ = RS.resample_taps(fs_noise, fs)
    want = RS.resample_numpy(audio[:, 0], taps, p, q)
    got = Q.preprocess_noise(audio, 'cafe', fs_noise, fs)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    # 'car' keeps [int(1.5 * 60 * fs), int(43 * 60 * fs)) of the resampled recording: at fs = 16 "Hz", samples 1440 ... 41 280
    car = Q.preprocess_noise(audio, 'car', fs_noise, fs)
    assert int(1.5 * 60 * fs) == 1440 and int(43 * 60 * fs) == 41280
    assert np.array_equal(car, want[1440:41280]) and car.size == 41280 - 1440 < want.size - 1440


def test_preprocess_noise_at_the_same_rate_returns_the_first_channel():
    audio = np.random.default_rng(8).standard_normal((5000, 2))
    assert np.array_equal(Q.preprocess_noise(audio, 'home', 16000, 16000), audio[:, 0])
    car = Q.preprocess_noise(audio, 'car', 2, 2)                              # at 2 "Hz" the cut is [180, 5160)
    assert np.array_equal(car, audio[180:5160, 0])


def test_noise_listings_and_segment(tmp_path):
    root = tmp_path / "QUT-NOISE"
    for rel in ("QUT-NOISE/CAFE-CAFE-1.wav", "QUT-NOISE/CAFE-CAFE-2.wav", "QUT-NOISE/CAR-WINDOWNB-1.wav", "extra/STREET-CITY-1.wav",
                "QUT-NOISE/notes.txt"):
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"")
    got = Q.noise_list(str(root) + "/", "test")
    assert got == {"cafe": "QUT-NOISE/CAFE-CAFE-1.wav", "car": "QUT-NOISE/CAR-WINDOWNB-1.wav", "street": "extra/STREET-CITY-1.wav"}
    pre = tmp_path / "pre"
    (pre / "test").mkdir(parents=True)
    (pre / "test" / "cafe.wav").write_bytes(b"")
    (pre / "train").mkdir()
    (pre / "train" / "car.wav").write_bytes(b"")
    assert Q.noise_list_preprocessed(str(pre) + "/", "test") == {"cafe": str(pre / "test" / "cafe.wav")}
    np.random.seed(3)
    bank, speech = np.arange(1000.0), np.zeros(100)
    seg = Q.noise_segment({"cafe": bank}, "cafe", speech)
    np.random.seed(3)
    start = np.random.randint(900)
    assert np.array_equal(seg, bank[start:start + 100])

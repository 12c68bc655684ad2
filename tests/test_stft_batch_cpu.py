"""Host side of the ragged-batch STFT / ISTFT (no GPU): the planner's per-utterance decisions equal the single-signal ones, and
bad offset tables are refused before anything reaches the device."""
import importlib

import numpy as np
import pytest

H = importlib.import_module("disentangled-vae_amd.stft")

KW = dict(fs=16000, wlen_sec=64e-3, hop_percent=0.25)


def quirk_lengths(count=3):
    """Exact multiples of the hop that the reference's floating-point end-pad rule pads all the same."""
    out = [k * 256 for k in range(4, 4000) if H.needs_end_pad(k * 256, **KW)]
    assert len(out) >= count
    return out[:count]


def _single(n, center, pad_at_end=True):
    nfft, hop = H.sizes(KW["fs"], KW["wlen_sec"], KW["hop_percent"])
    e = pad_at_end and H.needs_end_pad(n, **KW)
    p = n + (hop if e else 0) + (2 * (nfft // 2) if center else 0)
    return int(e), p, H.frame_count(p, nfft, hop)


@pytest.mark.parametrize("center", [False, True])
def test_planner_matches_single_signal_decisions(center):
    q = quirk_lengths()
    lengths = q + [1024, 1025, 1279, 1280, 16000, 80000, 80123] + ([600, 700] if center else [])
    plan = H.plan_stft_batch(lengths, center=center, **KW)
    for u, n in enumerate(lengths):
        e, p, T = _single(n, center)
        assert (plan["end_pad"][u], plan["padded"][u], plan["frames"][u]) == (e, p, T), n
    assert plan["frame_off"][0] == 0 and np.array_equal(np.diff(plan["frame_off"]), plan["frames"])
    assert plan["x0"][0] == 0 and np.array_equal(np.diff(plan["x0"]), plan["padded"][:-1])
    assert all(plan["end_pad"][u] == 1 for u in range(len(q)))          # the quirk: these multiples of the hop ARE padded


def test_planner_one_frame_and_exact_window():
    plan = H.plan_stft_batch([1024, 1024 + 255], center=False, pad_at_end=False, **KW)
    assert plan["frames"].tolist() == [1, 1]
    plan = H.plan_stft_batch([1024], center=False, pad_at_end=True, **KW)
    assert plan["frames"].tolist() == [_single(1024, False)[2]]


def test_planner_rejects_short_signals():
    with pytest.raises(ValueError, match="too small"):
        H.plan_stft_batch([2048, 1000], center=False, pad_at_end=False, **KW)
    with pytest.raises(ValueError, match="no signals"):
        H.plan_stft_batch([], **KW)


def test_stft_tables_layout_and_checks():
    plan = H.plan_stft_batch([16000, 1024, 5000], center=False, pad_at_end=True, **KW)
    n = int(plan["padded"].sum())
    tab = H.stft_tables(plan["frames"], plan["x0"], plan["padded"], n, 4)
    U = 3
    items = -(-plan["frames"] // 4)
    assert tab.dtype == np.int64 and tab.size == 3 * U + 2
    assert tab[:U + 1].tolist() == [0] + np.cumsum(items).tolist()
    assert tab[U + 1:2 * U + 2].tolist() == plan["frame_off"].tolist()
    assert tab[2 * U + 2:].tolist() == plan["x0"].tolist()
    bad_x0 = plan["x0"].copy(); bad_x0[[1, 2]] = bad_x0[[2, 1]]
    with pytest.raises(ValueError, match="non-decreasing"):
        H.stft_tables(plan["frames"], bad_x0, plan["padded"], n, 4)
    with pytest.raises(ValueError, match="overlap|leave"):
        H.stft_tables(plan["frames"], plan["x0"], plan["padded"], n - 1, 4)
    with pytest.raises(ValueError, match="beyond the end"):
        H.stft_tables(plan["frames"] + np.array([0, 1, 0]), plan["x0"], plan["padded"], n, 4)
    with pytest.raises(ValueError, match="at least one frame"):
        H.stft_tables(np.array([0, 1, 1]), plan["x0"], plan["padded"], n, 4)


def test_istft_plan_truncation_matches_istft_numpy():
    nfft, hop = 1024, 256
    for center in (False, True):
        for T, ml in [(309, None), (309, 1000), (309, 79104), (309, 200000), (5, 0), (1, 300)]:
            nfr, lens, start = H.istft_plan([T], ml, nfft, hop, center)
            n_frames = T
            if ml:
                n_frames = min(T, int(np.ceil((ml + nfft if center else ml) / hop)))
            ntot = nfft + hop * (n_frames - 1)
            out_len = (ntot - 2 * (nfft // 2) if center else ntot) if ml is None else int(ml)
            assert (nfr[0], lens[0], start) == (n_frames, max(out_len, 0), nfft // 2 if center else 0), (T, ml, center)
    with pytest.raises(ValueError, match="max_len"):
        H.istft_plan([3, 4], [100], nfft, hop, False)


def test_istft_tables_checks():
    f0, nfr, y0, lens, gcol = [0, 10, 30], [10, 20, 5], [0, 2560, 8192], [2500, 5000, 2000], [0, 32, 64]
    tab = H.istft_tables(f0, nfr, y0, lens, gcol, 35, 10240, 96, 4)
    assert tab.size == 6 * 3 + 1 and tab[:4].tolist() == [0, 3, 8, 10]
    with pytest.raises(ValueError, match="non-decreasing"):
        H.istft_tables([0, 30, 10], nfr, y0, lens, gcol, 35, 10240, 96, 4)
    with pytest.raises(ValueError, match="frames overlap"):
        H.istft_tables([0, 5, 30], nfr, y0, lens, gcol, 35, 10240, 96, 4)
    with pytest.raises(ValueError, match="frames overlap"):
        H.istft_tables(f0, nfr, y0, lens, gcol, 34, 10240, 96, 4)
    with pytest.raises(ValueError, match="odd sample"):
        H.istft_tables(f0, nfr, [0, 2561, 8192], lens, gcol, 35, 10240, 96, 4)
    with pytest.raises(ValueError, match="outputs overlap"):
        H.istft_tables(f0, nfr, y0, lens, gcol, 35, 10000, 96, 4)
    with pytest.raises(ValueError, match="gain columns"):
        H.istft_tables(f0, nfr, y0, lens, [0, 32, 92], 35, 10240, 96, 4)
    H.istft_tables(f0, nfr, y0, lens, [0, 32, 92], 35, 10240, None, 4)      # no gain: the columns are unused


def test_batch_symbols_declared():
    N = importlib.import_module("disentangled-vae_amd.native")
    for name in ("dvae_stft_batch", "dvae_istft_batch", "dvae_mcem_spec_init"):
        assert name in N.SIGNATURES


def test_mcem_batch_refuses_a_zero_frame_utterance_before_any_launch():
    """An utterance without frames has no columns on McemBatch's frame axis (its W updates would form 0/0): init_parameters names it
    and raises before it touches the device."""
    M = importlib.import_module("disentangled-vae_amd.mcem")
    mb = M.McemBatch(vae=None, niter=1)
    X = [np.ones((513, 40), np.complex64), np.ones((513, 7), np.complex64), np.zeros((513, 0), np.complex64)]
    with pytest.raises(ValueError, match="utterance 2"):
        mb.init_parameters(X, [np.ones((1, x.shape[1]), np.float32) for x in X], device="cpu")

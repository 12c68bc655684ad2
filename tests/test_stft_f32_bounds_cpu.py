"""The bounds and bars of tests/stft_f32_ref.py on the CPU: the two correct float32 transforms (the numpy restatement of the kernels'
arithmetic and the host torch.stft / torch.istft) stay inside every bound on every signal the GPU tests use, the per-frame L2 margin
lies between their spread and a wrong transform, and restatements that are wrong by construction are rejected by the bar named for
them.  The wrong transforms are altered restatements, never kernels.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import stft_bounds as B
import stft_f32_ref as R

T_CPU = 3000
SIGNALS = {"levels": R.levels, "tone_levels": R.tone_levels}


def test_the_restated_fft_is_a_float32_fft():
    """fft512 against np.fft.fft in double: every component within FFT u32 sum |z| (the count of stft_f32_ref's error model), and
    the axes' twiddles exact."""
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((R.M, 9)) * 10.0 ** rng.uniform(-3, 3, (R.M, 1)) + 1j * rng.standard_normal((R.M, 9))).astype(np.complex64)
    z[:, 0] = 0
    z[7, 0] = 1                                                                    # one impulse: every output is one twiddle product
    zr, zi = R.fft512(z.real.copy(), z.imag.copy())
    ref = np.fft.fft(z.astype(np.complex128), axis=0)
    bound = R.FFT * R.U32 * (np.abs(z.real) + np.abs(z.imag)).astype(np.float64).sum(axis=0)[None, :]
    worst = max(B.ratio(np.abs(zr - ref.real), bound), B.ratio(np.abs(zi - ref.imag), bound))
    rel = np.sqrt((np.abs(zr + 1j * zi - ref) ** 2).sum(axis=0) / (np.abs(ref) ** 2).sum(axis=0)).max()
    print(f"fft512: worst component err / (FFT u32 mass) {worst:.3f}, worst relative L2 error {rel / R.U32:.2f} u32")
    assert worst < 1 and rel < 4 * R.U32
    c, s = R.twiddle(np.array([0, 16, 32, 48]), 64)
    assert c.tolist() == [1, 0, -1, 0] and s.tolist() == [0, -1, 0, 1]


@pytest.mark.parametrize("name", list(SIGNALS))
def test_correct_transforms_hold_the_forward_bounds(name):
    x = SIGNALS[name](T_CPU)
    ref, mass = R.forward_reference(x, T_CPU)
    lv = R.schedule(T_CPU + 3, 0)
    quiet = [t for t in range(T_CPU) if lv[t:t + 4].max() <= 3e-4]
    print(f"{name}: {len(quiet)} whole frames at the quiet level, frame mass from {mass.min():.3g} to {mass.max():.3g}")
    assert len(quiet) >= 4 and mass.max() > 1e4 * mass.min()
    for who, got in (("restatement", R.stft_f32(x, T_CPU)), ("torch.stft", R.torch_stft(x, T_CPU))):
        comp = R.forward_worst(got, ref, mass)
        pw = R.power_worst(R.power_f32(got), ref, mass)
        rel = R.rel_l2(got, ref)
        print(f"forward {name} {who}: component err/bound {comp:.4f} ({comp * R.G_F:.2f} u32 mass), power err/bound {pw:.4f}, "
              f"per-frame relative L2 {rel.min() / R.U32:.2f} .. {rel.max() / R.U32:.2f} u32")
        assert comp < 1 and pw < 1


def test_correct_transforms_hold_the_forward_bounds_on_impulses():
    T = 203
    x, pos = R.impulses(T)
    ref, mass = R.impulse_reference(T, pos)
    ref_fft, mass_fft = R.forward_reference(x, T)
    assert np.abs(ref - ref_fft).max() < 1e-12 and np.array_equal(mass, mass_fft)  # the closed form is the transform
    silent = mass == 0
    assert silent.sum() >= T // 5 and (~silent).sum() >= 4 * (T // 5) - 4
    assert 0.0 in set((pos % R.HOP).tolist()) and R.HOP - 1 in set((pos % R.HOP).tolist())
    for who, got in (("restatement", R.stft_f32(x, T)), ("torch.stft", R.torch_stft(x, T))):
        comp = R.forward_worst(got, ref, mass)
        pw = R.power_worst(R.power_f32(got), ref, mass)
        print(f"forward impulses {who}: component err/bound {comp:.4f}, power {pw:.4f}, frames without an impulse exactly zero: {not got[:, silent].any()}")
        assert comp < 1 and pw < 1 and not got[:, silent].any()


def margin_figures(what, rest, th, mut):
    """The figures of the L2 bar for two correct transforms (rel per frame) and the float32-argument one, printed: the medians of
    either correct transform against the other (spread), the median of the wrong one against the larger of the two, and the largest
    per-frame ratios."""
    ok = np.isfinite(rest) & np.isfinite(th)
    s = (rest / th)[ok]
    med = R.l2_median(rest[ok], th[ok]), R.l2_median(th[ok], rest[ok])         # where both exist
    spread_med, spread_max = max(med), max(s.max(), 1 / s.min())
    mut_med, mut_max = R.l2_median(mut, rest, th), R.l2_ratio(mut, rest, th)
    print(f"{what}: restatement / torch per frame {s.min():.3f} .. {s.max():.3f}, medians against each other {med[0]:.3f}, {med[1]:.3f}; "
          f"float32-argument twiddles / larger of the two: median {mut_med:.3f}, max {mut_max:.3f}")
    return spread_med, spread_max, mut_med, mut_max


def test_the_margin_separates_correct_from_wrong():
    """On `levels`, on `tone_levels` and on the inverse: the median of the per-frame ratio puts the two correct implementations
    against each other below MARGIN and the transform whose twiddle arguments are formed in float32 above it, so the median bar
    (l2_median <= MARGIN) rejects that transform on all three.  On `levels` the largest per-frame ratio separates as well."""
    for name in SIGNALS:
        x = SIGNALS[name](T_CPU)
        ref, _ = R.forward_reference(x, T_CPU)
        rest, th = R.rel_l2(R.stft_f32(x, T_CPU), ref), R.rel_l2(R.torch_stft(x, T_CPU), ref)
        mut = R.rel_l2(R.stft_f32(x, T_CPU, f32_arguments=True), ref)
        spread_med, spread_max, mut_med, mut_max = margin_figures(name, rest, th, mut)
        assert spread_med < R.MARGIN < mut_med
        assert R.l2_median(rest, rest, th) <= 1 and R.l2_median(th, rest, th) <= 1
        if name == "levels":                                                       # the per-frame maximum: `levels` only (stft_f32_ref)
            assert spread_max < R.MARGIN < mut_max
            assert R.l2_ratio(rest, rest, th) <= 1 and R.l2_ratio(th, rest, th) <= 1

    S = R.spectrum_levels(T_CPU)
    refi, _ = R.inverse_reference(S)
    want = R.weighted_hops(refi, T_CPU)
    rest, th = R.rel_l2(R.weighted_hops(R.istft_f32(S), T_CPU), want), R.inverse_rel_torch(S, refi)
    mut = R.rel_l2(R.weighted_hops(R.istft_f32(S, f32_arguments=True), T_CPU), want)
    spread_med, _, mut_med, _ = margin_figures("inverse", rest, th, mut)
    assert spread_med < R.MARGIN < mut_med
    assert np.isnan(th[:2]).all() and np.isnan(th[T_CPU + 1:]).all()               # the end hops: the restatement alone
    assert R.l2_median([1.0, 3.0], [np.nan, 2.0], [np.nan, np.nan]) == 1.5


def test_wrong_forward_transforms_are_rejected():
    """The quietest frame returned as zeros; one frame whose last two pair slots (samples 768 .. 1023) are the previous frame's -- a
    stale slot of the register ring.  Both in a frame 10^5 below the loudest: the component bound, the power bound and the L2 bar see
    them; 5e-6 of the spectrogram's global maximum does not."""
    x = R.levels(T_CPU)
    ref, mass = R.forward_reference(x, T_CPU)
    good = R.stft_f32(x, T_CPU)
    rest, th = R.rel_l2(good, ref), R.rel_l2(R.torch_stft(x, T_CPU), ref)
    q = int(np.argmin(mass))
    zeroed = good.copy()
    zeroed[:, q] = 0
    raw = x[R.frame_index(T_CPU)]
    raw[768:, q] = raw[768:, q - 1]
    stale = R.stft_f32(x, T_CPU, raw=raw)
    assert np.array_equal(np.delete(stale, q, axis=1), np.delete(good, q, axis=1))
    for what, got in (("quietest frame zeroed", zeroed), ("stale ring slot", stale)):
        comp, pw = R.forward_worst(got, ref, mass), R.power_worst(R.power_f32(got), ref, mass)
        l2 = R.l2_ratio(R.rel_l2(got, ref), rest, th)
        old = np.abs(got - ref).max() / (5e-6 * np.abs(ref).max())
        print(f"{what} (frame {q}, mass {mass[q]:.3g} of {mass.max():.3g}): component err/bound {comp:.3g}, power {pw:.3g}, L2 bar {l2:.3g}; "
              f"in units of 5e-6 x the global maximum {old:.3g}")
        assert comp > 1 and pw > 1 and l2 > R.MARGIN and old < 1


T_INV = [1, 2, 3, 4, 5, 64, 321]


@pytest.mark.parametrize("T", T_INV)
def test_correct_transforms_hold_the_inverse_bound(T):
    S = R.spectrum_levels(T, T)
    assert S[0].imag.all() and S[-1].imag.all()
    ref, bound = R.inverse_reference(S)
    y = R.istft_f32(S)
    worst = R.inverse_worst(y, ref, bound)
    assert ref[0] == 0 and bound[0] == 0 and y[0] == 0                             # the sample whose envelope is 0
    print(f"inverse T={T} restatement: err/bound {worst:.4f}")
    assert worst < 1
    if T >= 2:
        wt = R.inverse_worst(R.torch_istft(S), ref, bound, 2 * R.HOP, len(ref) - 4 * R.HOP)
        s = (R.rel_l2(R.weighted_hops(y, T), R.weighted_hops(ref, T)) / R.inverse_rel_torch(S, ref))[2:T + 1]
        print(f"inverse T={T} torch.istft: err/bound {wt:.4f}; per-hop relative L2, restatement / torch {s.min():.3f} .. {s.max():.3f}")
        assert wt < 1


def test_correct_transforms_hold_the_inverse_bound_on_sparse_spectra():
    """Single non-zero frames six apart: exact zeros wherever no frame covers a sample, the bound elsewhere."""
    T = 64
    frames = np.arange(3, T, 6)
    S = R.sparse_spectrum(T, frames)
    ref, bound = R.inverse_reference(S)
    uncovered = bound == 0
    assert uncovered.reshape(-1, R.HOP).all(axis=1).sum() >= 2 * len(frames) - 2
    for who, y, lo in (("restatement", R.istft_f32(S), 0), ("torch.istft", R.torch_istft(S), 2 * R.HOP)):
        hi = lo + len(y)
        worst = R.inverse_worst(y, ref, bound, lo, len(y))
        print(f"inverse sparse {who}: err/bound {worst:.4f}, uncovered samples exactly zero: {not y[uncovered[lo:hi]].any()}")
        assert worst < 1 and not y[uncovered[lo:hi]].any()


def test_wrong_inverse_transforms_are_rejected():
    """One halo frame (the third in front of a hop) dropped from that hop's sums, in a loud hop and in a quiet one, and the envelope
    of an edge hop taken as the four-frame value: the per-sample bound rejects them (one wrong hop does not move the median of the L2
    bar; its per-hop ratio against the larger yardstick is printed).  Float32-argument twiddles: the L2 bar as the GPU module applies
    it, the median against the larger of restatement and torch.istft, rejects them at this length too."""
    T = 64
    S = R.spectrum_levels(T, T)
    ref, bound = R.inverse_reference(S)
    want = R.weighted_hops(ref, T)
    good = R.istft_f32(S)
    rel_rest, rel_torch = R.rel_l2(R.weighted_hops(good, T), want), R.inverse_rel_torch(S, ref)
    lv = R.schedule(T, T)
    for what, h in (("loudest", int(np.argmax(lv[3:T])) + 3), ("quietest", int(np.argmin(lv[3:T])) + 3)):
        y = R.istft_f32(S, drop=(h - 3, h))
        assert np.array_equal(np.delete(y.reshape(-1, R.HOP), h, axis=0), np.delete(good.reshape(-1, R.HOP), h, axis=0))
        worst = R.inverse_worst(y, ref, bound)
        rel = R.rel_l2(R.weighted_hops(y, T), want)
        print(f"halo frame {h - 3} dropped from hop {h} ({what} frame, level {lv[h]:.3g}): err/bound {worst:.3g}, "
              f"per-hop L2 against the larger yardstick: max {R.l2_ratio(rel, rel_rest, rel_torch):.3g}, median {R.l2_median(rel, rel_rest, rel_torch):.3f}")
        assert worst > 1
    y = R.istft_f32(S, f32_arguments=True)
    l2 = R.l2_median(R.rel_l2(R.weighted_hops(y, T), want), rel_rest, rel_torch)
    print(f"float32-argument twiddles, T={T}: err/bound {R.inverse_worst(y, ref, bound):.4f}, L2 bar (median) {l2:.3f}")
    assert l2 > R.MARGIN
    for h in (0, 1, 2, T, T + 1, T + 2):
        y = R.istft_f32(S, four_frame_hop=h)
        worst = R.inverse_worst(y, ref, bound)
        print(f"edge hop {h} divided by the four-frame envelope: err/bound {worst:.3g}")
        assert worst > 1

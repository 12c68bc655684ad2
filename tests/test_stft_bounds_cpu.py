"""The bounds of tests/stft_bounds.py on the CPU: the reference itself holds them at every nfft / hop that the GPU tests use, and
transforms that are wrong by construction exceed them.  The wrong transforms are altered numpy restatements, never kernels.  Every
test prints the worst error in units of the bound."""
import numpy as np
import pytest

import stft_bounds as B
from oracle import stft_oracle as so

T_CPU = 7


def longdouble_dft(fr, twiddle_dtype=None):
    """Matrix DFT of the columns of fr ([nfft, T]) in np.longdouble -> (re, im) [F, T].  twiddle_dtype: round the twiddles to it."""
    nfft = fr.shape[0]
    pi = 4 * np.arctan(np.longdouble(1))
    k = (np.arange(nfft // 2 + 1)[:, None] * np.arange(nfft)[None, :]) % nfft       # exact index reduction: small arguments
    ang = -2 * pi * k.astype(np.longdouble) / nfft
    c, s = np.cos(ang), np.sin(ang)
    if twiddle_dtype is not None:
        c, s = c.astype(twiddle_dtype).astype(np.longdouble), s.astype(twiddle_dtype).astype(np.longdouble)
    f = fr.astype(np.longdouble)
    return c @ f, s @ f


def power32(S):
    """float32 magnitude of a complex64 array within 1 ulp (the double hypot rounded once; numpy's float32 loop is not), squared."""
    a = np.hypot(S.real.astype(np.float64), S.imag.astype(np.float64)).astype(np.float32)
    return a * a


def signals(nfft, hop, T):
    n = (T - 1) * hop + nfft
    return {"tone": B.tone_noise(n, nfft, nfft + hop), "noise": np.random.default_rng(nfft * 7 + hop).standard_normal(n)}


def spectrum(nfft, T, seed):
    rng = np.random.default_rng(seed)
    F = nfft // 2 + 1
    return (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))).astype(np.complex64)     # DC and Nyquist: imaginary parts set


def packed_inverse_frames(S, win, nfft, ignore_imag=True):
    """The kernels' inverse restated: Z[k] = E + i O from the half spectrum, an nfft / 2-point complex inverse FFT, samples interleaved."""
    S = np.asarray(S).astype(np.complex128)
    M = nfft // 2
    X = S[:M].copy()
    Xc = np.conj(S[M - np.arange(M)])
    if ignore_imag:
        X[0] = X[0].real
        Xc[0] = Xc[0].real
    k = np.arange(M)[:, None]
    E, O = 0.5 * (X + Xc), 0.5 * (X - Xc) * np.exp(2j * np.pi * k / nfft)
    z = np.fft.ifft(E + 1j * O, axis=0)
    fr = np.empty((nfft, S.shape[1]))
    fr[0::2], fr[1::2] = z.real, z.imag
    return B.window(win, nfft)[:, None] * fr


@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_the_reference_holds_the_forward_bound(nfft, hop):
    """np.fft.rfft in float64, rounded to complex64 (what a correct kernel returns), against a longdouble matrix DFT."""
    for name, x in signals(nfft, hop, T_CPU).items():
        fr = B.windowed_frames(x, "hann", nfft, hop, T_CPU)
        re, im = longdouble_dft(fr)
        ref = re.astype(np.float64) + 1j * im.astype(np.float64)
        mass = np.abs(fr).sum(axis=0)
        got = np.fft.rfft(fr, axis=0).astype(np.complex64)
        bre, bim = B.forward_bound(ref, mass, nfft)
        worst = max(B.ratio(np.abs(got.real.astype(np.longdouble) - re).astype(np.float64), bre),
                    B.ratio(np.abs(got.imag.astype(np.longdouble) - im).astype(np.float64), bim))
        pw = B.power_worst(power32(got), ref, mass, nfft)
        print(f"forward {nfft}/{hop} {name}: reference err/bound {worst:.3f}, power {pw:.3f}")
        assert worst < 1 and pw < 1
        if name == "tone" and nfft >= 800:
            small = np.mean(np.abs(ref) < 1e-3 * mass[None, :])
            print(f"    bins below 1e-3 of the frame's mass: {small:.3f}")
            assert small > 0.97


@pytest.mark.parametrize("win", ["hann", "hamming"])
@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_the_reference_holds_the_inverse_bound(nfft, hop, win):
    """The float32 oracle (librosa's float32 overlap-add) against the float64 one, whole signal, no sample excluded."""
    kw = dict(win=win, center=False, **B.oracle_sizes(nfft, hop))
    nov = B.n_ov(nfft, hop)
    for T in sorted({1, 2, nov, nov + 1, 7}):
        S = spectrum(nfft, T, nfft + T)
        ref, M, wss = B.inverse_reference(S, win, nfft, hop)
        assert np.array_equal(ref, so.istft(S, dtype="float64", **kw))
        worst = B.inverse_worst(so.istft(S, dtype="float32", **kw), ref, M, wss, nfft, hop)
        packed = B.inverse_reference(S, win, nfft, hop, frames=packed_inverse_frames(S, win, nfft))[0]
        worst_packed = B.inverse_worst(packed.astype(np.float32), ref, M, wss, nfft, hop)
        print(f"inverse {nfft}/{hop} {win} T={T}: float32 oracle err/bound {worst:.3f}, packed restatement rounded to float32 {worst_packed:.3f}")
        assert worst < 1 and worst_packed < 1
        if win == "hann":
            assert wss[0] == 0 and M[0] == 0 and ref[0] == 0                       # the sample whose bound is 0


@pytest.mark.parametrize("nfft,hop", [s for s in B.SHAPES if s[0] >= 256])
def test_float32_twiddles_exceed_the_forward_bound(nfft, hop):
    x = signals(nfft, hop, T_CPU)["tone"]
    fr = B.windowed_frames(x, "hann", nfft, hop, T_CPU)
    ref, mass = B.forward_reference(x, "hann", nfft, hop, T_CPU)
    re, im = longdouble_dft(fr, np.float32)
    got = (re.astype(np.float64) + 1j * im.astype(np.float64)).astype(np.complex64)
    worst = B.forward_worst(got, ref, mass, nfft)
    print(f"forward {nfft}/{hop}: twiddles rounded to float32 err/bound {worst:.3g}")
    assert worst > 1


@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_a_bin_index_off_by_one_exceeds_the_forward_bound(nfft, hop):
    for name, x in signals(nfft, hop, T_CPU).items():
        ref, mass = B.forward_reference(x, "hann", nfft, hop, T_CPU)
        got = np.roll(ref, 1, axis=0).astype(np.complex64)
        worst = B.forward_worst(got, ref, mass, nfft)
        pw = B.power_worst(power32(got), ref, mass, nfft)
        dropped = ref.astype(np.complex64)
        dropped[-1] = 0                                                            # a dropped Nyquist bin
        wd = B.forward_worst(dropped, ref, mass, nfft)
        print(f"forward {nfft}/{hop} {name}: bins off by one err/bound {worst:.3g}, power {pw:.3g}; Nyquist dropped {wd:.3g}")
        assert worst > 1 and pw > 1 and wd > 1


@pytest.mark.parametrize("win", ["hann", "hamming"])
@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_wrong_inverses_exceed_the_inverse_bound(nfft, hop, win):
    """The imaginary part of DC / Nyquist not ignored, and one frame's overlap-add shifted by one sample."""
    T = B.n_ov(nfft, hop) + 1
    S = spectrum(nfft, T, nfft + hop)
    ref, M, wss = B.inverse_reference(S, win, nfft, hop)
    leaky = B.inverse_reference(S, win, nfft, hop, frames=packed_inverse_frames(S, win, nfft, ignore_imag=False))[0]
    w_imag = B.inverse_worst(leaky.astype(np.float32), ref, M, wss, nfft, hop)
    fr = B.inverse_frames(S, win, nfft)
    fr[:, T // 2] = np.roll(fr[:, T // 2], 1)
    shifted = B.inverse_reference(S, win, nfft, hop, frames=fr)[0]
    w_shift = B.inverse_worst(shifted.astype(np.float32), ref, M, wss, nfft, hop)
    # the first covering frame left out of a sample's sum (a wrong tlo in the overlap-add)
    fr = B.inverse_frames(S, win, nfft)
    fr[hop:, 0] = 0
    w_tlo = B.inverse_worst(B.inverse_reference(S, win, nfft, hop, frames=fr)[0].astype(np.float32), ref, M, wss, nfft, hop)
    print(f"inverse {nfft}/{hop} {win}: imaginary DC / Nyquist kept err/bound {w_imag:.3g}, frame shifted {w_shift:.3g}, first frame cut {w_tlo:.3g}")
    assert w_imag > 1 and w_shift > 1
    assert w_tlo > 1 or hop >= nfft


def test_round_trip_bound_holds_for_the_reference():
    """float32 oracle inverse of the complex64 float64 transform against the signal, where n_ov frames overlap."""
    for nfft, hop in ((800, 200), (512, 128)):
        T = 9
        x = np.random.default_rng(nfft).standard_normal((T - 1) * hop + nfft)
        ref, mass = B.forward_reference(x, "hann", nfft, hop, T)
        S = ref.astype(np.complex64)
        y64, M, wss = B.inverse_reference(S, "hann", nfft, hop)
        bound = B.inverse_bound(M, wss, nfft, hop) + B.carried_forward_bound(*B.forward_bound(ref, mass, nfft), "hann", nfft, hop, wss)
        y = so.istft(S, center=False, dtype="float32", **B.oracle_sizes(nfft, hop))
        lo, hi = (B.n_ov(nfft, hop) - 1) * hop, T * hop
        worst = B.ratio(np.abs(y.astype(np.float64) - x)[lo:hi], bound[lo:hi])
        print(f"round trip {nfft}/{hop}: err/bound {worst:.3f} over samples [{lo}, {hi})")
        assert worst < 1

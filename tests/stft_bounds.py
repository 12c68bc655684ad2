"""Error bounds of the generic STFT / ISTFT kernels against a float64 transform (tests/test_gpu_stft_generic.py; the bounds
themselves are checked on the CPU in tests/test_stft_bounds_cpu.py).  Every bound is derived from the arithmetic below; nothing is
fitted to what the code under test returns.  u32 = 2^-24, u64 = 2^-53 (unit roundoffs of float32 and float64), bounds are first
order in them.

FORWARD.  X[f, t] = sum_i w_i x[t hop + i] exp(-2 pi i f i / nfft).  The kernels form every product and sum in double and round each
component (re, im) once to float32; the reference `ref` is the same sum in float64 or better (oracle.stft_oracle.stft(...,
dtype="complex128") = np.fft.rfft of the windowed frames).  Per component of bin f, frame t:

    |got - ref| <= u32 |ref| + (nfft + C) u64 mass_t,     mass_t = sum_i |w_i x_i|,     C = 4.

First term: the one float32 rounding of the component.  Second term: a sum of nfft products in double.  Each term a_i = w_i x_i c_i
(c_i one component of the twiddle, |c_i| <= 1) carries one rounding for the product w_i x_i, one for the rounded twiddle, one for the
product with it: 3 u64 |w_i x_i|.  Adding nfft such terms in ANY order (the O(N^2) loop of stft_dft_kernel, the log2-depth tree of
the radix-2 / radix-8 FFTs) passes each through at most nfft - 1 additions, every partial sum at most mass_t: (nfft - 1) u64 mass_t.
The FFT kernels transform nfft / 2 complex points and recover the real transform with a split step X[k] = E + W^k O; its extra
operations (one addition for E or O, one product with W^k, one addition) apply to sums over half the samples each, and are counted
as 2 more roundings of the whole mass.  (nfft - 1) + 3 + 2 = nfft + 4.  A twiddle from sincospi is within 1 ulp, not 1/2: inside the
slack of the worst-case addition count, which no summation order of more than two terms attains for every term at once.

POWER (layout 1): hypotf(re32, im32)^2 in float32 against |ref|^2 in float64.  re32 = re (1 + d), im32 = im (1 + d'), |d| <= u32,
so the exact magnitude of the rounded pair is |ref| (1 + d''), |d''| <= u32.  The float32 magnitude a is within 1 ulp = 2 u32 of
that (hypotf's documented accuracy).  a a is rounded once more.  Relative: POW_REL = (1 + u32)^2 (1 + 2 u32)^2 (1 + u32) - 1 =
7 u32 + O(u32^2).  The double term moves each component by D = (nfft + C) u64 mass_t, hence |ref|^2 by 2 |ref| D (first order):

    |got - |ref|^2| <= POW_REL |ref|^2 + 2 |ref| D.

The bound is that of the reference's operation.  stft1024_kernel's power form does not call hypotf: it takes v_sqrt_f32 (1 ulp) of
fma(re, re, im im) (u32 for the product, u32 for the fma, halved by the root, 2 u32 for the root): a magnitude within 3 u32, a
worst case of 9 u32 for the power.  The bound is NOT widened for it: the kernel is held to the 7 u32 of hypotf, and the largest
error measured over 4.2 million values is 6.8 u32 (tests/test_gpu_stft_generic.py, the 8199-frame case).

INVERSE.  frame_t[m] = w_m irfft(S[:, t])[m] in double; y[i] = (sum over the covering frames, in frame order, one float32
rounding per addition) / (window sum of squares built the same way), as librosa does.  Reference: oracle.stft_oracle.istft(...,
dtype="float64").  With n_ov = ceil(nfft / hop) (the most frames that cover one sample), M_i = sum over the covering frames of
|frame_t[i - t hop]| and wss_i the float64 window sum of squares:

    |got - ref| <= (n_ov + 2) u32 M_i / wss_i + (nfft + C) u64 M_i          (no division where wss_i is not above tiny).

First term: at most n_ov float32 roundings of a running sum that never exceeds M_i in magnitude, one for the float32 window sum,
one for the quotient, all relative to M_i / wss_i >= |ref_i|.  Second term: the double transform of each frame value, a sum of nfft
products as above, taken relative to the frame values themselves.  Where no frame covers a sample (behind the signal) and where
wss_i is exactly zero (Hann: sample 0 of an uncentred signal, whose only frame value is 0 w_0 = 0) M_i = 0 and the bound is 0: got
must be exactly 0.  No sample is excluded.

ROUND TRIP.  istft(stft(x)) against x where n_ov frames overlap: the inverse bound at the spectrum the forward kernel returned, plus
the forward bound carried through the (linear) inverse: |irfft(dS)[m]| <= (1 / nfft) sum_f c_f (|d re_f| + |d im_f|), c_f = 1 at DC
and Nyquist and 2 elsewhere, windowed, overlap-added and divided by wss_i.
"""
import numpy as np
from scipy.signal import get_window

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C = 4
POW_REL = (1 + U32) ** 2 * (1 + 2 * U32) ** 2 * (1 + U32) - 1

# nfft / hop by kernel family (csrc/stft.hip picks the kernel from them)
POW2 = [(8, 2), (16, 4), (512, 128), (2048, 512)]
DFT = [(4, 1), (12, 3), (800, 200), (800, 240), (2046, 512)]
HOP1024 = [(1024, 128), (1024, 512), (1024, 1024), (1024, 341)]
SHAPES = POW2 + DFT + HOP1024


def family(nfft, hop):
    return "1024 generic hop" if nfft == 1024 else "pow2" if nfft >= 8 and nfft & (nfft - 1) == 0 else "DFT"


def n_ov(nfft, hop):
    return -(-nfft // hop)


def oracle_sizes(nfft, hop):
    """fs / wlen_sec / hop_percent from which the oracle (and the wrapper) derive exactly this nfft and hop: one-second windows at
    fs = nfft, the hop fraction half a sample above hop / nfft so that int() cannot land below it."""
    kw = dict(fs=nfft, wlen_sec=1.0, hop_percent=(hop + 0.5) / nfft)
    assert int(kw["wlen_sec"] * kw["fs"]) == nfft and int(kw["hop_percent"] * nfft) == hop
    return kw


def window(win, nfft):
    return get_window(win, nfft, fftbins=True)


def tone_noise(n, nfft, seed):
    """A loud tone between two bins plus weak noise: nearly every bin lies far below the frame's mass, so the relative term of the
    forward bound cannot hide an absolute error."""
    i = np.arange(n, dtype=np.float64)
    return 0.8 * np.sin(2 * np.pi * 3.3 * i / nfft) + 1e-4 * np.random.default_rng(seed).standard_normal(n)


def windowed_frames(x, win, nfft, hop, T):
    """float64 [nfft, T]: w_i x[t hop + i]."""
    x = np.asarray(x, np.float64)
    idx = np.arange(nfft)[:, None] + hop * np.arange(T)[None, :]
    return window(win, nfft)[:, None] * x[idx]


def forward_reference(x, win, nfft, hop, T):
    """(ref complex128 [F, T], mass float64 [T])."""
    fr = windowed_frames(x, win, nfft, hop, T)
    return np.fft.rfft(fr, axis=0), np.abs(fr).sum(axis=0)


def double_term(nfft, mass):
    return (nfft + C) * U64 * np.asarray(mass, np.float64)[None, :]


def forward_bound(ref, mass, nfft):
    """(bound of the real parts, bound of the imaginary parts), each [F, T]."""
    d = double_term(nfft, mass)
    return U32 * np.abs(ref.real) + d, U32 * np.abs(ref.imag) + d


def power_bound(ref, mass, nfft):
    a = np.abs(ref)
    return POW_REL * a * a + 2 * a * double_term(nfft, mass)


def ratio(err, bound):
    """The largest err / bound; an error where the bound is 0 counts as infinite."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def forward_worst(got, ref, mass, nfft):
    """got: complex [F, T] -> the largest component error in units of its bound."""
    got = np.asarray(got)
    bre, bim = forward_bound(ref, mass, nfft)
    return max(ratio(np.abs(got.real.astype(np.float64) - ref.real), bre), ratio(np.abs(got.imag.astype(np.float64) - ref.imag), bim))


def power_worst(got, ref, mass, nfft):
    """got: float32 power [F, T]."""
    return ratio(np.abs(np.asarray(got, np.float64) - np.abs(ref) ** 2), power_bound(ref, mass, nfft))


def overlap_add(frames, hop, dtype=np.float64):
    """frames [nfft, T] added at t hop, in frame order, in `dtype`."""
    nfft, T = frames.shape
    y = np.zeros(nfft + hop * (T - 1), dtype)
    for t in range(T):
        y[t * hop:t * hop + nfft] += frames[:, t].astype(dtype)
    return y


def inverse_frames(S, win, nfft):
    """float64 [nfft, T]: w irfft(S) (numpy's C2R ignores the imaginary parts of DC and Nyquist)."""
    return window(win, nfft)[:, None] * np.fft.irfft(np.asarray(S).astype(np.complex128), n=nfft, axis=0)


def divide(y, wss):
    nz = wss > np.finfo(wss.dtype).tiny
    y = y.copy()
    y[nz] /= wss[nz]
    return y


def inverse_reference(S, win, nfft, hop, frames=None):
    """The whole untrimmed signal: (ref float64 [ntot], M [ntot], wss float64 [ntot])."""
    fr = inverse_frames(S, win, nfft) if frames is None else frames
    T = fr.shape[1]
    wss = overlap_add(np.repeat(window(win, nfft)[:, None] ** 2, T, axis=1), hop)
    return divide(overlap_add(fr, hop), wss), overlap_add(np.abs(fr), hop), wss


def inverse_bound(M, wss, nfft, hop):
    nz = wss > np.finfo(np.float64).tiny
    scale = np.where(nz, M / np.where(nz, wss, 1.0), M)
    return (n_ov(nfft, hop) + 2) * U32 * scale + (nfft + C) * U64 * M


def cut(a, start, out_len):
    """librosa's y[start:] fixed to out_len samples (zeros behind the signal)."""
    a = np.asarray(a)[start:start + out_len]
    return np.pad(a, (0, out_len - len(a)))


def inverse_worst(got, ref, M, wss, nfft, hop, start=0, out_len=None):
    """got: the kernel's y[start : start + out_len] -> the largest error in units of the bound."""
    out_len = len(ref) - start if out_len is None else out_len
    b = cut(inverse_bound(M, wss, nfft, hop), start, out_len)
    got = np.asarray(got, np.float64)
    assert got.shape == (out_len,)
    return ratio(np.abs(got - cut(ref, start, out_len)), b)


def carried_forward_bound(bre, bim, win, nfft, hop, wss):
    """The forward bound of every bin carried through the inverse: [ntot]."""
    c = np.full(bre.shape[0], 2.0)
    c[0] = c[-1] = 1.0
    per_frame = (c[:, None] * (bre + bim)).sum(axis=0) / nfft                    # bound of |irfft(dS)[m]|, any m
    num = overlap_add(window(win, nfft)[:, None] * per_frame[None, :], hop)
    nz = wss > np.finfo(np.float64).tiny
    return np.where(nz, num / np.where(nz, wss, 1.0), num)

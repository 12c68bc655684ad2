"""The float32-ARITHMETIC 1024 / 256 transforms (dvae_stft_f32 -> stft1024_walk_f32_kernel<POWER>, dvae_istft_f32 ->
istft1024_walk_f32_kernel, both on Fft512F of csrc/fft_wave.hpp) restated in numpy float32, their float64 references, and bounds and
bars that hold every frame to its OWN level (tests/test_stft_f32_bounds_cpu.py checks them on the CPU, tests/test_gpu_stft_f32.py
holds the kernels to them).  Every constant below is counted from the arithmetic; none is fitted to what a kernel returns.
u32 = 2^-24, all bounds first order in it.  The window is torch.hann_window(1024) in float32, w; nfft = 1024, hop = 256, M = 512.

RESTATEMENTS (the arithmetic, not the launch: no chunks, no register ring, every frame transformed on its own, vectorised over frames).
Forward: a_i = fl(w_i x_i); the 512 complex points p_j = a_2j + i a_2j+1 through Fft512F's three radix-8 passes in the kernel's order
(dft8 as written, twiddles = double cos / sin rounded to float32, a complex product as two rounded products and one rounded sum per
component); the split step X[k] = E + W^k O as written; the power form as two rounded squares and one rounded sum.  Inverse: split and
conjugate as written, the same FFT, acc = fma(w / 512, v, acc) over the covering frames in ascending order, the envelope as fma(w, w,
env) in the same order, one division where the envelope is above 1e-11.  The kernels are compiled with FMA contraction, which removes
roundings from the complex products; the restatement keeps them, so it is not bit-equal to a kernel and its error is a little larger.
fma(a, b, c) is restated as the double a b + c rounded to float32 (a b is exact in double; the double rounding differs from a true fma
in about one case in 2^29).

REFERENCES.  Forward: np.fft.rfft of the double products w_i x_i (exact in double).  Inverse: np.fft.irfft of the complex128 spectrum,
times w in double, overlap-added and divided by the double window sum of squares wss_i where that is not zero.

ERROR MODEL.  Errors are counted as complex moduli: a value z that is a sum over a set J of the inputs, each times a factor of modulus
1, has |z| <= mass_J = sum over J of |p_j| <= sum of |a_2j| + |a_2j+1|.  An operation whose two components are each rounded once
(relative u32 per component) moves z by at most u32 |z|: one UNIT of u32 mass_J.  Exact operations (times -i, times 0.5, conjugate) cost
nothing, additions of values add their errors, factors of modulus 1 keep an error's modulus.  The sets J of one level of the FFT
partition the inputs, so a level whose every operation costs at most c units adds at most c u32 mass to every output.
    complex addition                                                                       1
    dft8: three levels of additions, and on the paths through b[5], b[7] the rotation
      ((d.x + d.y) H, (d.y - d.x) H): the sum 1, H's own rounding 1, the product 1         3 + 3 = 6           DFT8
    product with a twiddle rounded to float32, a.x wr - a.y wi as written: the rounded
      twiddle moves it by u32 |a|; the two products by u32 (|a.x wr| + |a.y wi|) <= u32 |a|
      in each component, sqrt2 u32 |a| in modulus; the sum by u32 |z|                      2 + sqrt2 = 3.41    CMUL
      (contracted into an fma: one product rounding less)
    Fft512F: three dft8 and two twiddle products                                           3 DFT8 + 2 CMUL = 24.83   FFT

FORWARD, per component of bin f, frame t (mass_t = sum_i |w_i x_i|):

    |got - ref| <= G_F u32 mass_t,        G_F = sqrt2 (1 + FFT) + (2 + CMUL) = 41.9.

The window product is 1 unit, so every FFT output Z[k] carries an error e_k, |e_k| <= (1 + FFT) u32 mass_t.  The split step forms
E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2 and X[k] = E + W^k O: BOTH outputs carry the whole frame's error, X moves
by (|e_k + e'| + |e_k - e'|) / 2 <= sqrt(|e_k|^2 + |e'|^2) <= sqrt2 (1 + FFT) u32 mass_t.  The split's own roundings: the sum for E and
the difference for O (E is the transform of the even samples, O of the odd ones: together 1 unit of the frame's mass), the product
with W^k (CMUL) and the last sum (1).  A count of the roundings along ONE path (about 28: 1 + 3 DFT8 + 2 x 3 + 3) is no bound: it leaves
out that the split adds two transform outputs each carrying the full error (the sqrt2), and the complex product costs 2 + sqrt2, not 3.
A correct float32 transform measures about 2 u32 mass_t in the worst component (tests/test_stft_f32_bounds_cpu.py prints it): errors
add like a random walk, the bound adds them in line.  What the bound is for: a wrong SAMPLE (a stale ring slot, a frame read one hop
off, a frame not written) moves a component by a fraction of mass_t itself, 10^5 times the bound, in a quiet frame as in a loud one.

POWER (layout 1), re^2 + im^2 as two rounded squares and one rounded sum, D_t = G_F u32 mass_t:

    |got - |ref|^2| <= 2 (|re| + |im|) D_t + 2 D_t^2 + 2 u32 ((|re| + D_t)^2 + (|im| + D_t)^2).

First two terms: the complex bound carried through the squares.  Last term: each square rounded once, their sum once.

INVERSE, per output sample i of the whole untrimmed signal (frames t cover it at window position i - 256 t):

    |got - ref| <= [ G_I u32 sum_t |w_{i-256t}| massS_t  +  N_OLA u32 M_i ] / wss_i,
    massS_t = (1 / 1024) sum_f c_f (|Re S_ft| + |Im S_ft|),  c_f = 1 at DC and Nyquist, 2 elsewhere,
    G_I = 2 (2 + CMUL / 2 + FFT) = 57.1,        N_OLA = 4 + 4 + 1 = 9,

M_i = sum over the covering frames of |w irfft(S_t)| at i and wss_i the double window sum of squares, as in stft_bounds.inverse_reference.
First term: the frame values.  Z[k] = E + i O is built from X[k] and conj X[M-k] with s_k = |X[k]| + |X[M-k]|: the sum for E (u32 s_k / 2),
the difference (u32 s_k / 2), the product with the twiddle (CMUL u32 s_k / 2), the last sum (u32 |Z[k]| <= u32 s_k): (2 + CMUL / 2) u32 s_k,
then the FFT's FFT u32 sum_k |Z[k]| <= FFT u32 sum_k s_k, and sum_k s_k = sum_f c_f |S_f| <= 1024 massS_t.  The 1 / 512 of the
512-point inverse leaves 2 (...) u32 massS_t in every component; the window product happens inside the fma, unrounded.  This term is
needed because a float32 inverse FFT is not accurate relative to its own output where that cancels.  Second term: at most four fma
roundings of a running sum that never exceeds M_i, four of the envelope (each relative to a partial sum <= wss_i), one of the
quotient.  Where wss_i is exactly 0 (sample 0: w_0 = 0) both terms are 0 and the result must be exactly 0; where the envelope is not
above 1e-11 the kernel does not divide, which for this window happens at sample 0 only (w_1^2 = 8.9e-11).  No sample is excluded.

PER-FRAME L2 BAR.  rel_t(a) = ||a_t - ref_t||_2 / ||ref_t||_2 over the 513 bins of frame t; inverse: over the 256 samples of output hop h,
every sample weighted by its envelope wss_i, i.e. measured where the float32 sums are formed, before the division.  Inside the signal
wss_i is the constant 1.5 and the weight changes nothing; in the first and the last hop, where w falls to 1e-5, the unweighted norm is
the error of the one or two outermost samples divided by w, in which two correct transforms differ by any factor (3.6 measured), and
the weighted norm is that of all 256 samples (the outermost samples are held to the per-sample bound like every other).  The
yardsticks are the two correct float32 implementations, never the code under test:
    ratio_t(got) = rel_t(got) / max(rel_t(restatement), rel_t(host torch.stft / torch.istft in float32)).
MARGIN = 1.25 is one number for every case.  It must lie above what the two correct implementations give against each other and below
what a transform gives whose twiddle ARGUMENTS are formed in float32 (f32_arguments), and it is asserted through two statistics:
  l2_median  the median of ratio_t over the frames (hops) of the case: on every case.  tests/test_stft_f32_bounds_cpu.py recomputes, on
             `levels`, on `tone_levels` and on the inverse, the median of either correct implementation against the other (0.93 .. 1.08)
             and of the wrong transform against the larger of the two (1.44, 1.44, 1.43) and asserts spread < MARGIN < wrong on each.
  l2_ratio   the largest ratio_t: on `levels`, where every bin carries signal and the two correct implementations differ in no frame of
             3000 by more than 1.16, so that MARGIN separates frame by frame too (the wrong transform: 1.82 in its worst frame).
On `tone_levels` (a frame's norm and error sit in the few bins of the tone) and in the inverse (a hop's error is that of its loudest
covering frame) the two correct implementations differ in single frames by up to 1.6 and 1.4: there a bar of 1.25 on the largest
ratio_t would refuse torch against the restatement, so the largest ratio_t is printed only and the median carries the bar; a single
wrong frame or hop is what the component and per-sample bounds and the exact zeros are for.  A hop with one yardstick only (torch.istft
demands center=True and returns samples [512, ntot - 512): the two hops at either end) is measured against the restatement alone.
"""
import numpy as np
import torch

import stft_bounds as B

U32 = B.U32
NFFT, HOP, M, F = 1024, 256, 512, 513
DFT8 = 6.0
CMUL = 2.0 + np.sqrt(2.0)
FFT = 3 * DFT8 + 2 * CMUL
G_F = np.sqrt(2.0) * (1 + FFT) + 2 + CMUL
G_I = 2 * (2 + CMUL / 2 + FFT)
N_OLA = 4 + 4 + 1
MARGIN = 1.25
ENV_MIN = np.float32(1e-11)

f32 = np.float32
_H = f32(0.70710678118654752440)
_HALF = f32(0.5)


def window32():
    """torch.hann_window(1024): periodic, float32."""
    return torch.hann_window(NFFT).numpy().copy()


def twiddle(k, n, sign=-1, f32_arguments=False):
    """exp(sign 2 pi i k / n) as (cos, sin) in float32: double cos / sin rounded (exact 0 and +-1 on the axes, as sincospi gives them);
    f32_arguments: the wrong transform whose angle and cos / sin are formed in float32."""
    k = np.asarray(k, np.int64) % n
    if f32_arguments:
        ang = f32(sign) * f32(2) * f32(np.pi) * k.astype(f32) / f32(n)
        return np.cos(ang), np.sin(ang)
    ang = sign * 2 * np.pi * k.astype(np.float64) / n
    c, s = np.cos(ang), np.sin(ang)
    c[(4 * k) % n == 0] = np.round(c[(4 * k) % n == 0])
    s[(4 * k) % n == 0] = np.round(s[(4 * k) % n == 0])
    return c.astype(f32), s.astype(f32)


def cmulc(ax, ay, wr, wi):
    """fft_wave.hpp cmulc as written: every product and sum rounded to float32."""
    return ax * wr - ay * wi, ax * wi + ay * wr


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def dft8(ar, ai):
    """fft_wave.hpp dft8 on float32 arrays [8, ...]: natural-order output."""
    br, bi = np.empty_like(ar), np.empty_like(ai)
    br[:4], bi[:4] = ar[:4] + ar[4:], ai[:4] + ai[4:]
    dr, di = ar[:4] - ar[4:], ai[:4] - ai[4:]
    br[4], bi[4] = dr[0], di[0]
    br[5], bi[5] = (dr[1] + di[1]) * _H, (di[1] - dr[1]) * _H
    br[6], bi[6] = di[2], -dr[2]
    br[7], bi[7] = (di[3] - dr[3]) * _H, -(dr[3] + di[3]) * _H
    cr, ci = np.empty_like(ar), np.empty_like(ai)
    for q in (0, 4):
        cr[q], ci[q] = br[q] + br[q + 2], bi[q] + bi[q + 2]
        cr[q + 1], ci[q + 1] = br[q + 1] + br[q + 3], bi[q + 1] + bi[q + 3]
        cr[q + 2], ci[q + 2] = br[q] - br[q + 2], bi[q] - bi[q + 2]
        cr[q + 3], ci[q + 3] = bi[q + 1] - bi[q + 3], -(br[q + 1] - br[q + 3])
    orr, oi = np.empty_like(ar), np.empty_like(ai)
    for lo, a, b in ((0, 0, 1), (2, 2, 3), (1, 4, 5), (3, 6, 7)):
        orr[lo], oi[lo] = cr[a] + cr[b], ci[a] + ci[b]
        orr[lo + 4], oi[lo + 4] = cr[a] - cr[b], ci[a] - ci[b]
    return orr, oi


def fft512(zr, zi, f32_arguments=False):
    """Fft512F::run on float32 [512, T] (natural order in and out): lane l holds points l + 64 r; pass 0 writes index 8 l + r, pass 1
    multiplies by exp(-2 pi i r (l & 7) / 64) and writes (l >> 3) 64 + (l & 7) + 8 r, pass 2 multiplies by exp(-2 pi i r l / 512)."""
    T = zr.shape[1]
    lane, r = np.arange(64)[None, :], np.arange(8)[:, None]
    t1r, t1i = twiddle(r * (lane & 7), 64, f32_arguments=f32_arguments)
    t2r, t2i = twiddle(r * lane, 512, f32_arguments=f32_arguments)
    vr, vi = dft8(zr.reshape(8, 64, T), zi.reshape(8, 64, T))
    vr, vi = (a.transpose(1, 0, 2).reshape(8, 64, T) for a in (vr, vi))
    vr, vi = cmulc(vr, vi, t1r[:, :, None], t1i[:, :, None])
    vr, vi = dft8(vr, vi)
    vr, vi = (a.reshape(8, 8, 8, T).transpose(1, 0, 2, 3).reshape(8, 64, T) for a in (vr, vi))
    vr, vi = cmulc(vr, vi, t2r[:, :, None], t2i[:, :, None])
    vr, vi = dft8(vr, vi)
    return vr.reshape(M, T), vi.reshape(M, T)


def frame_index(T):
    return np.arange(NFFT)[:, None] + HOP * np.arange(T)[None, :]


def stft_f32(x, T, raw=None, f32_arguments=False):
    """The forward walk restated: x float32 -> complex64 [513, T].  raw: the frames' samples [1024, T] if not x[frame_index(T)]."""
    raw = np.asarray(x, f32)[frame_index(T)] if raw is None else np.asarray(raw, f32)
    fr = window32()[:, None] * raw
    zr, zi = fft512(fr[0::2], fr[1::2], f32_arguments)
    k = np.arange(M // 2)
    sr, si = twiddle(k, NFFT, f32_arguments=f32_arguments)
    zkr, zki, zcr, zci = zr[k], zi[k], zr[(M - k) & (M - 1)], -zi[(M - k) & (M - 1)]
    er, ei = _HALF * (zkr + zcr), _HALF * (zki + zci)
    dr, di = zkr - zcr, zki - zci
    wr, wi = cmulc(_HALF * di, -_HALF * dr, sr[:, None], si[:, None])
    X = np.empty((F, T), np.complex64)
    X.real[k], X.imag[k] = er + wr, ei + wi
    X.real[M - k], X.imag[M - k] = er - wr, -(ei - wi)
    X.real[M // 2], X.imag[M // 2] = zr[M // 2], -zi[M // 2]
    return X


def power_f32(X):
    """re^2 + im^2 of a complex64 array: two rounded squares, one rounded sum."""
    return X.real * X.real + X.imag * X.imag


def hop_range(j, T):
    """The output hops frame t = h - j contributes to at window positions [256 j, 256 j + 256): h = j .. T - 1 + j."""
    return slice(j, T + j)


def envelope_f32(T, four_frame_hop=None):
    """float32 [T + 3, 256]: fma(w, w, env) over the covering frames in ascending order.  four_frame_hop: that hop wrongly takes the
    value of a sample covered by four frames."""
    w = window32()
    env = np.zeros((T + 3, HOP), f32)
    full = np.zeros(HOP, f32)
    for j in (3, 2, 1, 0):
        seg = w[j * HOP:(j + 1) * HOP]
        env[hop_range(j, T)] = fma(seg, seg, env[hop_range(j, T)])
        full = fma(seg, seg, full)
    if four_frame_hop is not None:
        env[four_frame_hop] = full
    return env


def istft_f32(S, drop=None, four_frame_hop=None, f32_arguments=False):
    """The inverse walk restated: S complex [513, T] -> float32 [256 (T + 3)], the whole untrimmed signal.  drop = (t, h): frame t left
    out of the sums of output hop h; four_frame_hop: see envelope_f32; f32_arguments: see twiddle."""
    S = np.asarray(S).astype(np.complex64)
    T = S.shape[1]
    w = window32()
    k = np.arange(M)
    xkr, xki = S.real[k].copy(), S.imag[k].copy()
    xcr, xci = S.real[M - k].copy(), -S.imag[M - k]
    xki[0] = 0
    xci[0] = 0
    twr, twi = twiddle(k, NFFT, sign=1, f32_arguments=f32_arguments)
    er, ei = _HALF * (xkr + xcr), _HALF * (xki + xci)
    orr, oi = cmulc(_HALF * (xkr - xcr), _HALF * (xki - xci), twr[:, None], twi[:, None])
    vr, vi = fft512(er - oi, -(ei + orr), f32_arguments)
    v = np.empty((NFFT, T), f32)
    v[0::2], v[1::2] = vr, vi
    wn = w * f32(1.0 / M)
    wn[1::2] = -wn[1::2]
    acc = np.zeros((T + 3, HOP), f32)
    for j in (3, 2, 1, 0):                                                         # hop h takes frames h - 3, h - 2, h - 1, h in this order
        term_w = np.broadcast_to(wn[None, j * HOP:(j + 1) * HOP], (T, HOP)).copy()
        if drop is not None and drop[1] - drop[0] == j:
            term_w[drop[0]] = 0
        acc[hop_range(j, T)] = fma(term_w, v[j * HOP:(j + 1) * HOP].T, acc[hop_range(j, T)])
    env = envelope_f32(T, four_frame_hop)
    y = acc.copy()
    np.divide(acc, env, out=y, where=env > ENV_MIN)
    return y.reshape(-1)


# ---- float64 references and bounds -----------------------------------------------------------------------------------------------

def forward_reference(x, T, raw=None):
    """(ref complex128 [513, T], mass [T]) of float32 samples."""
    raw = np.asarray(x, f32)[frame_index(T)] if raw is None else raw
    fr = window32().astype(np.float64)[:, None] * raw.astype(np.float64)
    return np.fft.rfft(fr, axis=0), np.abs(fr).sum(axis=0)


def forward_bound(mass):
    return G_F * U32 * np.asarray(mass, np.float64)[None, :]


def forward_worst(got, ref, mass):
    """The largest component error in units of the bound."""
    got = np.asarray(got)
    b = forward_bound(mass)
    return max(B.ratio(np.abs(got.real.astype(np.float64) - ref.real), b), B.ratio(np.abs(got.imag.astype(np.float64) - ref.imag), b))


def power_bound(ref, mass):
    D = forward_bound(mass)
    re, im = np.abs(ref.real), np.abs(ref.imag)
    return 2 * (re + im) * D + 2 * D * D + 2 * U32 * ((re + D) ** 2 + (im + D) ** 2)


def power_worst(got, ref, mass):
    return B.ratio(np.abs(np.asarray(got, np.float64) - (ref.real ** 2 + ref.imag ** 2)), power_bound(ref, mass))


def overlap_add64(fr):
    """[1024, T] double -> [256 (T + 3)]."""
    T = fr.shape[1]
    y = np.zeros((T + 3, HOP))
    for j in range(4):
        y[hop_range(j, T)] += fr[j * HOP:(j + 1) * HOP].T
    return y.reshape(-1)


def inverse_reference(S):
    """The whole untrimmed signal: (ref [ntot], bound [ntot]) in float64."""
    S = np.asarray(S).astype(np.complex128)
    T = S.shape[1]
    w = window32().astype(np.float64)
    fr = w[:, None] * np.fft.irfft(S, n=NFFT, axis=0)
    c = np.full(F, 2.0)
    c[0] = c[-1] = 1.0
    massS = (c[:, None] * (np.abs(S.real) + np.abs(S.imag))).sum(axis=0) / NFFT
    wss = overlap_add64(np.repeat(w[:, None] ** 2, T, axis=1))
    num = G_I * U32 * overlap_add64(w[:, None] * massS[None, :]) + N_OLA * U32 * overlap_add64(np.abs(fr))
    nz = wss > 0
    safe = np.where(nz, wss, 1.0)
    return np.where(nz, overlap_add64(fr) / safe, 0.0), np.where(nz, num / safe, num)


def inverse_worst(got, ref, bound, start=0, out_len=None):
    """got: y[start : start + out_len] (zeros behind the signal) -> the largest error in units of the bound."""
    out_len = len(ref) - start if out_len is None else out_len
    got = np.asarray(got, np.float64)
    assert got.shape == (out_len,)
    return B.ratio(np.abs(got - B.cut(ref, start, out_len)), B.cut(bound, start, out_len))


# ---- the per-frame L2 bar --------------------------------------------------------------------------------------------------------------

def rel_l2(got, ref):
    """Per column of [n, T] arrays: ||got - ref|| / ||ref||."""
    got, ref = np.asarray(got), np.asarray(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((np.abs(got - ref) ** 2).sum(axis=0)) / np.sqrt((np.abs(ref) ** 2).sum(axis=0))


def envelope64(T):
    """wss_i of the whole untrimmed signal in double."""
    return overlap_add64(np.repeat(window32().astype(np.float64)[:, None] ** 2, T, axis=1))


def weighted_hops(y, T, first_hop=0):
    """Whole hops of the untrimmed signal of T frames, from hop first_hop on, every sample times its envelope, as columns: [256, n]."""
    y = np.asarray(y, np.float64)
    w = envelope64(T)[first_hop * HOP:first_hop * HOP + len(y)]
    return (y * w).reshape(-1, HOP).T


def l2_ratio(rel_got, *rel_yardsticks):
    """The largest rel_got / max(yardsticks) over the frames (a frame whose reference is zero must be returned as zero)."""
    yard = np.fmax.reduce([np.asarray(r, np.float64) for r in rel_yardsticks])
    return B.ratio(np.nan_to_num(rel_got, nan=0.0, posinf=np.inf), np.nan_to_num(yard, nan=0.0, posinf=0.0))


def l2_median(rel_got, *rel_yardsticks):
    """The median of rel_got / max(yardsticks) over the frames that have a yardstick (a yardstick that is NaN in a frame does not
    count there).  Every case of the tests has such frames; a case without one fails."""
    yard = np.fmax.reduce([np.asarray(r, np.float64) for r in rel_yardsticks])
    ok = np.isfinite(yard) & (yard > 0)
    assert ok.any()
    return float(np.median(np.asarray(rel_got, np.float64)[ok] / yard[ok]))


def torch_stft(x, T):
    """Host torch.stft in float32, uncentred -> complex64 [513, T]."""
    x = torch.from_numpy(np.asarray(x, f32)[:(T - 1) * HOP + NFFT].copy())
    return torch.stft(x, NFFT, HOP, window=torch.hann_window(NFFT), center=False, return_complex=True).numpy()


def torch_istft(S):
    """Host torch.istft in float32 (center=True: it refuses the zero envelope of sample 0) -> samples [512, ntot - 512) of the
    untrimmed signal."""
    S = torch.from_numpy(np.ascontiguousarray(S, np.complex64))
    return torch.istft(S, NFFT, HOP, window=torch.hann_window(NFFT), center=True).numpy()


def inverse_rel_torch(S, ref):
    """rel_l2 per output hop of torch.istft; NaN (no yardstick) for the two hops at either end, which it does not return."""
    T = np.asarray(S).shape[1]
    rel = np.full(T + 3, np.nan)
    if T >= 2:
        y = torch_istft(S)
        assert y.shape == (HOP * (T - 1),)
        rel[2:T + 1] = rel_l2(weighted_hops(y, T, 2), weighted_hops(ref[2 * HOP:(T + 1) * HOP], T, 2))
    return rel


# ---- signals ---------------------------------------------------------------------------------------------------------------------------

def schedule(n, seed):
    """n levels, log-uniform over 1e-4 .. 1e2; from 16 levels on with two runs of six quiet ones (1e-4 .. 3e-4): whole frames that are
    quiet next to loud ones."""
    rng = np.random.default_rng(seed)
    lv = 10.0 ** rng.uniform(-4, 2, n)
    if n >= 16:
        for a in (2, n // 2):
            lv[a:a + 6] = 1e-4 * rng.uniform(1, 3, 6)
    return lv


def n_samples(T):
    return (T - 1) * HOP + NFFT


def levels(T, seed=0):
    """Gaussian noise whose level changes every hop."""
    rng = np.random.default_rng(1000 + seed)
    return (np.repeat(schedule(T + 3, seed), HOP) * rng.standard_normal(n_samples(T))).astype(f32)


def tone_levels(T, seed=0):
    """stft_bounds.tone_noise (a loud tone between two bins plus weak noise) times the same schedule."""
    return (np.repeat(schedule(T + 3, seed), HOP) * B.tone_noise(n_samples(T), NFFT, 2000 + seed)).astype(f32)


def impulses(T, seed=0):
    """Zeros with a single 1.0 in every fifth hop at a varying offset: a frame sees at most one impulse, every fifth frame none.
    -> (x float32, positions)."""
    rng = np.random.default_rng(3000 + seed)
    hop_ids = np.arange(3, T + 3, 5)
    pos = hop_ids * HOP + rng.integers(0, HOP, len(hop_ids))
    pos[::7] = hop_ids[::7] * HOP                                                  # some at the very first sample of a hop
    pos[3::7] = hop_ids[3::7] * HOP + HOP - 1                                      # ... and at the last
    x = np.zeros(n_samples(T), f32)
    x[pos] = 1.0
    return x, pos


def impulse_reference(T, pos):
    """The float64 transform of impulses(): frame t with an impulse at window position i is w_i exp(-2 pi i f i / 1024), mass_t = w_i;
    a frame without one is zero.  -> (ref [513, T], mass [T])."""
    w = window32().astype(np.float64)
    ref, mass = np.zeros((F, T), np.complex128), np.zeros(T)
    f = np.arange(F)
    for p in pos:
        for t in range(max(0, (p - NFFT) // HOP + 1), min(T - 1, p // HOP) + 1):
            i = p - t * HOP
            assert 0 <= i < NFFT and mass[t] == 0
            ang = -2 * np.pi * ((f * i) % NFFT) / NFFT
            ref[:, t], mass[t] = w[i] * (np.cos(ang) + 1j * np.sin(ang)), w[i]
    return ref, mass


def spectrum_levels(T, seed=0):
    """complex64 noise [513, T] whose level changes every frame (the same schedule); the imaginary parts of DC and Nyquist are set,
    and the transform must ignore them."""
    rng = np.random.default_rng(4000 + seed)
    S = schedule(T, seed)[None, :] * (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T)))
    return S.astype(np.complex64)


def sparse_spectrum(T, frames, seed=0):
    """Zero except for the given frames."""
    S = np.zeros((F, T), np.complex64)
    S[:, frames] = spectrum_levels(T, seed)[:, frames]
    return S

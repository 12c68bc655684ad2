"""STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) restated in float64 numpy, laid out the way the pystoi package does it:
the contract of dvae_estoi_batch (include/dvae.h) and the reference of tests/test_estoi_cpu.py and tests/test_gpu_estoi.py.  pystoi
itself is not available to this repository, so parity with the package is unpinned; what is pinned is this file.  No scipy here.

    stoi(x, y, fs, extended)        the score
    stages(x, y, fs, extended)      the score with every intermediate: resampled signals, energies, mask, tob, per-segment terms

The two frame-count rules (silent-frame removal uses i + N_FRAME <= len, the spectra i + N_FRAME < len) are the named functions
frames_silent and frames_spec.
"""
from fractions import Fraction

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
WINDOW = np.hanning(N_FRAME + 2)[1:-1]
CLIP = 1.0 + 10.0 ** (-BETA / 20.0)
SHORT = 1e-5                      # the score of an utterance with fewer than N spectral frames


def frames_silent(n):
    """Frames of step 2 (silent-frame removal) in a signal of n samples: starts i = 0, HOP, ... with i + N_FRAME <= n."""
    return (int(n) - N_FRAME) // HOP + 1 if n >= N_FRAME else 0


def frames_spec(n):
    """Frames of step 3 (spectra) in a signal of n samples: starts i = 0, HOP, ... with i + N_FRAME < n (strict)."""
    return (int(n) - N_FRAME - 1) // HOP + 1 if n > N_FRAME else 0


def ratio(fs):
    """p / q = FS / fs reduced."""
    f = Fraction(FS, int(fs))
    return f.numerator, f.denominator


def resample_length(n, fs):
    p, q = ratio(fs)
    return -(-int(n) * p // q)


def resample_taps(fs):
    """-> (h [2 L + 1] float64 or None when fs == FS, p, q, L): the Kaiser-windowed sinc of Octave's resample, normalised to sum 1."""
    p, q = ratio(fs)
    if p == q:
        return None, 1, 1, 0
    fc = 1.0 / (2.0 * max(p, q))
    L = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return h / np.sum(h), p, q, L


def resample(x, fs, taps=None):
    """Output k of ceil(n p / q) = p sum_j h[j] xu[k q + j - L], xu = x zero-stuffed by p and zero outside the signal: one dot
    product per output over the taps of its phase, j = j0, j0 + p, ... with j0 = (L - k q) mod p."""
    x = np.asarray(x, np.float64)
    h, p, q, L = resample_taps(fs) if taps is None else taps
    if h is None:
        return x.copy()
    n = x.size
    out = np.zeros(-(-n * p // q))
    xp = np.concatenate([np.zeros(2 * L // p + 2), x, np.zeros(2 * L // p + 2)])
    pad = 2 * L // p + 2
    for r in range(p):                                   # outputs k = r (mod p) share a phase
        k = np.arange(r, out.size, p)
        if k.size == 0:
            continue
        j0 = (L - r * q) % p
        hp = h[j0::p]
        src0 = (k * q + j0 - L) // p                     # exact: k q + j0 - L is a multiple of p
        idx = src0[:, None] + np.arange(hp.size)[None, :] + pad
        out[k] = p * (xp[idx] @ hp)
    return out


def band_edges():
    """-> int64 [NUMBAND + 1]: band b sums the bins [edges[b], edges[b + 1]) of the NFFT-point spectrum at FS."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = np.array([int(np.argmin(np.square(f - MINFREQ * 2.0 ** ((2 * b - 1) / 6.0)))) for b in k])
    hi = np.array([int(np.argmin(np.square(f - MINFREQ * 2.0 ** ((2 * b + 1) / 6.0)))) for b in k])
    assert np.array_equal(lo[1:], hi[:-1])
    return np.concatenate([lo, hi[-1:]]).astype(np.int64)


def _frames(x, count):
    return np.stack([x[i * HOP:i * HOP + N_FRAME] for i in range(count)]) if count else np.zeros((0, N_FRAME))


def remove_silent_frames(x, y):
    """-> (xs, ys, energies of x's frames, mask): the kept windowed frames of both signals overlap-added at HOP in kept order."""
    J = frames_silent(len(x))
    xf, yf = _frames(x, J) * WINDOW, _frames(y, J) * WINDOW
    e = 20.0 * np.log10(np.sqrt(np.sum(xf * xf, axis=1)) + EPS)
    mask = (np.max(e) - DYN_RANGE - e) < 0 if J else np.zeros(0, bool)
    xf, yf = xf[mask], yf[mask]
    K = xf.shape[0]
    xs, ys = np.zeros((K - 1) * HOP + N_FRAME if K else 0), np.zeros((K - 1) * HOP + N_FRAME if K else 0)
    for i in range(K):
        xs[i * HOP:i * HOP + N_FRAME] += xf[i]
        ys[i * HOP:i * HOP + N_FRAME] += yf[i]
    return xs, ys, e, mask


def third_octaves(x, edges=None):
    """-> (tob [M, NUMBAND], windowed frames [M, N_FRAME]): sqrt of the band sums of the power spectrum of every frame."""
    edges = band_edges() if edges is None else edges
    M = frames_spec(len(x))
    v = _frames(x, M) * WINDOW
    power = np.abs(np.fft.rfft(v, NFFT, axis=1)) ** 2 if M else np.zeros((0, NFFT // 2 + 1))
    tob = np.sqrt(np.stack([power[:, edges[b]:edges[b + 1]].sum(axis=1) for b in range(NUMBAND)], axis=1))
    return tob, v


def _normalise(a, axis):
    a = a - np.mean(a, axis=axis, keepdims=True)
    return a / (np.sqrt(np.sum(a * a, axis=axis, keepdims=True)) + EPS)


def segment_terms(xt, yt, extended):
    """xt, yt: tob [M, NUMBAND] -> the per-segment terms [M - N + 1], whose mean is the score (segments m = N ... M)."""
    M = xt.shape[0]
    terms = np.zeros(max(M - N + 1, 0))
    for s in range(terms.size):
        X, Y = xt[s:s + N].T, yt[s:s + N].T              # [NUMBAND, N]: rows are bands
        if extended:
            xn, yn = _normalise(_normalise(X, 1), 0), _normalise(_normalise(Y, 1), 0)
            terms[s] = np.sum(xn * yn) / N
        else:
            alpha = np.sqrt(np.sum(X * X, axis=1, keepdims=True)) / (np.sqrt(np.sum(Y * Y, axis=1, keepdims=True)) + EPS)
            yp = np.minimum(alpha * Y, X * CLIP)
            terms[s] = np.sum(_normalise(yp, 1) * _normalise(X, 1)) / NUMBAND
    return terms


def stages(x, y, fs, extended=False):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y: 1-D arrays of equal length")
    taps = resample_taps(fs)
    xr, yr = resample(x, fs, taps), resample(y, fs, taps)
    xs, ys, e, mask = remove_silent_frames(xr, yr)
    xt, vx = third_octaves(xs)
    yt, vy = third_octaves(ys)
    terms = segment_terms(xt, yt, extended)
    d = float(np.mean(terms)) if terms.size else SHORT
    return {"d": d, "xr": xr, "yr": yr, "energies": e, "mask": mask, "xs": xs, "ys": ys, "vx": vx, "vy": vy, "tob_x": xt, "tob_y": yt,
            "terms": terms, "taps": taps, "info": (xr.size, int(mask.sum()), terms.size)}


def stoi(x, y, fs, extended=False):
    return stages(x, y, fs, extended)["d"]


def mask_clearance_db(st):
    """The distance in dB of the nearest non-zero frame of x to the silent-frame threshold (inf without such frames)."""
    e = st["energies"]
    if e.size == 0:
        return np.inf
    live = e > 20.0 * np.log10(EPS) + 1.0
    return float(np.min(np.abs(np.max(e) - DYN_RANGE - e[live]))) if live.any() else np.inf

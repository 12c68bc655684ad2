"""The contract of dvae_frame_stats (include/dvae.h) restated in numpy float64, its exact value, and the error bound the tests hold
both the restatement and the device to.  No GPU here.

Contract: s = sum x, q = sum x^2 (exact squares), mean = s / n, std = sqrt(max(q - n mean^2, 0) / (n - 1)), in double, any order of the
two sums; both results rounded to float32.

Bound, per bin, against the exact mean M and standard deviation sigma of the n float32 values (u = 2^-53, gamma_k = k u / (1 - k u),
A = sum |x|, Q = sum x^2, D = Q - n M^2 >= 0, V = D / (n - 1)):
  * a sum of n doubles in ANY order errs by at most gamma_{n-1} times the sum of the magnitudes (Higham, Accuracy and Stability, 4.2):
        |s^ - S| <= gamma_{n-1} A,        |q^ - Q| <= gamma_{n-1} Q        (the squares are exact, so they carry no error of their own);
  * mean:   m^ = fl(s^ / n):     em = gamma_{n-1} A / n + u (|M| + gamma_{n-1} A / n);
  * n m^2:  two rounded products: |fl(n fl(m^ m^)) - n M^2| <= gamma_2 n (|M| + em)^2 + n (2 |M| em + em^2)  =: ep;
  * d^ = fl(q^ - that):          ed = gamma_{n-1} Q + ep + u (D + gamma_{n-1} Q + ep);
  * v^ = fl(d^ / (n - 1)):       ev = ed / (n - 1) + u (V + ed / (n - 1));
  * sqrt:   |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= min(|a - b| / sqrt(b), sqrt(|a - b|)), the clamp at 0 only moves v^
            towards V >= 0:      es = min(ev / sigma, sqrt(ev)) + u (sigma + sqrt(ev));
  * float32: a double y rounds to float32 within 2^-24 |y| (normal range) or 2^-150 (below it).
The exact values themselves come from math.fsum (the correctly rounded exact sums) and long double arithmetic (u_l = 2^-64), whose
own error, 4 u (Q + n M^2) / (n - 1) on V carried through the same square root, is added to the bound, not neglected.
With std >= 1e-3 mean (make_frames) D >= 1e-6 Q or so, and gamma_{n-1} Q / D stays below 1e-6 for the sizes the tests use; on the gamma
draws themselves (std ~ mean) the double part is ~ n u and the bound is the float32 rounding, 6e-8 relative."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
BINS = 513


def gamma(k):
    return k * U / (1.0 - k * U)


def stats_ref(x):
    """The contract in numpy float64 on rows x [n, >= 513] -> (mean, std) float32 [513]."""
    x = np.asarray(x, np.float32)[:, :BINS].astype(np.float64)
    n = x.shape[0]
    if n < 2:
        raise ValueError("n < 2")
    s, q = x.sum(0), (x * x).sum(0)
    mean = s / n
    d = q - n * (mean * mean)
    std = np.sqrt(np.maximum(d, 0.0) / (n - 1))
    return mean.astype(np.float32), std.astype(np.float32)


def exact(x):
    """(M, sigma, A, Q) per bin: long doubles from the exactly rounded sums."""
    x = np.asarray(x, np.float32)[:, :BINS].astype(np.float64)
    n = x.shape[0]
    S = np.array([math.fsum(c) for c in x.T], LD)
    Q = np.array([math.fsum(c) for c in (x * x).T], LD)
    A = np.array([math.fsum(c) for c in np.abs(x).T], LD)
    M = S / LD(n)
    D = np.maximum(Q - LD(n) * M * M, LD(0))
    return M, np.sqrt(D / LD(n - 1)), A, Q


def bound(x):
    """(bound on |mean32 - M|, bound on |std32 - sigma|) per bin, float64."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    M, sig, A, Q = (np.asarray(a, np.float64) for a in exact(x))
    g = gamma(n - 1)
    em = g * A / n + U * (np.abs(M) + g * A / n)
    ep = gamma(2) * n * (np.abs(M) + em) ** 2 + n * (2 * np.abs(M) * em + em ** 2)
    D = sig ** 2 * (n - 1)
    ed = g * Q + ep + U * (D + g * Q + ep)
    ev = ed / (n - 1) + U * (sig ** 2 + ed / (n - 1))
    ev = ev + 4 * U * (Q + n * M * M) / (n - 1)                          # the error of `exact` itself
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.minimum(np.where(sig > 0, ev / sig, np.inf), np.sqrt(ev)) + U * (sig + np.sqrt(ev))
    f32 = lambda y, e: e + 2.0 ** -24 * (np.abs(y) + e) + 2.0 ** -149
    return f32(M, em), f32(sig, es)


CONST_BIN, CONST_VALUE = 100, 2.5        # exact in every partial sum of the sizes here: mean 2.5, std exactly 0
ODD_CONST_BIN = 101                      # a constant with a full mantissa: held to the bound (sigma = 0: the sqrt(ev) branch)
ZERO_BIN = 7


def make_frames(n, seed, ld=BINS):
    """Power-like rows [n, ld] float32: gamma(2) draws scaled per bin over four orders of magnitude (std = mean / sqrt(2)), one constant
    bin, one constant bin with a full mantissa, one bin of zeros; columns past 513 hold NaN (never read)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** np.linspace(-2.0, 1.7, BINS)
    x = np.full((n, ld), np.nan, np.float32)
    x[:, :BINS] = (rng.gamma(2.0, 1.0, size=(n, BINS)) * scale).astype(np.float32)
    v = x[:, :BINS].astype(np.float64)
    close = v.std(0, ddof=1) < 2e-3 * v.mean(0)              # (two draws of a short store may nearly coincide)
    x[0, :BINS][close] *= 2
    x[:, CONST_BIN] = CONST_VALUE
    x[:, ODD_CONST_BIN] = np.float32(0.1234567)
    x[:, ZERO_BIN] = 0.0
    return x


def check_inputs(x):
    """std >= 1e-3 mean in every non-constant bin (the bound is then not dominated by the cancellation in q - n mean^2)."""
    M, sig, _, _ = exact(x)
    varies = np.ptp(np.asarray(x)[:, :BINS], axis=0) > 0
    return bool(np.all(sig[varies] >= 1e-3 * np.abs(M[varies])))

"""Error bounds of the device's STOI / ESTOI against tests/estoi_ref.py, derived from the arithmetic and evaluated on each test's own
inputs from the restatement's intermediates.  Nothing here is fitted to what the code under test returns.

Both sides compute in float64 (u = 2^-53) and both round; a bound below is the sum of the two sides' worst cases, so rounding terms
carry a factor 2.  All bounds are first order in u; SLACK = 1.01 covers the products of two of them under the conditions asserted
(every relative perturbation of a norm <= 1e-3).

1. Resampler.  Output k is p times a sum of nt = ceil((2 L + 1) / p) products h_j x_j.  The device adds them by one fma per tap in
   tap order and multiplies by p: |err| <= (nt + 1) u p sum |h_j x_j|.  The restatement's matrix product adds them in an order that
   is not specified: the worst case of any order, (nt + 1) u on the same sum.  Together eps_r[k] = 2 (nt + 2) u S_k with
   S_k = p sum |h_j| |x_j| (the resampler applied to |x| with the taps |h|).  Without resampling eps_r = 0 (float32 -> double is exact).
2. Silent frames.  The mask is a discontinuity, not an error term: every test asserts from the restatement that no non-zero frame lies
   within MASK_CLEAR_DB of the threshold, and asserts the device's kept-frame count equal to the restatement's.  The energies differ
   by at most (20 / ln 10) (eps_r-induced + (256 + 70) u) dB, some 1e-12 dB: six orders inside the clearance.
3. Spectral input.  v = w (w a + w b) is linear in the resampled samples with weights in [0, 1], formed by the same three roundings
   per sample on both sides: |dv| <= P(eps_r) + 2 * 3 u P(|xr|), P = the frame / overlap-add / frame pipeline on a non-negative array.
4. FFT.  Every bin is a sum of the 256 inputs times unit-modulus factors that pass through log2 512 = 9 butterfly levels (four
   radix-4 passes and the real-FFT split on the device; pocketfft's passes in numpy), each level one complex product with a
   correctly rounded twiddle (<= 4 u) and one sum (u): |dX_k| <= |dv|_1 + 2 * 9 * 5 u |v|_1.  (|v|_1 >= |X_k| for every k, so this is
   the O(log2 512 u) per bin of the usual statement with the worst-case constant.)
5. Bands.  tob_b is the 2-norm of its nb bins: a norm is 1-Lipschitz, so |d tob_b| <= sqrt(nb) max_k |dX_k|; its own rounding (2
   per power, nb sums, one sqrt) is (nb + 4) u tob_b per side.  E_tob = sqrt(nb) E_bin + 2 (nb + 4) u tob_b -- also the bound of the
   per-element check of the debug output.
6. Mean removal and normalisation of c values a_i with bounds E_i: r = a - mean, |dr_i| <= E_i + mean(E) + 2 ((c + 1) u mean |a| +
   u |r_i|) -- the relative cost of the cancellation, |a| / |a - mean|, appears once r is divided by its norm;
   |d |r|| <= |E_r|_2 + 2 (c + 2) u |r|; out = r / (|r| + EPS): |d out_i| <= E_r,i / den + |r_i| E_norm / den^2 + 2 * 2 u |out_i|.
   ESTOI applies it to rows (c = 30), then columns (c = 15), of both blocks; STOI to rows of x and of y' = min(alpha y, CLIP x), where
   alpha = |x_row| / (|y_row| + EPS) carries the bounds of two norms and a division, and min is 1-Lipschitz in each argument
   (|d y'| <= max of the two arguments' bounds).
7. A segment's term sum(xn yn) / 30 (or / 15): |d| <= sum(|xn| E_y + |yn| E_x) / c + 2 (450 + 2) u sum |xn yn| / c, and the score is
   the mean of the terms: their mean bound plus 2 (segments + 2) u mean |term|.
For the inputs of the test suite the bound on d comes out between 1e-12 and 1e-9: six orders and more below the 1e-3 that a wrong
frame rule or band edge moves d by.
"""
import numpy as np

import estoi_ref as R

U = 2.0 ** -53
SLACK = 1.01
MASK_CLEAR_DB = 1e-6
FFT_LEVELS = 9


def resample_bound(x, taps):
    h, p, q, L = taps
    if h is None:
        return np.zeros(np.asarray(x).size)
    nt = -(-(2 * L + 1) // p)
    return 2.0 * (nt + 2) * U * R.resample(np.abs(x), None, (np.abs(h), p, q, L))


def _pipeline(z, mask):
    """Step 2's overlap-add of the kept windowed frames and step 3's windowed frames, on a non-negative array -> [M, 256]."""
    J = R.frames_silent(len(z))
    f = (R._frames(z, J) * R.WINDOW)[mask]
    K = f.shape[0]
    s = np.zeros((K - 1) * R.HOP + R.N_FRAME if K else 0)
    for i in range(K):
        s[i * R.HOP:i * R.HOP + R.N_FRAME] += f[i]
    return R._frames(s, R.frames_spec(len(s))) * R.WINDOW


def tob_bound(sig_r, eps_r, mask, v, tob, edges):
    """|device tob - restatement tob| per element [M, 15]."""
    dv = _pipeline(eps_r, mask) + 2 * 3 * U * _pipeline(np.abs(sig_r), mask)
    e_bin = dv.sum(axis=1) + 2 * FFT_LEVELS * 5 * U * np.abs(v).sum(axis=1)
    nb = np.diff(edges).astype(np.float64)
    return SLACK * (np.sqrt(nb)[None, :] * e_bin[:, None] + 2 * (nb[None, :] + 4) * U * tob)


def _norm_bound(a, E, axis):
    """Mean removal and normalisation along `axis` -> (result, its bound)."""
    c = a.shape[axis]
    r = a - a.mean(axis=axis, keepdims=True)
    Er = E + E.mean(axis=axis, keepdims=True) + 2 * ((c + 1) * U * np.abs(a).mean(axis=axis, keepdims=True) + U * np.abs(r))
    nr = np.sqrt(np.sum(r * r, axis=axis, keepdims=True))
    En = np.sqrt(np.sum(Er * Er, axis=axis, keepdims=True)) + 2 * (c + 2) * U * nr
    den = nr + R.EPS
    assert np.all(En <= 1e-3 * den), "a row or column whose norm is not resolved: the first-order bound does not apply"
    out = r / den
    return out, SLACK * (Er / den + np.abs(r) * En / den ** 2 + 4 * U * np.abs(out))


def score_bound(xt, yt, Ex, Ey, extended):
    """|device d - restatement d| from the tob of both signals and their element bounds."""
    M = xt.shape[0]
    nseg = max(M - R.N + 1, 0)
    if nseg == 0:
        return 0.0
    tot, mag = 0.0, 0.0
    for s in range(nseg):
        X, Y, EX, EY = xt[s:s + R.N].T, yt[s:s + R.N].T, Ex[s:s + R.N].T, Ey[s:s + R.N].T
        if extended:
            xn, Exn = _norm_bound(*_norm_bound(X, EX, 1), 0)
            yn, Eyn = _norm_bound(*_norm_bound(Y, EY, 1), 0)
            c = R.N
        else:
            nx, ny = np.sqrt(np.sum(X * X, axis=1, keepdims=True)), np.sqrt(np.sum(Y * Y, axis=1, keepdims=True))
            Enx = np.sqrt(np.sum(EX * EX, axis=1, keepdims=True)) + 2 * (R.N + 2) * U * nx
            Eny = np.sqrt(np.sum(EY * EY, axis=1, keepdims=True)) + 2 * (R.N + 2) * U * ny
            dy = ny + R.EPS
            assert np.all(Eny <= 1e-3 * dy)
            alpha = nx / dy
            Ealpha = Enx / dy + nx * Eny / dy ** 2 + 4 * U * alpha
            a, cl = alpha * Y, X * R.CLIP
            Ea = np.abs(Y) * Ealpha + alpha * EY + 2 * U * np.abs(a)
            Ecl = R.CLIP * EX + 4 * U * np.abs(cl)
            xn, Exn = _norm_bound(X, EX, 1)
            yn, Eyn = _norm_bound(np.minimum(a, cl), SLACK * np.maximum(Ea, Ecl), 1)
            c = R.NUMBAND
        tot += (np.sum(np.abs(xn) * Eyn + np.abs(yn) * Exn) + 2 * (R.N * R.NUMBAND + 2) * U * np.sum(np.abs(xn * yn))) / c
        mag += abs(np.sum(xn * yn)) / c
    return SLACK * (tot / nseg + 2 * (nseg + 2) * U * mag / nseg)


def evaluate(args):
    """(x, y, fs) -> everything a test needs about one utterance, for both scores: the restatement's values and intermediates that
    are compared, and the bounds.  A plain function of numpy arrays (it runs in worker processes)."""
    x, y, fs = args
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    st = R.stages(x, y, fs, True)
    edges = R.band_edges()
    Ex = tob_bound(st["xr"], resample_bound(x, st["taps"]), st["mask"], st["vx"], st["tob_x"], edges)
    Ey = tob_bound(st["yr"], resample_bound(y, st["taps"]), st["mask"], st["vy"], st["tob_y"], edges)
    out = {"info": st["info"], "clearance_db": R.mask_clearance_db(st), "tob_x": st["tob_x"], "tob_y": st["tob_y"], "E_tob_x": Ex, "E_tob_y": Ey,
           "estoi": st["d"], "estoi_bound": score_bound(st["tob_x"], st["tob_y"], Ex, Ey, True)}
    terms = R.segment_terms(st["tob_x"], st["tob_y"], False)
    out["stoi"] = float(np.mean(terms)) if terms.size else R.SHORT
    out["stoi_bound"] = score_bound(st["tob_x"], st["tob_y"], Ex, Ey, False)
    return out

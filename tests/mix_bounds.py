"""Error bounds of the device mixer against the reference (tests/test_gpu_mix.py), derived from the arithmetic.  Nothing here is
fitted to what the code under test returns.

Both sides run the operations of scripts/create_test_set.py:95-115 in double on the same inputs; they differ only in the ORDER of
the two power sums.  Notation: u = 2^-53, n = len, primes for the device's values; every bound is first order in u (the products of
two of them are below 1e-9 of the bound for n <= 1e6, which SLACK = 1.001 covers).  A correctly rounded operation applied to inputs
that differ relatively by e gives results that differ relatively by at most e + 2 u (each side's own rounding).

1. p = max |speech| is exact on both sides and s_i = fl(speech_i / p) has the same bits.
2. Ps = sum fl(s_i^2), Pn = sum fl(noise_i^2): both sides round every square, so they add the SAME non-negative terms and any order
   has a relative error of at most (adds on the longest path) u.  Device: at most 64 adds per lane, 6 butterfly levels, k = ceil(n /
   4096) partials in item order, gamma_dev = (70 + k) u.  Reference (numpy's pairwise sum, whose order is not specified): the worst
   case of any order, gamma_ref = (n - 1) u.  e_P = gamma_dev + gamma_ref.
3. target = fl(Ps f): e_P + 2 u.  k = fl(target / Pn): e_k = 2 e_P + 4 u.  g = sqrt(k), correctly rounded: e_g = e_k / 2 + 2 u =
   e_P + 4 u.  v_i = fl(noise_i g): e_v = e_P + 6 u, per element.
4. m_i = fl(s_i + v_i): |m'_i - m_i| <= e_v |v_i| + 2 u (|s_i| + |v_i|).  norm = max(|s|, |v|, |m|): a maximum moves by no more than
   its largest entry does, and norm >= max |v_i|, 2 norm >= max (|s_i| + |v_i|): e_norm = e_v + 4 u = e_P + 10 u.
5. out_speech_i = fl(s_i / norm):   e_speech = e_norm + 2 u       = e_P + 12 u, relative, per element.
   out_noise_i  = fl(v_i / norm):   e_noise  = e_v + e_norm + 2 u = 2 e_P + 18 u, relative, per element.
   out_mix_i    = fl(m_i / norm):   |out_mix'_i - out_mix_i| <= e_mix (|out_speech_i| + |out_noise_i|) with
                                    e_mix = (e_v + 2 u) + (e_norm + 2 u) = 2 e_P + 20 u.
   The mixture's bound cannot be relative to |s_i + v_i|, which can cancel.

At n = 48 000 (k = 12): e_P = 48 081 u = 5.3e-12, e_noise = 1.07e-11.  Nearly all of it is the reference's own worst case, n u.
"""
import numpy as np

from metrics_bounds import SLACK, U, gamma_dev, items


def e_power(n):
    """Relative difference of a power sum between the device and the reference."""
    return gamma_dev(items(n)) + (int(n) - 1) * U


def bounds(n):
    """Relative bounds by name for an utterance of n samples: k, norm, speech, noise (per element, relative to the reference's value)
    and mix (per element, relative to |out_speech| + |out_noise|)."""
    e = e_power(n)
    return {"k": SLACK * (2 * e + 4 * U), "norm": SLACK * (e + 10 * U), "speech": SLACK * (e + 12 * U), "noise": SLACK * (2 * e + 18 * U),
            "mix": SLACK * (2 * e + 20 * U)}


def worst(got, ref):
    """got, ref: dicts with speech, noise, mixture (arrays) and k, norm -> {name: (the largest error in units of its bound)}."""
    b = bounds(len(ref["speech"]))
    rs, rn = np.abs(ref["speech"]), np.abs(ref["noise"])

    def ratio(err, scale, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / (scale * bound))        # a sample that is zero in the reference must be zero
        return float(np.max(r))
    return {"speech": ratio(np.abs(got["speech"] - ref["speech"]), rs, b["speech"]),
            "noise": ratio(np.abs(got["noise"] - ref["noise"]), rn, b["noise"]),
            "mix": ratio(np.abs(got["mixture"] - ref["mixture"]), rs + rn, b["mix"]),
            "k": abs(got["k"] - ref["k"]) / (abs(ref["k"]) * b["k"]),
            "norm": abs(got["norm"] - ref["norm"]) / (abs(ref["norm"]) * b["norm"])}

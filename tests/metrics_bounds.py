"""Error bounds of the scale-invariant scores (tests/test_metrics_cpu.py, tests/test_gpu_metrics.py), derived from the arithmetic
and evaluated on each test's own inputs in numpy.longdouble.  Nothing here is fitted to what the code under test returns.

Notation: u = 2^-53; sh, s, n the estimate, the clean speech and the noise; alpha_s = <sh, s> / |s|^2, alpha_n = <sh, n> / |n|^2;
s_t = alpha_s s, e_n = alpha_n n, r1 = sh - s_t (= e_noise + e_art), r2 = r1 - e_n (= e_art).  All bounds are first order in u; the
products of two of them are below 1e-9 of the bound for every input the tests use (kappa <= 1e3, |ratio| <= 60 dB), which the
factor SLACK = 1.001 covers.

1. A sum of terms t_i.
   * device, `k` work items: every lane of a wave does at most 64 fma, then 6 butterfly levels, then the k partials are added in
     item order: |err| <= (64 + 6 + k) u sum |t_i|, gamma_dev = (70 + k) u.
   * reference (numpy's pairwise sums and BLAS dots, whose order is not specified): the worst case of any order, n u sum |t_i|;
     np.linalg.norm(x) ** 2 adds a square root and a square, 2 u more: gamma_ref = (n + 2) u.
   For |s|^2, |n|^2 and the residual energies all terms are positive and the relative error is gamma; for the dot products it is
   gamma kappa with kappa_s = sum |sh_i s_i| / |sum sh_i s_i| (kappa_n likewise).
2. alpha = dot / energy, one IEEE division: eps_alpha = gamma (kappa + 1) + u.
3. |s_t|^2 = alpha_s^2 |s|^2 and |e_n|^2 = alpha_n^2 |n|^2, two products: eps = 2 eps_alpha + gamma + 2 u.  (The reference squares
   the norm of the array alpha s instead: n roundings of the products, u, inside the same gamma_ref sum: the same expression holds.)
4. The residual energies.  Each r1_i = fl(sh_i - fl(alpha_s s_i)) carries |delta_i| <= u (|s_t,i| + |r1_i|), so that sum r1_i^2 moves
   by at most 2 sum |r1_i| |delta_i| <= 2 u (|r1| |s_t| + |r1|^2) (Cauchy-Schwarz), relatively rho_1 = 2 u (1 + |s_t| / |r1|): this is
   where a large ratio costs digits (at +50 dB, |s_t| / |r1| = 316).  alpha_s minimises |sh - alpha s|^2, so its error enters r1
   only in second order, eps_alpha_s^2 |s_t|^2 / |r1|^2, which is kept.  For r2_i = fl(r1_i - fl(alpha_n n_i)):
   rho_2 = 2 u (1 + (|s_t| + |r1| + |e_n|) / |r2|), and alpha_s, alpha_n are NOT its joint minimisers, so they enter in first order:
   |d |r2|^2| <= 2 |<r2, s>| |d alpha_s| + 2 |<r2, n>| |d alpha_n| <= 2 |r2| (eps_alpha_s |s_t| + eps_alpha_n |e_n|).
   With n, the SI-SDR denominator is formed as the reference forms it, e_noise + e_art = fl(e_n,i + r2_i) (alpha_n cancels in it,
   so only alpha_s enters, in second order as above), two more roundings per sample on top of r2's:
   rho_1 = 2 u (1 + (|s_t| + 2 |r1| + |e_n| + |r2|) / |r1|).
   eps_r = gamma + rho + the alpha terms.
5. A ratio in dB: (10 / ln 10) (eps_num + eps_den), plus two ulps of the result for log10 and the product with 10.

bound_db(..., k) is the device against the exact value; against the reference's recorded values the reference's own bound
(ref_db) is added.  Conditions on the inputs (asserted by every test that uses these bounds): kappa_s, kappa_n <= 1e3.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SLACK = 1.001
KAPPA_MAX = 1e3
DB = 10.0 / np.log(10.0)


def exact(sh, s, n=None):
    """Every quantity of the scores in long double (64-bit significand: its own error, n 2^-64, is 1e-3 of the smallest bound
    here).  n = None: the n-free form."""
    sh, s = np.asarray(sh, LD), np.asarray(s, LD)
    q = {"len": sh.size, "dot_s": np.sum(sh * s), "abs_dot_s": np.sum(np.abs(sh * s)), "ss": np.sum(s * s)}
    q["alpha_s"] = q["dot_s"] / q["ss"]
    r1 = sh - q["alpha_s"] * s
    q["e_noise_art"] = np.sum(r1 * r1)
    q["s_target"] = q["alpha_s"] ** 2 * q["ss"]
    q["kappa_s"] = float(q["abs_dot_s"] / abs(q["dot_s"]))
    q["si_sdr"] = float(10 * np.log10(q["s_target"] / q["e_noise_art"]))
    if n is not None:
        n = np.asarray(n, LD)
        q.update(dot_n=np.sum(sh * n), abs_dot_n=np.sum(np.abs(sh * n)), nn=np.sum(n * n))
        q["alpha_n"] = q["dot_n"] / q["nn"]
        r2 = r1 - q["alpha_n"] * n
        q["e_art"] = np.sum(r2 * r2)
        q["e_noise"] = q["alpha_n"] ** 2 * q["nn"]
        q["kappa_n"] = float(q["abs_dot_n"] / abs(q["dot_n"]))
        q["si_sir"] = float(10 * np.log10(q["s_target"] / q["e_noise"]))
        q["si_sar"] = float(10 * np.log10(q["s_target"] / q["e_art"]))
    return q


def items(length, chunk=4096):
    return -(-int(length) // chunk)


def gamma_dev(k):
    return (64 + 6 + k) * U


def gamma_ref(n):
    return (n + 2) * U


def relative(q, gamma):
    """Relative error bounds of the sums / energies of one utterance under the summation bound gamma: dict by the names of exact()."""
    f = lambda v: float(v)
    e = {"ss": gamma, "dot_s": gamma * q["kappa_s"]}
    e["alpha_s"] = gamma * (q["kappa_s"] + 1) + U
    e["s_target"] = 2 * e["alpha_s"] + gamma + 2 * U
    st, r1 = np.sqrt(f(q["s_target"])), np.sqrt(f(q["e_noise_art"]))
    if "nn" in q:
        e.update(nn=gamma, dot_n=gamma * q["kappa_n"])
        e["alpha_n"] = gamma * (q["kappa_n"] + 1) + U
        e["e_noise"] = 2 * e["alpha_n"] + gamma + 2 * U
        en, r2 = np.sqrt(f(q["e_noise"])), np.sqrt(f(q["e_art"]))
        first_order = 2 * (e["alpha_s"] * st + e["alpha_n"] * en)
        e["e_art"] = gamma + 2 * U * (1 + (st + r1 + en) / r2) + first_order / r2
    rho_1 = 2 * U * (1 + (st + 2 * r1 + en + r2) / r1) if "nn" in q else 2 * U * (1 + st / r1)
    e["e_noise_art"] = gamma + rho_1 + e["alpha_s"] ** 2 * (st / r1) ** 2
    return {k: SLACK * v for k, v in e.items()}


RATIOS = (("si_sdr", "e_noise_art"), ("si_sir", "e_noise"), ("si_sar", "e_art"))


def _db(q, e):
    out = {}
    for name, den in RATIOS:
        if name in q:
            out[name] = DB * (e["s_target"] + e[den]) + 2 * np.spacing(abs(q[name]))
    return out


def bound_db(q, k=None):
    """Device result against the exact value, in dB, by ratio name."""
    return _db(q, relative(q, gamma_dev(items(q["len"]) if k is None else k)))


def ref_db(q):
    """The reference's own result against the exact value, in dB, by ratio name."""
    return _db(q, relative(q, gamma_ref(q["len"])))


def check_kappa(q):
    assert q["kappa_s"] <= KAPPA_MAX and q.get("kappa_n", 1.0) <= KAPPA_MAX, (q["kappa_s"], q.get("kappa_n"))

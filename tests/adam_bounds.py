"""Truth, error bound and inputs of the optimizer update (tests/test_adam_bounds_cpu.py, tests/test_gpu_fused_apply.py).
Nothing here is fitted to what the code under test returns: the bound is derived below from the documented operation order.

The update under test (csrc/apply_common.hpp: adam_element; csrc/losses.hip: adam_kernel), every operation in float32:

    g   = fl(G * gs^)                 G = the float32 slab sum in slab order, gs^ = fl(grad_scale)
    m'  = fl(m + fl(c1^ * fl(g - m)))                          c1^ = fl(1 - b1)
    v'  = fl(fl(v * b2^) + fl(c2^ * fl(g * g)))                b2^ = fl(b2), c2^ = fl(1 - b2)
    den = fl(fl(sqrt(v') / s^) + eps^)                         s^ = fl(sqrt(1 - b2^t)), eps^ = fl(eps)
    p'  = fl(p - fl(ss^ * fl(m' / den)))                       ss^ = fl(lr / (1 - b1^t))

Truth: oracle.vae_oracle.adam_step on float64 copies of the float32 p, m, v and of G, with g = G * grad_scale and the hyper-parameters
as doubles.  Its own error (a dozen roundings of 2^-53) is 1e-8 of the smallest bound below.

Derivation.  u = 2^-24; every fl() and every rounded constant multiplies by (1 + d), |d| <= u; first order in u throughout.  c1, c2, s,
ss, m', v', p' are the float64 values and den = sqrt(v') / s + eps.  The inputs the tests use (|g|, |m| in 1e-12 .. 1e2, v in
1e-24 .. 1e4, eps >= 1e-8, c2 >= 1e-4) keep every intermediate either exactly zero or between 1e-29 and 1e9, so nothing underflows or
overflows and the relative model holds for every operation.

 g.  g^ = g (1 + th), |th| <= n_g u: n_g = 2 (the rounding of gs^ and the product), and n_g = 0 when grad_scale is a power of two, 1
     included: the constant and the product are then exact.
 m'. c1^ (g^ - m) carries three roundings (c1^, the difference, the product) on c1 (g - m), plus c1 g th; the final sum one rounding of m':
         bm = u (3 c1 |g - m| + n_g c1 |g| + |m'|)
 v'. both products are positive: v b2 carries two roundings (b2^, the product), c2 g^2 carries 3 + 2 n_g (c2^, the square, the product, twice
     th), the sum one more, so relatively at most 1 + max(2, 3 + 2 n_g):
         bv = (4 + 2 n_g) u v'
 den. sqrt moves by half the relative error of its argument and rounds once; s^ and the division round once each:
     |r^ - r| <= r (bv / (2 v') + 3 u) with r = sqrt(v') / s (r = 0 exactly when v' = 0: v' = 0 only if g = v = 0, and then the device's
     v' is 0 too).  eps^ carries u eps, the sum u den:
         bden = r (bv / (2 v') + 3 u) + u (eps + den)
 p'. q = m' / den moves by bm / den + |m'| bden / den^2 and rounds once; ss^ and the product round once each; the difference rounds p':
         bp = u |p'| + ss (bm / den + |m'| bden / den^2 + 3 u |m'| / den)

 Underflow.  The generated inputs never underflow (above), but the gradients of real steps may be tiny.  A product or quotient whose result
     falls below 2^-126 is rounded to a multiple of ETA = 2^-149: an absolute error of at most ETA on top of the relative one; sums and
     differences are exact there.  Two products can underflow on the way to m' (g, c1^ (g - m)), three on the way to v' (g^2, c2^ g^2,
     v b2^): bm += 2 ETA, bv += 3 ETA.  |sqrt(a) - sqrt(b)| <= sqrt(|a - b|) whatever a and b, so r moves by at most sqrt(3 ETA) / s more
     (bden += that; the first-order term bv / (2 v') is formed WITHOUT the ETA part), and q and ss^ q by ETA each:
     bp += ETA + ss (ETA + 2 ETA / den + |m'| sqrt(3 ETA) / (s den^2)).  Against the generated inputs these terms are below 1e-14 of the bound.

The asserted bounds are SLACK = 2 times these.  The neglected products of two errors are below 1e-6 of the first-order terms (every
relative error above is a few u = 6e-8 times at most c1 |g| / |m'|-like ratios that the first-order terms already carry), so 2 is
generous; it is the slack the issue of this test sets, and the float32 emulation -- which performs exactly the roundings counted --
reaches about half of the bound (tests/test_adam_bounds_cpu.py prints the ratios).  An implementation that contracts a product and a
sum into one fused multiply-add performs FEWER roundings and stays inside.  sqrt and the division must be correctly rounded.
"""
import math

import numpy as np

from oracle import vae_oracle as vo

U = 2.0 ** -24
ETA = 2.0 ** -149
SLACK = 2.0
F32 = np.float32

# (t, lr, b1, b2, eps, zero_state): the default first step (m = v = 0), the second step, a late step, a loose set whose 1 - b1 = 0.5 and
# eps = 1e-3 are far from the defaults, and a long-horizon set (b2 = 0.9999: 1 - b2 formed from the float32 b2 is off by 1e-3 relative)
HYPER = [(1, 1e-4, 0.9, 0.999, 1e-8, True), (2, 1e-4, 0.9, 0.999, 1e-8, False), (1000, 1e-3, 0.9, 0.999, 1e-8, False),
         (7, 1e-2, 0.5, 0.9, 1e-3, False), (100000, 1e-4, 0.95, 0.9999, 1e-6, False)]
GRAD_SCALES = [1.0, 1.0 / 8.0, 1.0 / 3.0]
FAULTS = ["bc_f32", "eps_inside", "no_bc2", "c2_from_f32_b2", "gscale_after_square", "slabs_reversed"]


def gscale_roundings(gs):
    return 0 if math.frexp(float(gs))[0] == 0.5 else 2


def slab_sum(slabs, reverse=False):
    """The float32 sum of the slabs in slab order, one rounded addition per slab (sequential: what slab_sum_at does)."""
    slabs = np.asarray(slabs, F32)
    order = range(slabs.shape[0] - 1, -1, -1) if reverse else range(slabs.shape[0])
    t = None
    with np.errstate(all="ignore"):
        for k in order:
            t = slabs[k].copy() if t is None else (t + slabs[k]).astype(F32)
    return t


def _signed_log_uniform(rng, n, lo, hi):
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(F32)


def block(n, k):
    """Index range of special block k (0 .. 5) of make_inputs(n, ...)."""
    b = max(n // 16, 1)
    return slice(k * b, (k + 1) * b)


def make_inputs(n, n_slabs, seed, zero_state=False, grad_scale=1.0):
    """p, m, v [n] and slabs [n_slabs, n], float32.  The slab SUM is signed log-uniform over about 1e-12 .. 1e2 (each slab = that value
    times a weight in (-1, 1)), m likewise, v log-uniform over 1e-24 .. 1e4, |p| over 1e-8 .. 3.  Six blocks of n / 16 elements,
    in this order: p = 0 (biases start at zero); g = 0; m = v = 0; m = g; slabs that cancel (terms 1e3 times their sum, as
    the frame slices of a weight gradient do); p tiny (1e-8 .. 1e-4: one ulp of p hides nothing there).  The first six sixteenths of the
    range are these blocks (block(n, k)), so that a prefix of a longer draw keeps them."""
    rng = np.random.default_rng(seed)
    g = _signed_log_uniform(rng, n, 1e-12, 1e2)
    m = _signed_log_uniform(rng, n, 1e-12, 1e2)
    v = np.exp(rng.uniform(np.log(1e-24), np.log(1e4), n)).astype(F32)
    p = _signed_log_uniform(rng, n, 1e-8, 3.0)
    b = max(n // 16, 1)
    blk = lambda k: block(n, k)
    if n_slabs == 1:
        slabs = g[None, :].copy()
    else:
        w = rng.uniform(-1.0, 1.0, (n_slabs, n))
        slabs = (g.astype(np.float64)[None, :] * w).astype(F32)
        c = blk(4)                                   # cancelling slabs: all but the last are 1e3 times the target, the last brings the sum back to it
        slabs[:-1, c] = (1e3 * g.astype(np.float64)[None, c] * w[:-1, c]).astype(F32)
        slabs[-1, c] = (g[c] - slab_sum(slabs[:-1, c])).astype(F32)
    p[blk(0)] = 0.0
    slabs[:, blk(1)] = 0.0
    m[blk(2)] = 0.0
    v[blk(2)] = 0.0
    p[blk(5)] = _signed_log_uniform(rng, b, 1e-8, 1e-4)
    if zero_state:
        m[:] = 0.0
        v[:] = 0.0
    else:
        with np.errstate(all="ignore"):
            m[blk(3)] = (slab_sum(slabs[:, blk(3)]) * F32(grad_scale)).astype(F32)
    return p, m, v, slabs


def truth(p, m, v, G, hyper, grad_scale=1.0):
    """float64 p', m', v' from the float32 inputs (G = the float32 slab sum)."""
    t, lr, b1, b2, eps = hyper[:5]
    f = lambda a: np.asarray(a, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        return vo.adam_step(f(p), f(G) * float(grad_scale), f(m), f(v), t, lr, b1, b2, eps)


def bounds(p, m, v, G, hyper, grad_scale=1.0):
    """(bp, bm, bv): SLACK times the first-order bounds of the module docstring, per element, from the float64 truth."""
    t, lr, b1, b2, eps = hyper[:5]
    f = lambda a: np.asarray(a, F32).astype(np.float64)
    m0, g = f(m), f(G) * float(grad_scale)
    p1, m1, v1 = truth(p, m, v, G, hyper, grad_scale)
    ng = gscale_roundings(grad_scale)
    c1, s, ss = 1.0 - b1, math.sqrt(1.0 - b2 ** t), lr / (1.0 - b1 ** t)
    r = np.sqrt(v1) / s
    den = r + eps
    bm = U * (3 * c1 * np.abs(g - m0) + ng * c1 * np.abs(g) + np.abs(m1))
    bv = (4 + 2 * ng) * U * v1
    with np.errstate(all="ignore"):
        rel_v = np.where(v1 > 0, bv / (2 * np.where(v1 > 0, v1, 1.0)), 0.0)
    bden = r * (rel_v + 3 * U) + U * (eps + den) + math.sqrt(3 * ETA) / s
    bm = bm + 2 * ETA
    bv = bv + 3 * ETA
    bp = U * np.abs(p1) + ss * (bm / den + np.abs(m1) * bden / den ** 2 + 3 * U * np.abs(m1) / den + ETA) + ETA
    return SLACK * bp, SLACK * bm, SLACK * bv


def emulate(p, m, v, slabs, hyper, grad_scale=1.0, fault=None):
    """The documented operation order in numpy float32, one rounding per operation (IEEE: infinities, NaN and subnormals as the
    hardware has them).  fault = one of FAULTS: the same with that one mistake (the sharpness tests)."""
    t, lr, b1, b2, eps = hyper[:5]
    p, m, v = (np.asarray(a, F32) for a in (p, m, v))
    with np.errstate(all="ignore"):
        G = slab_sum(slabs, reverse=(fault == "slabs_reversed"))
        gs = F32(grad_scale)
        c1, b2f = F32(1.0 - b1), F32(b2)
        c2 = F32(1.0) - b2f if fault == "c2_from_f32_b2" else F32(1.0 - b2)
        if fault == "bc_f32":                        # powf and the subtractions in float32
            bc1 = F32(1.0) - np.power(F32(b1), F32(t), dtype=F32)
            bc2 = F32(1.0) - np.power(b2f, F32(t), dtype=F32)
            ss, s = F32(lr) / bc1, np.sqrt(bc2, dtype=F32)
        else:
            ss, s = F32(lr / (1.0 - b1 ** t)), F32(math.sqrt(1.0 - b2 ** t))
        epsf = F32(eps)
        if fault == "gscale_after_square":
            g2 = G * G
            g = G * gs
        else:
            g = G * gs
            g2 = g * g
        m1 = m + c1 * (g - m)
        v1 = v * b2f + c2 * g2
        if fault == "eps_inside":
            den = (np.sqrt(v1) + epsf) / s
        elif fault == "no_bc2":
            den = np.sqrt(v1) + epsf
        else:
            den = np.sqrt(v1) / s + epsf
        p1 = p - ss * (m1 / den)
    assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
    return p1, m1, v1


def ratios(got, want, bound):
    """Per element |got - want| / bound; 0 where both the error and the bound are 0 (an exact result), inf where only the bound is."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
        r = np.where((err > 0) & ~(bound > 0), np.inf, r)
    return np.where(np.isnan(err), np.inf, r)


def special_values():
    """p, m, v, g [k] float32 whose update is compared EXACTLY with emulate() (one slab): zero state and zero gradient (p bit-unchanged);
    |g| = 1e20 (g^2 and v' infinite, the quotient 0, p unchanged, m' finite); a subnormal gradient; a NaN gradient (reaches p, m and v)."""
    sub = 1e-40
    rows = [(0.25, 0.0, 0.0, 0.0), (-0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0),
            (0.25, 0.01, 1e-4, 1e20), (-1.5, -0.01, 0.0, -1e20), (0.0, 0.0, 0.0, 1e20),
            (0.25, 0.0, 0.0, sub), (0.25, 1e-3, 1e-6, -sub), (1e-8, 0.0, 0.0, sub), (0.0, sub, 0.0, sub),
            (0.25, 0.01, 1e-4, np.nan), (0.0, 0.0, 0.0, np.nan)]
    a = np.array(rows, dtype=np.float64)
    return tuple(a[:, k].astype(F32) for k in range(4))


def same_bits(a, b):
    """Element-wise: the same float32 bit pattern, or both NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))

"""The per-element bound of the optimizer update (tests/adam_bounds.py) is SOUND -- a float32 emulation of the documented operation
order stays inside it against float64 on every element -- and SHARP: the same emulation with one plausible mistake leaves it on more
than 1 % of the elements.  The float64 oracle itself is pinned to torch.optim.Adam at the non-default hyper-parameters.  No GPU.

Measured (400 000 elements per case, 17 slabs): worst error / bound of the faultless emulation 0.50 (p), 0.50 (m), 0.44 (v) over the
five hyper-parameter sets x three grad_scale values.  Share of the elements outside the bound, per fault (100 000 elements, range over the
hyper-parameter sets on which the fault shows): bias corrections in float32 51 - 60 % of p at t <= 1000 (none at t = 7 with b1 = 0.5, b2 = 0.9
and at t = 100 000: the corrections are 1 there to float32); eps inside the division 26 - 88 % of p; no bc2 55 - 94 % of p; 1 - b2 from the
float32 b2 46 - 94 % of v (27 x its bound, 348 x at b2 = 0.9999; none at b2 = 0.9, whose float32 complement happens to be close);
grad_scale 1/3 applied after the square 56 - 94 % of v; slabs summed in reverse order 9 - 21 % of v, 6 - 12 % of m, 2 % of p (the elements
whose slabs cancel, where the order decides the last bits of the sum)."""
import numpy as np
import pytest
import torch

import adam_bounds as ab
from oracle import vae_oracle as vo

N_ELEM = 400_000
N_SLABS = 17


def _case(hi, hyper, gs, n=N_ELEM, n_slabs=N_SLABS):
    return ab.make_inputs(n, n_slabs, 1000 + hi, zero_state=hyper[5], grad_scale=gs)


@pytest.mark.parametrize("gs", ab.GRAD_SCALES, ids=["gs1", "gs1/8", "gs1/3"])
@pytest.mark.parametrize("hi", range(len(ab.HYPER)))
def test_float32_emulation_stays_inside_the_bound(hi, gs):
    hyper = ab.HYPER[hi]
    p, m, v, slabs = _case(hi, hyper, gs)
    G = ab.slab_sum(slabs)
    want = ab.truth(p, m, v, G, hyper, gs)
    bnd = ab.bounds(p, m, v, G, hyper, gs)
    got = ab.emulate(p, m, v, slabs, hyper, gs)
    # the emulation IS the oracle's own float32 form on the float32 scaled gradient
    ref32 = vo.adam_step(p, (G * np.float32(gs)).astype(np.float32), m, v, *hyper[:5])
    for a, b in zip(got, ref32):
        assert b.dtype == np.float32 and ab.same_bits(a, b).all()
    worst = [float(ab.ratios(g, w, b).max()) for g, w, b in zip(got, want, bnd)]
    print(f"adam bound soundness, set {hyper[:5]}, grad_scale {gs:.4g}: worst error/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst
    # ... and the bound is not vacuous: the emulation's error is a real share of it
    assert max(worst) >= 0.25, worst


def _outside(fault, hi, gs):
    hyper = ab.HYPER[hi]
    p, m, v, slabs = _case(hi, hyper, gs, n=100_000)
    G = ab.slab_sum(slabs)
    want = ab.truth(p, m, v, G, hyper, gs)
    bnd = ab.bounds(p, m, v, G, hyper, gs)
    got = ab.emulate(p, m, v, slabs, hyper, gs, fault=fault)
    return [float(np.mean(ab.ratios(g, w, b) > 1.0)) for g, w, b in zip(got, want, bnd)], [float(ab.ratios(g, w, b).max()) for g, w, b in zip(got, want, bnd)]


@pytest.mark.parametrize("fault", ab.FAULTS)
def test_one_fault_leaves_the_bound(fault):
    """Each fault must put more than 1 % of the elements of p, m or v outside the bound at one hyper-parameter set at least (grad_scale 1/3
    for the fault that concerns it, 1 otherwise)."""
    gs = 1.0 / 3.0 if fault == "gscale_after_square" else 1.0
    best = 0.0
    for hi in range(len(ab.HYPER)):
        share, worst = _outside(fault, hi, gs)
        print(f"fault {fault}, set {ab.HYPER[hi][:5]}: outside the bound p {share[0]:.1%} m {share[1]:.1%} v {share[2]:.1%}; worst ratio "
              f"p {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}")
        best = max(best, max(share))
    assert best > 0.01, (fault, best)


def test_special_values_follow_ieee():
    """What the device tests compare exactly, stated once on the emulation: a zero update leaves p bit-unchanged, an infinite g^2 leaves p
    unchanged with v' infinite and m' finite, a subnormal gradient is not flushed, a NaN gradient reaches p, m and v."""
    p, m, v, g = ab.special_values()
    for hyper in ab.HYPER:
        p1, m1, v1 = ab.emulate(p, m, v, g[None, :], hyper)
        zero = (g == 0) & (m == 0) & (v == 0)
        assert zero.sum() == 3 and ab.same_bits(p1[zero], p[zero]).all() and (m1[zero] == 0).all() and (v1[zero] == 0).all()
        big = np.abs(g) == np.float32(1e20)
        assert big.sum() == 3 and ab.same_bits(p1[big], p[big]).all() and np.isinf(v1[big]).all() and np.isfinite(m1[big]).all()
        nan = np.isnan(g)
        assert nan.sum() == 2 and np.isnan(p1[nan]).all() and np.isnan(m1[nan]).all() and np.isnan(v1[nan]).all()
        sub = (np.abs(g) > 0) & (np.abs(g) < np.finfo(np.float32).tiny)
        assert sub.sum() == 4 and (m1[sub] != m[sub]).any() and np.isfinite(p1[sub]).all()


@pytest.mark.parametrize("hi", range(1, len(ab.HYPER)))
def test_oracle_adam_matches_torch_at_non_default_hyper_parameters(hi):
    """vo.adam_step in float64 against torch.optim.Adam (float64, foreach=False) over five steps, 1e-12 relative."""
    _, lr, b1, b2, eps, _ = ab.HYPER[hi]
    rng = np.random.default_rng(hi)
    p0 = rng.standard_normal(4096)
    grads = [rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 1, 4096) for _ in range(5)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = vo.adam_step(p, g, m, v, t, lr, b1, b2, eps)
        st = opt.state[tp]
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)

"""The optimizer launch of the fused train step (csrc/apply_common.hpp: slab_sum_at, adam_element, apply_element; apply_kernel in
csrc/train_wgrad.hip; make_apply_args in csrc/train_fused.hip) and the layer-level dvae_adam_step (csrc/losses.hip) against float64, PER ELEMENT, from the
kernel's own inputs: the slabs it summed and the p, m, v it read.  The bound is derived in tests/adam_bounds.py (a few float32
roundings per element; tests/test_adam_bounds_cpu.py shows it sound and sharp); no element is exempted and no share may be off.

A. synthetic slabs, p, m, v written into a Trainer's buffers, dvae_train_apply called directly: M1, M2 y 1, M2 y 513, M2_info under fp32,
   bf16 and bf16x3; n_slabs 1, 2, 8, 9, 12, 13, 16, 17 (all four branches of slab_sum_at: <= 8, <= 12, <= 16 and the loop) on plans made
   with the ksplit hint 17, and n_slabs = 0 (the plan's own slab count) on the plans the library chooses at 8192 frames.
   dvae_train_plan itself never chooses more than 16 slabs (uniform slices cap at 16, the fp32 class-sliced schedule at min(16, frames / 128)):
   the loop branch of slab_sum_at is reachable through the caller's ksplit hint (up to 64) only, and is tested through it.
B. five real steps per case through Trainer.step with lr, betas and adam_eps changed between the steps, each update checked on its own
   inputs; repeated with DVAE_DEFER_APPLY=1 (the update of step n runs inside step n + 1's call and must use step n's hyper-parameters;
   the deferred rows kernel exists in the diagnostic library only: with the default library dvae_train_can_defer says no, the step is the
   three-launch one and is checked all the same).
C. dvae_adam_step through ops.adam_step_ at 5 000 011 elements.
D. recorded, not asserted: the share of elements bit-equal to torch.optim.Adam (CPU, float32, foreach=False) on the same float32 gradient.

Measured on the MI355X (55 tests, 22 s of wall time).  Worst error / bound -- the bound is 2 x the first-order sum, so a faultless float32
update reaches 0.5 -- A: p 0.499, m 0.499, v 0.447 on every model and policy (the arithmetic does not depend on them); B: p 0.497, m 0.500,
v 0.425, the same with the update deferred (diagnostic library: 5 of 5 updates of M2 y 513 / 8192 frames / bf16x3 ran inside the next
call); C: p 0.500, m 0.499, v 0.454.  No ratio above 1 anywhere.  D: p is bit-equal to torch.optim.Adam (CPU, float32) on 70 - 79 % of
the elements of A and 67 - 76 % of C -- the same share the numpy emulation of the documented order has against torch, whose CPU kernels
form lerp and addcmul / addcdiv in another order: "torch's op order" holds to the bound, not to the bit.

Scratch breakages of the product code (one at a time, nothing of them committed; the module was run once against each library):
  1 bias corrections with powf in make_apply_args          37 of 55 tests fail (A, B: p outside the bound)
  2 denom = (sqrtf(vi) + eps) / bc2_sqrt                     37 fail
  3 one_minus_b2 = 1.f - (float)beta2                        37 fail (v)
  4 grad_scale applied after g2                              24 fail (every case with grad_scale != 1)
  5 nslabs <= 9 in slab_sum_at                               15 fail (n_slabs 9: the bit-exact sum, the bound, the special values)
  6 no `i >= rows * cols` guard in apply_element             27 fail (p, m, v written in the alignment gaps)
  7 chunk_tensor built with ne / 64                          37 fail (the 16-element biases and the last element of the 513-element
                                                             bias never move: p at 3e5 x its bound)
  8 deferred step with the running call's lr                 1 fails (diagnostic library: the one case that defers; the same library
                                                             without the fault passes all 55)
The suite as it stood before this module was NOT run against the eight libraries (no device time was spent on it), so which of them it
also catches is reasoned, not measured: its checks of the parameters after a step allow 6 % of the elements off by steps x lr,
|dp| <= 1.05 lr, or an RMS drift of 2 - 8 %; faults 1 - 3 move p by 1e-7 relative of a step (float32 emulation,
tests/test_adam_bounds_cpu.py), far below all three; it passes grad_scale 1 or 1/2 only (4 would show at 1/2 in the data-parallel
tests; 5 shows only in a case that sums exactly 9 slabs, which was not looked for), no learning rate that changes between deferred
steps (8), and reads no gap (6); 7 leaves 33 bias elements one lr short, inside the 6 % and the 1.05 lr allowances.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import adam_bounds as ab
import golden_util as gu

pytestmark = pytest.mark.gpu
trainer = importlib.import_module("disentangled-vae_amd.trainer")
ops = importlib.import_module("disentangled-vae_amd.ops")
N = importlib.import_module("disentangled-vae_amd.native")

MODELS = [("M1", 0), ("M2", 1), ("M2", 513), ("M2_info", 1)]
PRECISIONS = ["fp32", "bf16", "bf16x3"]
N_SLABS = [1, 2, 8, 9, 12, 13, 16, 17]
HINT = 17
GAP_P, GAP_M, GAP_V, GAP_G = 7.0, 3.0, 5.0, 11.0            # finite sentinels of the alignment gaps: an update there would move all three


def _branch(n):
    return "<= 8" if n <= 8 else "<= 12" if n <= 12 else "<= 16" if n <= 16 else "loop"


def _dims(y_dim):
    return dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))


def _real_mask(tr):
    P = tr.plan.n_params
    real = np.zeros(P, bool)
    for i in range(tr.plan.n_tensors):
        o = tr.plan.tensor_offset[i]
        real[o:o + tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i]] = True
    return real


def _locate(tr, idx):
    for i in range(tr.plan.n_tensors):
        o, ne = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i]
        if o <= idx < o + ne:
            return f"{tr.names[i]}[{idx - o} of {ne}]"
    return f"gap at flat index {idx}"


def _slab_view(tr):
    P, ks, go = tr.plan.n_params, tr.plan.ksplit, tr.plan.grad_offset_bytes
    return tr.ws[go:go + 4 * P * ks].view(torch.float32).view(ks, P)


NMAX = 302784                                              # the longest flat buffer (M2 y 513)


@functools.lru_cache(maxsize=16)
def _drawn(n, n_slabs):
    return ab.make_inputs(n, n_slabs, 4000 + n_slabs)


def _inputs(P, n_slabs, zero_state, gs):
    """Generated inputs for a flat buffer of P floats (drawn once per slab count for the longest buffer, prefix taken)."""
    assert P <= NMAX
    p, m, v, slabs = (a[..., :P].copy() for a in _drawn(NMAX, n_slabs))
    if zero_state:
        m[:], v[:] = 0.0, 0.0
    else:
        b = ab.block(NMAX, 3)                    # the m = g block, for this grad_scale
        m[b] = (ab.slab_sum(slabs[:, b]) * np.float32(gs)).astype(np.float32)
    return p, m, v, slabs


def _load(tr, p, m, v, slabs, real):
    """Write p, m, v and the slabs into the trainer's buffers, the sentinels into every alignment gap; slabs the call must not read get NaN."""
    p, m, v, slabs = p.copy(), m.copy(), v.copy(), slabs.copy()
    p[~real], m[~real], v[~real] = GAP_P, GAP_M, GAP_V
    slabs[:, ~real] = GAP_G
    tr._params.copy_(torch.from_numpy(p))
    tr._m.copy_(torch.from_numpy(m))
    tr._v.copy_(torch.from_numpy(v))
    sv = _slab_view(tr)
    sv.fill_(float("nan"))
    sv[:slabs.shape[0]].copy_(torch.from_numpy(slabs))
    return p, m, v, slabs


def _apply(tr, n_slabs, hyper, gs):
    t, lr, b1, b2, eps = hyper[:5]
    N.check(tr.lib.dvae_train_apply(ctypes.byref(tr.plan), N.ptr(tr._params), N.ptr(tr._m), N.ptr(tr._v), N.ptr(tr.ws), n_slabs, t, lr, b1, b2,
                                    eps, gs, N.ptr(tr.losses), N.stream()), "dvae_train_apply")
    return tr._params.cpu().numpy(), tr._m.cpu().numpy(), tr._v.cpu().numpy()


def _check(tr, tag, before, G, got, hyper, gs, real, gap=None):
    """Every real element of p, m, v within the bound of its float64 update; every gap element bit-unchanged.  Returns the worst ratios."""
    p, m, v = before
    want = ab.truth(p[real], m[real], v[real], G[real], hyper, gs)
    bnd = ab.bounds(p[real], m[real], v[real], G[real], hyper, gs)
    idx = np.flatnonzero(real)
    worst = []
    gap = ~real if gap is None else gap
    for name, g_, w_, b_ in zip("pmv", got, want, bnd):
        r = ab.ratios(g_[real], w_, b_)
        k = int(np.argmax(r))
        worst.append(float(r[k]))
        assert r[k] <= 1.0, (f"{tag}: {name} outside the bound at {_locate(tr, int(idx[k]))}: got {g_[real][k]!r}, float64 {w_[k]!r}, bound {b_[k]:.3e}, "
                             f"ratio {r[k]:.3g}; {int((r > 1).sum())} of {r.size} elements outside")
    for name, g_, b_ in zip("pmv", got, before):
        same = ab.same_bits(g_[gap], b_[gap])
        assert same.all(), f"{tag}: {name} written in an alignment gap, first at {_locate(tr, int(np.flatnonzero(gap)[np.argmin(same)]))}"
    return worst


def _torch_share(before, G, got, hyper, gs):
    """D: share of the elements of p equal bit for bit to torch.optim.Adam (CPU, float32, foreach=False) on the gradient fl(G * fl(gs))."""
    t, lr, b1, b2, eps = hyper[:5]
    p, m, v = before
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    tp.grad = torch.from_numpy((G * np.float32(gs)).astype(np.float32))
    opt.step()
    return float(np.mean(ab.same_bits(tp.detach().numpy(), got[0])))


# ---- A. synthetic slabs through the C ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("model,y_dim", MODELS, ids=[f"{m}_y{y}" for m, y in MODELS])
def test_apply_from_synthetic_slabs_per_element(model, y_dim, precision):
    """Every slab count x every hyper-parameter set (grad_scale rotating through 1, 1/8, 1/3 so that each set meets each scale): p, m, v of
    every element within the bound, the gaps untouched.  Then beta1 = 0, m = 0: m' must be the float32 slab sum in slab order bit for bit
    (grad_scale 1), and fl(sum * fl(grad_scale)) at grad_scale 1/3 -- the order and the number of the slabs summed."""
    tr = trainer.Trainer(model, _dims(y_dim), gu.make_params(model, _dims(y_dim), 5), batch=HINT * 128, precision=precision, ksplit=HINT)
    assert tr.plan.ksplit == HINT
    real = _real_mask(tr)
    P = tr.plan.n_params
    reached, top = set(), [0.0, 0.0, 0.0]
    for si, n_slabs in enumerate(N_SLABS):
        for hi, hyper in enumerate(ab.HYPER):
            gs = ab.GRAD_SCALES[(si + hi) % 3]
            before = _load(tr, *_inputs(P, n_slabs, hyper[5], gs), real)
            G = ab.slab_sum(before[3])
            got = _apply(tr, n_slabs, hyper, gs)
            tag = f"apply[{model},y{y_dim},{precision}] n_slabs {n_slabs} ({_branch(n_slabs)}) set {hyper[:5]} grad_scale {gs:.4g}"
            worst = _check(tr, tag, before[:3], G, got, hyper, gs, real)
            share = _torch_share(before[:3], G, got, hyper, gs) if si == len(N_SLABS) - 1 else None
            print(f"{tag}: worst error/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}"
                  + ("" if share is None else f"; p bit-equal to torch.optim.Adam (CPU float32) on {share:.2%} of the elements"))
            top = [max(a, b) for a, b in zip(top, worst)]
            reached.add(_branch(n_slabs))
        for gs in (1.0, 1.0 / 3.0):
            hyper = (3, 1e-4, 0.0, 0.999, 1e-8)
            before = _load(tr, *_inputs(P, n_slabs, True, gs), real)
            got = _apply(tr, n_slabs, hyper, gs)
            G = ab.slab_sum(before[3])
            want_m = G if gs == 1.0 else (G * np.float32(gs)).astype(np.float32)
            same = ab.same_bits(got[1][real], want_m[real])
            assert same.all(), (f"apply[{model},y{y_dim},{precision}] n_slabs {n_slabs} ({_branch(n_slabs)}) grad_scale {gs:.4g}: m' is not the float32 slab sum in "
                                f"slab order on {int((~same).sum())} elements, first at {_locate(tr, int(np.flatnonzero(real)[np.argmin(same)]))}")
    assert reached == {"<= 8", "<= 12", "<= 16", "loop"}
    print(f"apply[{model},y{y_dim},{precision}]: branches of slab_sum_at reached {sorted(reached)}; worst error/bound over all cases p {top[0]:.3f} m {top[1]:.3f} v {top[2]:.3f}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("model,y_dim", MODELS, ids=[f"{m}_y{y}" for m, y in MODELS])
def test_apply_sums_the_plans_own_slab_count(model, y_dim, precision):
    """n_slabs = 0 on the plan the library chooses at 8192 frames (uniform slices under the bf16 policies, the class-sliced schedule under
    fp32): the slabs the weight-gradient launch of that plan fills are summed, no more (the rest hold NaN here) and no fewer."""
    tr = trainer.Trainer(model, _dims(y_dim), gu.make_params(model, _dims(y_dim), 5), batch=8192, precision=precision)
    real, P, n = _real_mask(tr), tr.plan.n_params, tr._used_slabs()
    assert 1 <= n <= tr.plan.ksplit <= 16
    for hi, hyper in enumerate(ab.HYPER):
        gs = ab.GRAD_SCALES[hi % 3]
        before = _load(tr, *_inputs(P, n, hyper[5], gs), real)
        G = ab.slab_sum(before[3])
        got = _apply(tr, 0, hyper, gs)
        tag = f"apply[{model},y{y_dim},{precision},own plan] ksplit {tr.plan.ksplit}, {n} slabs ({_branch(n)}), class-sliced {tr.plan.reserved0 > 0}, set {hyper[:5]} grad_scale {gs:.4g}"
        worst = _check(tr, tag, before[:3], G, got, hyper, gs, real)
        print(f"{tag}: worst error/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_apply_special_values(precision):
    """Zero state and zero gradient, an infinite g^2, a subnormal and a NaN gradient, planted at both ends of several tensors: exactly the
    IEEE result of the documented order (adam_bounds.emulate), bit for bit (NaN for NaN)."""
    tr = trainer.Trainer("M2", _dims(513), gu.make_params("M2", _dims(513), 5), batch=HINT * 128, precision=precision, ksplit=HINT)
    real, P = _real_mask(tr), tr.plan.n_params
    sp, sm, sv, sg = ab.special_values()
    k = sp.size
    for n_slabs in (1, 9, 17):
        for hyper in (ab.HYPER[1], ab.HYPER[3]):
            p, m, v, slabs = _inputs(P, n_slabs, False, 1.0)
            spots = []
            for i in (0, 1, 4, 8, 12, 13):           # first and last elements of weights and biases (each tensor holds two runs of k apart)
                o, ne = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i]
                for at in (o, o + ne - k):
                    p[at:at + k], m[at:at + k], v[at:at + k] = sp, sm, sv
                    slabs[:, at:at + k] = 0.0
                    slabs[n_slabs // 2, at:at + k] = sg            # the special gradient in one slab, zeros in the others
                    spots.append(at)
            before = _load(tr, p, m, v, slabs, real)
            got = _apply(tr, n_slabs, hyper, 1.0)
            want = ab.emulate(sp, sm, sv, sg[None, :], hyper)
            for at in spots:
                for name, g_, w_ in zip("pmv", got, want):
                    same = ab.same_bits(g_[at:at + k], w_)
                    assert same.all(), (precision, n_slabs, hyper[:5], name, _locate(tr, at + int(np.argmin(same))), g_[at:at + k], w_)
            zero = (sg == 0) & (sm == 0) & (sv == 0)
            big = np.abs(sg) == np.float32(1e20)
            for at in spots:
                assert ab.same_bits(got[0][at:at + k][zero | big], sp[zero | big]).all()
                assert np.isnan(got[0][at:at + k][np.isnan(sg)]).all() and np.isnan(got[1][at:at + k][np.isnan(sg)]).all() and np.isnan(got[2][at:at + k][np.isnan(sg)]).all()
            # the elements around them are ordinary ones
            fin = real.copy()
            for at in spots:
                fin[at:at + k] = False
            G = ab.slab_sum(before[3])
            _check(tr, f"special[{precision}] n_slabs {n_slabs}", before[:3], G, got, hyper, 1.0, fin, gap=~real)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("model,y_dim", MODELS, ids=[f"{m}_y{y}" for m, y in MODELS])
def test_apply_refreshes_the_weight_copies(model, y_dim, precision):
    """After dvae_train_apply the kernel-layout weight copies hold the NEW parameters: evaluate() on a fixed batch equals, bit for bit, the
    evaluate() of a fresh Trainer that loaded state_dict() -- and differs from the evaluate() before the update.  The apply launch and the
    repack go through the same apply_element, so this guards STALENESS of the copies and the ADAM / non-ADAM template pair, not the
    layout: the layout is guarded by the gradient tests of any following step (tests/test_gpu_fused.py)."""
    dims = _dims(y_dim)
    B = 256
    tr = trainer.Trainer(model, dims, gu.make_params(model, dims, 5), batch=B, precision=precision, ksplit=3)
    x, y, e = gu.make_batch(dims, B, 6)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    before = tr.evaluate(t(x), t(y) if y_dim else None, t(e)).cpu().numpy()
    P = tr.plan.n_params
    rng = np.random.default_rng(9)
    _slab_view(tr).copy_(torch.from_numpy(rng.standard_normal((tr.plan.ksplit, P)).astype(np.float32)))
    N.check(tr.lib.dvae_train_apply(ctypes.byref(tr.plan), N.ptr(tr._params), N.ptr(tr._m), N.ptr(tr._v), N.ptr(tr.ws), 3, 1, 1e-3, 0.9, 0.999, 1e-8,
                                    1.0, N.ptr(tr.losses), N.stream()), "dvae_train_apply")
    after = tr.evaluate(t(x), t(y) if y_dim else None, t(e)).cpu().numpy()
    fresh = trainer.Trainer(model, dims, tr.state_dict_numpy(), batch=B, precision=precision)
    want = fresh.evaluate(t(x), t(y) if y_dim else None, t(e)).cpu().numpy()
    assert np.all(np.isfinite(after)), after
    assert ab.same_bits(after, want).all(), (after, want)
    assert not ab.same_bits(after, before).all(), "every parameter moved by lr = 1e-3 and the losses did not"


# ---- B. real steps through Trainer.step -----------------------------------------------------------------------------------------------
SCHEDULE = [(1e-4, (0.9, 0.999), 1e-8), (3e-4, (0.9, 0.999), 1e-8), (1e-3, (0.8, 0.99), 1e-6), (5e-4, (0.95, 0.9999), 1e-7), (2e-3, (0.5, 0.9), 1e-3)]
STEP_CASES = [("M2", 513, 8192, "bf16x3"), ("M1", 0, 8192, "bf16"), ("M2", 1, 20000, "fp32"), ("M2_info", 1, 8192, "fp32"), ("M2_info", 1, 8192, "bf16x3")]


@pytest.mark.parametrize("defer", ["0", "1"], ids=["three_launch", "DVAE_DEFER_APPLY"])
@pytest.mark.parametrize("model,y_dim,B,precision", STEP_CASES, ids=[f"{m}_y{y}_B{b}_{p}" for m, y, b, p in STEP_CASES])
def test_five_real_steps_each_update_on_its_own_inputs(model, y_dim, B, precision, defer, monkeypatch):
    """p, m, v before a step, the slabs after it (include/dvae_train.h: they hold that step's gradient), p, m, v after the update: each of five
    consecutive updates within the bound of ITS inputs under ITS hyper-parameters, which change every step as a schedule would change
    them.  Where the update is deferred it runs inside the NEXT call, whose learning rate is another: the raw buffers are read without a
    flush after that call (they then hold the state after the deferred update and before the pending one)."""
    monkeypatch.setenv("DVAE_DEFER_APPLY", defer)
    dims = _dims(y_dim)
    tr = trainer.Trainer(model, dims, gu.make_params(model, dims, 21), batch=B, precision=precision)
    real, n = _real_mask(tr), tr._used_slabs()
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    raw = lambda: tuple(a.cpu().numpy().copy() for a in (tr._params, tr._m, tr._v))          # no flush
    state, waiting, deferred, top = raw(), None, 0, [0.0, 0.0, 0.0]

    def verify(k, job, got):
        before, G, hyper = job
        tag = f"step[{model},y{y_dim},B{B},{precision},defer {defer}] update {k} ({n} slabs: {_branch(n)}) set {hyper}"
        worst = _check(tr, tag, before, G, got, hyper, 1.0, real)
        print(f"{tag}: worst error/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
        top[:] = [max(a, b) for a, b in zip(top, worst)]

    for k, (lr, betas, eps) in enumerate(SCHEDULE, 1):
        tr.lr, tr.betas, tr.adam_eps = lr, betas, eps
        x, y, e = gu.make_batch(dims, B, 30 + k)
        tr.step(t(x), t(y) if y_dim else None, t(e))
        got = raw()
        if waiting is not None:                       # update k - 1 ran in the opening of this call
            verify(k - 1, waiting, got)
            state, waiting = got, None
        G = ab.slab_sum(_slab_view(tr)[:n].cpu().numpy())
        job = (state, G, (k, lr, betas[0], betas[1], eps))
        if tr.lib.dvae_train_pending(N.ptr(tr.ws)):
            assert defer == "1" and tr.lib.dvae_train_can_defer(ctypes.byref(tr.plan), N.ptr(tr.ws)) == 1
            for a, b in zip(got, state):
                assert ab.same_bits(a, b).all(), "a pending update has already touched p, m or v"
            waiting, deferred = job, deferred + 1
        else:
            verify(k, job, got)
            state = got
    if waiting is not None:
        tr.flush()                                    # the last pending update: apply_kernel, with the stored hyper-parameters
        verify(len(SCHEDULE), waiting, raw())
    print(f"step[{model},y{y_dim},B{B},{precision},defer {defer}]: {deferred} of {len(SCHEDULE)} updates deferred; worst error/bound p {top[0]:.3f} m {top[1]:.3f} v {top[2]:.3f}")


# ---- C. the layer-level optimizer kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hi", range(len(ab.HYPER)))
def test_adam_step_kernel_per_element(hi):
    """dvae_adam_step (csrc/losses.hip) through ops.adam_step_ at 5 000 011 elements (the grid-stride loop, an odd tail), every
    hyper-parameter set, grad_scale rotating through 1, 1/8, 1/3: the same bound; D's share recorded."""
    n = 5_000_011
    hyper, gs = ab.HYPER[hi], ab.GRAD_SCALES[(hi + 1) % 3]
    p, m, v, slabs = ab.make_inputs(n, 1, 77 + hi, zero_state=hyper[5], grad_scale=gs)
    G = slabs[0]
    dp, dm, dv, dg = (torch.from_numpy(a.copy()).cuda() for a in (p, m, v, G))
    ops.adam_step_(dp, dg, dm, dv, hyper[0], lr=hyper[1], betas=(hyper[2], hyper[3]), eps=hyper[4], grad_scale=gs)
    got = (dp.cpu().numpy(), dm.cpu().numpy(), dv.cpu().numpy())
    assert ab.same_bits(dg.cpu().numpy(), G).all()
    want = ab.truth(p, m, v, G, hyper, gs)
    bnd = ab.bounds(p, m, v, G, hyper, gs)
    worst = []
    for name, g_, w_, b_ in zip("pmv", got, want, bnd):
        r = ab.ratios(g_, w_, b_)
        k = int(np.argmax(r))
        worst.append(float(r[k]))
        assert r[k] <= 1.0, f"adam_step_ set {hyper[:5]} grad_scale {gs:.4g}: {name}[{k}] got {g_[k]!r}, float64 {w_[k]!r}, bound {b_[k]:.3e}, ratio {r[k]:.3g}; {int((r > 1).sum())} outside"
    print(f"adam_step_[n {n}] set {hyper[:5]} grad_scale {gs:.4g}: worst error/bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}; "
          f"p bit-equal to torch.optim.Adam (CPU float32) on {_torch_share((p, m, v), G, got, hyper, gs):.2%} of the elements")


def test_adam_step_kernel_special_values():
    sp, sm, sv, sg = ab.special_values()
    for hyper in ab.HYPER:
        dp, dm, dv, dg = (torch.from_numpy(a.copy()).cuda() for a in (sp, sm, sv, sg))
        ops.adam_step_(dp, dg, dm, dv, hyper[0], lr=hyper[1], betas=(hyper[2], hyper[3]), eps=hyper[4])
        got = (dp.cpu().numpy(), dm.cpu().numpy(), dv.cpu().numpy())
        zero = (sg == 0) & (sm == 0) & (sv == 0)
        big = np.abs(sg) == np.float32(1e20)
        nan = np.isnan(sg)
        assert ab.same_bits(got[0][zero | big], sp[zero | big]).all(), (hyper, got[0], sp)
        assert np.isinf(got[2][big]).all() and np.isfinite(got[1][big]).all()
        assert all(np.isnan(a[nan]).all() for a in got)
        sub = ~(zero | big | nan)                     # the subnormal gradients: the compiler may contract a product and a sum here, so the bound, not the bits
        want = ab.truth(sp[sub], sm[sub], sv[sub], sg[sub], hyper)
        bnd = ab.bounds(sp[sub], sm[sub], sv[sub], sg[sub], hyper)
        for g_, w_, b_ in zip(got, want, bnd):
            assert ab.ratios(g_[sub], w_, b_).max() <= 1.0, (hyper, g_[sub], w_, b_)

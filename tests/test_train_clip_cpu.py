"""Global-norm clipping on the any-size train steps, the parts that need no GPU (include/dvae_train.h:
dvae_train_{generic,clf,info}_apply_flat_clipped, dvae_train_gradnorm_scratch_bytes; disentangled-vae_amd/clip.py, accumulate.py).

A. tests/clip_ref.py -- the truth the GPU tests hold the device to -- against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in
   float64 on CPU tensors: the same arithmetic, bar 1e-12 relative.  torch keeps grad * coef in float64, so the restatement runs with
   scale_dtype=float64 here; the device's float32 scale is that number rounded once (asserted: within 2^-24 of it).
B. The library's refusals, host only: every one comes before anything touches the device, so the pointers handed over are never
   dereferenced (non-null, 16-byte aligned fakes).
C. max_norm=None on apply() / step() calls none of the new entry points: a stub `lib` records what is called."""
import contextlib
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import clip_ref

native = importlib.import_module("disentangled-vae_amd.native")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")
K = importlib.import_module("disentangled-vae_amd.clip")

E_BADARG = 1001
FAKE = ctypes.c_void_p(0x10000)          # never dereferenced
DIMS = dict(x_dim=513, y_dim=3, z_dim=17, h_dim=(129, 127))
HYPER = (1e-4, 0.9, 0.999, 1e-8)
KINDS = ["generic", "clf", "info"]


# ---- A: the restatement against torch ----
def _shapes(n_tensors):
    """weight / bias pairs of odd small sizes: 6 tensors (the classifier's count) or 26 (M2_info's)."""
    rng = np.random.default_rng(n_tensors)
    out = []
    for _ in range(n_tensors // 2):
        r, c = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        out += [(r, c), (r,)]
    return out


def _draw(n_tensors, seed):
    rng = np.random.default_rng(seed)
    mk = lambda scale: [(rng.standard_normal(s) * scale).astype(np.float32) for s in _shapes(n_tensors)]
    return mk(0.3), mk(2.0), mk(0.5)          # p, the gradient of step 1, of step 2


@pytest.mark.parametrize("threshold", ["clipped", "unclipped", "inf"])
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("n_tensors", [6, 26])
def test_restatement_equals_torch_clip_grad_norm_and_adam_in_float64(n_tensors, grad_scale, threshold):
    p0, g1, g2 = _draw(n_tensors, 7)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    norm1 = abs(grad_scale) * math.sqrt(clip_ref.sum_squares(g1))
    max_norm = {"clipped": 0.1 * norm1, "unclipped": 10.0 * norm1, "inf": math.inf}[threshold]
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p0]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    p = [a.astype(np.float64) for a in p0]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    for t, g in ((1, g1), (2, g2)):
        for q, gi in zip(params, g):
            q.grad = torch.tensor(gi, dtype=torch.float64) * grad_scale
        want_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2))
        opt.step()
        p, m, v, info = clip_ref.clipped_step(p, m, v, g, (t, lr, b1, b2, eps), grad_scale, max_norm, scale_dtype=np.float64)
        assert not info["skipped"] and abs(info["total_norm"] - want_norm) <= 1e-12 * want_norm
        assert (info["coef"] < 0.5) if threshold == "clipped" else (info["coef"] == 1.0)      # (step 2's gradient is a quarter of step 1's)
        f32 = clip_ref.clip_scale(g, grad_scale, max_norm)["gscale_eff"]          # the device's contract: the same scale rounded once
        assert abs(f32 - info["gscale_eff"]) <= 2.0 ** -24 * abs(info["gscale_eff"]) and f32 == float(np.float32(f32))
        for i, q in enumerate(params):
            st = opt.state[q]
            for got, want, what in ((p[i], q.detach().numpy(), "p"), (m[i], st["exp_avg"].numpy(), "m"), (v[i], st["exp_avg_sq"].numpy(), "v")):
                # relative to the tensor's largest element: m' = m + c1 (g - m) cancels where step 2's gradient opposes step 1's, and
                # an element 1e-4 of its terms carries their roundings of 2^-53 (seen: 5e-12 of one such element)
                assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want))), (t, i, what)


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_restatement_skips_a_gradient_that_is_not_finite(bad):
    p0, g1, _ = _draw(6, 3)
    g1[2].reshape(-1)[1] = bad
    z = [np.zeros_like(a) for a in p0]
    p, m, v, info = clip_ref.clipped_step(p0, z, z, g1, (1,) + HYPER, 0.5, 1.0)
    assert info["skipped"] and info["coef"] == 0.0 and info["gscale_eff"] == 0.0
    assert math.isnan(info["total_norm"]) if math.isnan(bad) else info["total_norm"] == math.inf
    for a, b in zip(p + m + v, p0 + z + z):
        assert np.array_equal(a, b.astype(np.float64))


# ---- B: the library's refusals ----
def _err():
    return native.load().dvae_last_error().decode()


def _plans():
    return {"generic": G.make_plan("M2", DIMS, 48), "clf": C.make_plan([513, [48, 200], 2], 48), "info": I.make_plan(DIMS, 48)}


def _clipped(kind, plan, params=FAKE, m=FAKE, v=FAKE, ws=FAKE, flat=FAKE, step=1, scale=1.0, max_norm=1.0, scratch=FAKE, norm2_out=FAKE,
             skipped=FAKE, plan_ptr=True):
    fn = getattr(native.load(), f"dvae_train_{kind}_apply_flat_clipped")
    return fn(ctypes.byref(plan) if plan_ptr else None, params, m, v, ws, flat, step, *HYPER, scale, max_norm, scratch, norm2_out, skipped, None)


@pytest.mark.parametrize("kind", KINDS)
def test_apply_flat_clipped_refuses_bad_arguments(kind):
    plan = _plans()[kind]
    assert _clipped(kind, plan, plan_ptr=False) == E_BADARG and "null plan" in _err()
    for name in ("params", "m", "v", "ws", "flat", "scratch", "norm2_out", "skipped"):
        assert _clipped(kind, plan, **{name: None}) == E_BADARG and "null pointer" in _err() and "apply_flat_clipped" in _err(), name
    for bad in (0.0, -1.0, math.nan, -math.inf):
        assert _clipped(kind, plan, max_norm=bad) == E_BADARG and "max_norm" in _err() and "positive" in _err(), bad
    # +inf is legal: the refusal it meets is the next check's, not max_norm's
    assert _clipped(kind, plan, max_norm=math.inf, flat=ctypes.c_void_p(0x10004)) == E_BADARG and "16-byte" in _err() and "max_norm" not in _err()
    assert _clipped(kind, plan, scratch=ctypes.c_void_p(0x10004)) == E_BADARG and "8-byte" in _err()
    assert _clipped(kind, plan, step=0) == E_BADARG and "1-based" in _err()
    for s in (math.nan, math.inf):
        assert _clipped(kind, plan, scale=s) == E_BADARG and "finite" in _err(), s
    plan.n_params += 64
    assert _clipped(kind, plan) == E_BADARG and "changed" in _err()


def test_gradnorm_scratch_bytes():
    lib = native.load()
    for bad in (0, -64, 1 << 31):
        assert lib.dvae_train_gradnorm_scratch_bytes(bad) == 0 and "n_params" in _err(), bad
    assert lib.dvae_train_gradnorm_scratch_bytes(64) == 8 and lib.dvae_train_gradnorm_scratch_bytes(4096) == 8
    assert lib.dvae_train_gradnorm_scratch_bytes(4160) == 16
    for plan in _plans().values():                         # one double per chunk of 4096 floats, whatever the plan
        assert lib.dvae_train_gradnorm_scratch_bytes(plan.n_params) == 8 * ((plan.n_params + 4095) // 4096)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.nan, -math.inf])
def test_python_refuses_max_norm_before_any_call(bad):
    with pytest.raises(ValueError, match="max_norm"):
        K.check_max_norm(bad)
    assert K.check_max_norm(math.inf) == math.inf and K.check_max_norm(5) == 5.0


# ---- C: max_norm=None calls none of the new entry points ----
class _StubLib:
    """Every dvae_* symbol: recorded, returns 0 (a size query: 8)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dvae_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            return 8 if name.endswith("_bytes") else 0
        return fn


def _host_trainer(kind, monkeypatch):
    """A trainer with host tensors and a stub library: step(), _micro() and _apply_flat() run their host code and the stub records the
    entry points they would launch."""
    cls = {"generic": G.GenericTrainer, "clf": C.ClassifierTrainer, "info": I.InfoTrainer}[kind]
    plan = _plans()[kind]
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(native, "stream", lambda: None)
    tr = cls.__new__(cls)
    tr.plan, tr.B, tr.device, tr.seed, tr.lib = plan, 48, torch.device("cpu"), 0, _StubLib()
    tr._shared = {"step_count": 0, "version": 0}
    tr._copy_version = 0
    tr._params, tr._m, tr._v = (torch.zeros(plan.n_params) for _ in range(3))
    tr.ws = torch.zeros(16, dtype=torch.uint8)
    tr.lr, tr.betas, tr.adam_eps, tr.elbo_eps, tr.bce_eps = 1e-4, (0.9, 0.999), 1e-8, 1e-8, 1e-8
    tr.y_dim, tr.z_dim = plan.y_dim, getattr(plan, "z_dim", 0)
    tr._losses3 = torch.zeros(3)
    tr.losses = tr._losses3[:1] if kind == "clf" else torch.zeros(8 if kind == "info" else 3)
    tr.counts = torch.zeros(4, dtype=torch.int64)
    tr.names = []
    x, y = torch.zeros(48, 513), torch.zeros(48, plan.y_dim)
    batch = (x, y) if kind == "clf" else (x, y, torch.zeros(48, tr.z_dim))
    return tr, batch


@pytest.mark.parametrize("kind", KINDS)
def test_max_norm_none_calls_none_of_the_new_entry_points(kind, monkeypatch):
    tr, batch = _host_trainer(kind, monkeypatch)
    new = lambda: [c for c in tr.lib.calls if "clipped" in c or "gradnorm" in c]
    tr.step(*batch)
    tr.step(*batch, max_norm=None)
    assert tr.lib.calls == [f"dvae_train_{kind}_step"] * 2
    acc = A.AccumulatedStep(tr)
    acc.micro(*batch)
    acc.apply()
    acc.micro(*batch)
    acc.apply(max_norm=None)
    assert tr.lib.calls[2:] == [f"dvae_train_{kind}_grads", f"dvae_train_{kind}_reduce", f"dvae_train_{kind}_apply_flat"] * 2
    assert new() == [] and "clip" not in tr._shared and tr.step_count == 4
    # a refused threshold: raised before the step is counted or anything is called; the micro-batch stays pending
    acc.micro(*batch)
    n = len(tr.lib.calls)
    with pytest.raises(ValueError, match="max_norm"):
        acc.apply(max_norm=0.0)
    with pytest.raises(ValueError, match="max_norm"):
        tr.step(*batch, max_norm=math.nan)
    assert len(tr.lib.calls) == n and tr.step_count == 4 and acc._pending == [48]
    # the control: with a threshold the stub does see them -- one clipped apply behind the reduce, five entry points for a step
    acc.apply(max_norm=math.inf)
    assert tr.lib.calls[n:] == ["dvae_train_gradnorm_scratch_bytes", f"dvae_train_{kind}_apply_flat_clipped"]
    n = len(tr.lib.calls)
    tr.step(*batch, max_norm=5.0)
    assert tr.lib.calls[n:] == [f"dvae_train_{kind}_grads", f"dvae_train_{kind}_reduce", f"dvae_train_{kind}_apply_flat_clipped"]
    assert tr.step_count == 6 and tuple(acc.grad_norm.shape) == (2,) and acc.skipped_step_count() == 0

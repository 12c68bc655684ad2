"""The float64 layer-level truths of oracle/vae_oracle.py (per-frame Itakura-Saito / KL rows, the BCE family, the squared-error
family, the reparametrisation and the MLP stack, each with its analytic gradients) against torch.float64 autograd of the reference's
own expressions: the host path of packages/models/utils.py is the reference's ATen expression (utils.py:55-118), the reparametrisation
is models.py:17-20, the stack is F.linear + torch.cat + torch's activations (models.py:57-63, 102-105, 119-122, 201-202).  This keeps
the truth of tests/test_gpu_layers_scale.py from being a restatement of the kernels' hand-written gradients."""
import numpy as np
import pytest
import torch

from oracle import vae_oracle as vo
from packages.models import utils as U

RTOL = 1e-12
SHAPES = [(3, 5, 2), (7, 37, 5)]             # (B, F, Z)
EPS = 1e-8


def close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    # elementwise: relative to the element plus the tensor's typical size (a cancelling matmul term), never to its maximum -- the forced
    # corner's 1e8-scale BCE derivative must not widen the bar of the other elements
    bar = RTOL * (np.abs(ref) + np.median(np.abs(ref)))
    assert np.all(np.abs(got - ref) <= bar), (what, float(np.max(np.abs(got - ref) / (bar / RTOL + 1e-300))))


def T(a, grad=True):
    return torch.from_numpy(np.array(a)).requires_grad_(grad)


def draws(B, F, Z):
    rng = np.random.default_rng(1000 * B + F)
    d = dict(x=rng.standard_normal((B, F)) ** 2, r=np.exp(rng.standard_normal((B, F))), mu=rng.standard_normal((B, Z)),
             lv=rng.standard_normal((B, Z)), e=rng.standard_normal((B, Z)), p=rng.random((B, F)) * 0.98 + 0.01,
             p2=rng.random((B, F)) * 0.98 + 0.01, t=rng.random((B, F)), y=rng.random((B, F)), yh=rng.random((B, F)),
             xc=rng.standard_normal((B, F)) + 1j * rng.standard_normal((B, F)), sc=rng.standard_normal((B, F)) + 1j * rng.standard_normal((B, F)),
             g_rec=rng.standard_normal(B), g_kl=rng.standard_normal(B), g=rng.standard_normal((B, Z)))
    d["p"][0, 0] = 1.0                       # the eps-inside-the-log corner
    d["t"][0, 0] = 0.0
    return d


@pytest.mark.parametrize("B,F,Z", SHAPES)
def test_rows_and_elbo(B, F, Z):
    d = draws(B, F, Z)
    x, r, mu, lv = T(d["x"], False), T(d["r"]), T(d["mu"]), T(d["lv"])
    tot, rec, kl = U.L_loss(x, r, mu, lv, EPS)
    close(vo.is_rows(d["x"], d["r"], EPS), rec.detach().numpy(), "is_rows")
    close(vo.is_rows(d["x"], d["r"], EPS), U.ikatura_saito_divergence(r, x, EPS).detach().numpy(), "isd")
    close(vo.kl_rows(d["mu"], d["lv"]), kl.detach().numpy(), "kl_rows")
    ((rec * T(d["g_rec"], False)).sum() + (kl * T(d["g_kl"], False)).sum()).backward()
    close(vo.is_rows_bwd(d["x"], d["r"], d["g_rec"]), r.grad.numpy(), "is_rows_bwd")
    dmu, dlv = vo.kl_rows_bwd(d["mu"], d["lv"], d["g_kl"])
    close(dmu, mu.grad.numpy(), "kl_rows_bwd mu")
    close(dlv, lv.grad.numpy(), "kl_rows_bwd logvar")

    r, mu, lv = T(d["r"]), T(d["mu"]), T(d["lv"])
    loss, recon, KL = U.elbo(x, r, mu, lv, EPS)
    close(vo.elbo(d["x"], d["r"], d["mu"], d["lv"], EPS), [v.item() for v in (loss, recon, KL)], "elbo")
    (0.7 * loss + 1.3 * recon - 0.4 * KL).backward()
    dr, dmu, dlv = vo.elbo_bwd_r(d["x"], d["r"], d["mu"], d["lv"], 0.7 + 1.3, 0.7 - 0.4)
    close(dr, r.grad.numpy(), "elbo dr")
    close(dmu, mu.grad.numpy(), "elbo dmu")
    close(dlv, lv.grad.numpy(), "elbo dlogvar")
    # elbo_bwd() is the same gradient taken with respect to a = log r
    da, _, _ = vo.elbo_bwd(d["x"], np.log(d["r"]), d["mu"], d["lv"], 2.0)
    close(da, r.grad.numpy() * d["r"], "elbo da")


@pytest.mark.parametrize("B,F,Z", SHAPES)
def test_bce_family(B, F, Z):
    d = draws(B, F, Z)
    p, t = T(d["p"]), T(d["t"])
    v = U.binary_cross_entropy(p, t, EPS)
    close(vo.binary_cross_entropy(d["p"], d["t"], EPS), v.item(), "bce")
    (v * 1.7).backward()
    close(vo.bce_bwd(d["p"], d["t"], EPS, 1.7), p.grad.numpy(), "bce dr")
    close(vo.bce_bwd_t(d["p"], d["t"], EPS, 1.7), t.grad.numpy(), "bce dt")
    for fn, ref, bwd in ((U.binary_cross_entropy_v2, vo.binary_cross_entropy_v2, vo.bce_v2_bwd),
                         (U.binary_cross_entropy_v3, vo.binary_cross_entropy_v3, vo.bce_v3_bwd)):
        p = T(d["p"])
        v = fn(p, EPS)
        close(ref(d["p"], EPS), v.item(), fn.__name__)
        (v * -0.6).backward()
        close(bwd(d["p"], EPS, -0.6), p.grad.numpy(), fn.__name__ + " dr")
    p1, p2, t = T(d["p"]), T(d["p2"]), T(d["t"])
    v = U.binary_cross_entropy_2classes(p1, p2, t, EPS)
    close(vo.binary_cross_entropy_2classes(d["p"], d["p2"], d["t"], EPS), v.item(), "bce2")
    (v * 2.5).backward()
    for got, ref, what in zip(vo.bce2_bwd(d["p"], d["p2"], d["t"], EPS, 2.5), (p1.grad, p2.grad, t.grad), ("dr1", "dr2", "dt")):
        close(got, ref.numpy(), "bce2 " + what)


@pytest.mark.parametrize("B,F,Z", SHAPES)
def test_squared_error_family(B, F, Z):
    d = draws(B, F, Z)
    x, y, yh = T(d["x"]), T(d["y"]), T(d["yh"])
    v = U.mean_square_error_signal(x, y, yh)
    close(vo.sqerr(0, d["x"], d["y"], d["yh"]), v.item(), "mse_signal")
    (v * 1.1).backward()
    for got, ref, what in zip(vo.sqerr_bwd(0, d["x"], d["y"], d["yh"], 1.1), (yh.grad, y.grad, x.grad), ("dyhat", "dy", "dx")):
        close(got, ref.numpy(), "mse_signal " + what)
    y, yh = T(d["y"]), T(d["yh"])
    v = U.mean_square_error_mask(y, yh)
    close(vo.sqerr(1, None, d["y"], d["yh"]), v.item(), "mse_mask")
    (v * -0.3).backward()
    dyh, dy, dx = vo.sqerr_bwd(1, None, d["y"], d["yh"], -0.3)
    assert dx is None
    close(dyh, yh.grad.numpy(), "mse_mask dyhat")
    close(dy, y.grad.numpy(), "mse_mask dy")
    yh = T(d["yh"])
    v = U.magnitude_spectrum_approxiamation_loss(T(d["xc"], False), T(d["sc"], False), yh)
    close(vo.sqerr(2, d["xc"], d["sc"], d["yh"]), v.item(), "msa")
    (v * 0.9).backward()
    dyh, dy, dx = vo.sqerr_bwd(2, d["xc"], d["sc"], d["yh"], 0.9)
    assert dy is None and dx is None
    close(dyh, yh.grad.numpy(), "msa dyhat")


@pytest.mark.parametrize("B,F,Z", SHAPES)
def test_reparam_backward(B, F, Z):
    d = draws(B, F, Z)
    mu, lv = T(d["mu"]), T(d["lv"])
    z = mu.addcmul(lv.mul(0.5).exp(), T(d["e"], False))           # models.py:17, 20
    z.backward(T(d["g"], False))
    dmu, dlv = vo.reparam_bwd(d["g"], d["lv"], d["e"])
    close(dmu, mu.grad.numpy(), "reparam dmu")
    close(dlv, lv.grad.numpy(), "reparam dlogvar")


TORCH_ACT = {0: lambda v: v, 1: torch.tanh, 2: torch.relu, 3: torch.sigmoid, 4: torch.exp}
# (widths after the input, activation codes, index of the layer without a bias or None)
STACKS = [((4,), (3,), None), ((6, 1), (2, 3), None), ((5, 4, 3), (1, 1, 4), 1), ((6, 5, 4, 2), (2, 0, 1, 3), 2), ((3, 3), (0, 0), 0)]


@pytest.mark.parametrize("B,k0,k1", [(3, 5, 0), (7, 6, 2)])
@pytest.mark.parametrize("widths,acts,nobias", STACKS)
def test_mlp_stack(B, k0, k1, widths, acts, nobias):
    rng = np.random.default_rng(B + 10 * k0 + sum(widths))
    x0 = rng.standard_normal((B, k0))
    x1 = rng.standard_normal((B, k1)) if k1 else None
    layers, fan = [], k0 + k1
    for i, (n, a) in enumerate(zip(widths, acts)):
        layers.append((rng.standard_normal((n, fan)) / np.sqrt(fan), None if i == nobias else rng.standard_normal(n) * 0.3, a))
        fan = n
    # an exact zero before a ReLU (a zero weight row and bias): torch's relu'(0) = 0
    for i, (W, b, a) in enumerate(layers):
        if a == 2 and b is not None:
            W[0], b[0] = 0.0, 0.0
    dout = rng.standard_normal((B, widths[-1]))
    tx0, tx1 = T(x0), (None if x1 is None else T(x1))
    tl = [(T(W), None if b is None else T(b)) for W, b, _ in layers]
    h = tx0 if tx1 is None else torch.cat([tx0, tx1], dim=1)
    touts = []
    for (W, b), a in zip(tl, acts):
        h = TORCH_ACT[a](torch.nn.functional.linear(h, W, b))
        touts.append(h)
    h.backward(T(dout, False))
    outs = vo.mlp_stack_fwd(x0, layers, x1)
    for i, (o, to) in enumerate(zip(outs, touts)):
        close(o, to.detach().numpy(), f"layer {i} out")
    grads, dx0, dx1 = vo.mlp_stack_bwd(x0, layers, outs, dout, x1)
    for i, ((dW, db), (W, b)) in enumerate(zip(grads, tl)):
        close(dW, W.grad.numpy(), f"layer {i} dW")
        assert (db is None) == (b is None)
        if b is not None:
            close(db, b.grad.numpy(), f"layer {i} db")
    close(dx0, tx0.grad.numpy(), "dx0")
    assert (dx1 is None) == (x1 is None)
    if x1 is not None:
        close(dx1, tx1.grad.numpy(), "dx1")

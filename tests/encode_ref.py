"""The encoder stage restated in numpy, for tests/test_encode_cpu.py, tests/test_gpu_encode.py and
tests/golden/make_encode_golden.py: the network of include/dvae.h (dvae_encode_batch) in float64, the natural scale of the rounding
error of its outputs, and the bars that the tests hold the device to.  No GPU, no library, no reference checkout.

Scale.  As in tests/classify_ref.py a float32 evaluation differs from the float64 one by a sum of rounding errors, each relative to
a partial sum bounded by the sum of the absolute products: the mass of a pre-activation.  The activation here is tanh, not relu: an
error d of the pre-activation a reaches h = tanh(a) as s d with the slope s = 1 - h^2 (linearised: the errors are ~1e-6 of a), and
tanhf itself adds a rounding of a few ulp relative to |h|.  In units of u = 2^-24, with v = [x | y]:
    m1 = |v| |W1|^T + |b1|            the mass of layer 1's pre-activation
    e1 = s1 m1 + |h1|                 the error scale of h1
    m2 = e1 |W2|^T + |h1| |W2|^T + |b2|     h1's error carried through W2, plus layer 2's own summation mass
    e2 = s2 m2 + |h2|
    M  = e2 |W|^T + |h2| |W|^T + |b|        per head (W = Wmu or Wlv)
and the error of an output element is c u M with a factor c that is a fraction of one because the errors are many, signed and
independent.  c is MEASURED on the reference's own float32 CPU evaluation, c_ref = max |out32_ref - out64| / (u M) per head over the
fixture, recorded there; the device adds the same products in another float32 order -- another draw from the same distribution --
and is allowed BAR_FACTOR = 8 times that, the factor of tests/classify_ref.py for the reason given there (the maximum of a second
draw over ~1e4 elements lies within a small factor of the first).  A wrong index, a dropped slab or a missing bias moves an output
by >= 1e-3 M, orders above.

z = mu + exp(0.5 log_var) eps: the error of log_var enters through the slope 0.5 exp(0.5 log_var) |eps|, the float32 expf, the
product and the sum each add a few ulp: bar_z = bar_mu + |eps| exp(0.5 lv64) (0.5 bar_lv + 4 u) + u |z64|."""
import numpy as np

from classify_ref import BAR_FACTOR, U32, power          # the factor is classify_ref's, not a second number


def forward64(V, w):
    """w = (W1, b1, W2, b2, Wmu, bmu, Wlv, blv) in the state_dict layout [out][in]; V [T, 513 + y_dim] = [x | y] -> float64
    (mu, log_var, h1, h2)."""
    W1, b1, W2, b2, Wm, bm, Wl, bl = (np.asarray(a, np.float64) for a in w)
    h1 = np.tanh(np.asarray(V, np.float64) @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    return h2 @ Wm.T + bm, h2 @ Wl.T + bl, h1, h2


def masses(V, w):
    """(M_mu, M_log_var) per element, the linearised error mass of the module docstring."""
    _, _, h1, h2 = forward64(V, w)
    W1, b1, W2, b2, Wm, bm, Wl, bl = (np.abs(np.asarray(a, np.float64)) for a in w)
    m1 = np.abs(np.asarray(V, np.float64)) @ W1.T + b1
    e1 = (1.0 - h1 * h1) * m1 + np.abs(h1)
    m2 = e1 @ W2.T + np.abs(h1) @ W2.T + b2
    e2 = (1.0 - h2 * h2) * m2 + np.abs(h2)
    return tuple(e2 @ W.T + np.abs(h2) @ W.T + b for W, b in ((Wm, bm), (Wl, bl)))


def inputs(P, y):
    """[x | y] as torch.cat([x, y], 1) lays it; y None or [T, 0]: x alone."""
    P = np.asarray(P)
    return P if y is None or np.asarray(y).shape[1] == 0 else np.concatenate([P, np.asarray(y, P.dtype)], axis=1)


def z64(mu64, lv64, eps):
    return mu64 + np.exp(0.5 * lv64) * np.asarray(eps, np.float64)


def bars(M_mu, M_lv, c_mu, c_lv, lv64=None, eps=None, zz=None, factor=BAR_FACTOR):
    """(bar_mu, bar_log_var, bar_z) per element; bar_z None without eps."""
    bm, bl = factor * c_mu * U32 * M_mu, factor * c_lv * U32 * M_lv
    bz = None
    if eps is not None:
        bz = bm + np.abs(np.asarray(eps, np.float64)) * np.exp(0.5 * lv64) * (0.5 * bl + 4 * U32) + U32 * np.abs(zz)
    return bm, bl, bz


def worst(got, want, bar):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / bar))


def check(name, mu, log_var, z, V, w, c_mu, c_lv, eps=None, factor=BAR_FACTOR):
    """Print the worst errors in units of the bars, then assert.  z (with eps) may be None."""
    mu64, lv64, _, _ = forward64(V, w)
    Mm, Ml = masses(V, w)
    zz = z64(mu64, lv64, eps) if eps is not None else None
    bm, bl, bz = bars(Mm, Ml, c_mu, c_lv, lv64, eps, zz, factor)
    wm, wl = worst(mu, mu64, bm), worst(log_var, lv64, bl)
    wz = worst(z, zz, bz) if z is not None else float("nan")
    print(f"{name}: worst mu error {wm:.3f} bars, worst log_var error {wl:.3f} bars, worst z error {wz:.3f} bars "
          f"(bars: mu {bm.min():.2e}..{bm.max():.2e}, log_var {bl.min():.2e}..{bl.max():.2e}; |mu| up to {np.abs(mu64).max():.3g})")
    assert np.all(np.isfinite(np.asarray(mu))) and np.all(np.isfinite(np.asarray(log_var)))
    assert wm <= 1.0, (name, "mu", wm)
    assert wl <= 1.0, (name, "log_var", wl)
    if z is not None:
        assert wz <= 1.0, (name, "z", wz)
    return wm, wl, wz


CASES = {"m1": 0, "m2_y1": 1, "m2_y513": 513}          # fixture case -> y_dim


def build_model(models, case, seed):
    """The model of a fixture case from a `packages.models.models` module (the reference's in the fixture script, this
    repository's in the tests): the seeded construction, then every Linear bias drawn N(0, 0.05) in module order (xavier init zeroes
    them, and a dropped bias would not show)."""
    import torch
    torch.manual_seed(int(seed))
    y_dim = CASES[case]
    model = models.VariationalAutoencoder([513, 16, [128, 128]]) if y_dim == 0 else models.DeepGenerativeModel([513, y_dim, 16, [128, 128]], None)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    return model


def encoder_weights(encoder):
    return [t.detach().cpu().numpy() for l in (*encoder.hidden, encoder.sample.mu, encoder.sample.log_var) for t in (l.weight, l.bias)]


def tensor_sums(model):
    return np.array([np.sum(v.detach().cpu().numpy().astype(np.float64)) for v in model.state_dict().values()])

"""The chain oracle against itself: mcem_oracle.sample_posterior in float32 (what the device chains are held to in
test_gpu_mcem.py) against the same function in float64, on the label widths 2..16 and the soft labels of mcem_cases.LABEL_CASES.
The device tests allow log ratios rtol 2e-4 / atol 2e-3, kept samples rtol 1e-5 / atol 1e-6 and 3 % of the frames to branch
differently; those bars only say something about a kernel if the float32 reference itself sits well inside them on these inputs."""
import numpy as np
import pytest

import mcem_cases as mc
from oracle import mcem_oracle as mo

NIT, BURNIN = 12, 5


@pytest.mark.parametrize("model,y_dim,N,soft", mc.LABEL_CASES, ids=[f"y{c[1]}-N{c[2]}-{'soft' if c[3] else 'binary'}" for c in mc.LABEL_CASES])
def test_float32_chain_oracle_stays_inside_the_device_bars(model, y_dim, N, soft):
    params, prefix, X2, y, Z, g, W, H, rng = mc.chain_inputs(model, y_dim, N, 5, soft=soft)
    if soft:
        assert ((y > 0) & (y < 1)).mean() > 0.99 and np.unique(y).size > 0.9 * y.size      # fractional labels, not binary ones in disguise
    noise = rng.standard_normal((NIT, 16, N)).astype(np.float32)
    logu = np.log(rng.random((NIT, N)).astype(np.float32))
    Vb = (W @ H).astype(np.float32)
    Zs32, tp32, ta32 = mo.sample_posterior(params, prefix, Z, y, g, Vb, X2, noise, logu, BURNIN, return_trace=True)
    Zs64, tp64, ta64 = mo.sample_posterior(params, prefix, Z, y, g, Vb, X2, noise, logu, BURNIN, dtype=np.float64, return_trace=True)
    assert Zs32.dtype == np.float32 and Zs64.dtype == np.float64
    diff = ta32 != ta64
    first = np.where(diff.any(axis=0), diff.argmax(axis=0), NIT)
    worst = 0.0
    for n in range(N):                                          # log ratios while both chains are in the same state
        k = min(first[n] + 1, NIT)
        worst = max(worst, float(np.max(np.abs(tp32[:k, n] - tp64[:k, n]) / (2e-3 + 2e-4 * np.abs(tp64[:k, n])))))
    same = first == NIT
    dz = float(np.abs(Zs32[same] - Zs64[same]).max())
    print(f"y_dim {y_dim} soft {soft}: same decisions {same.mean():.3f}, worst log ratio {worst:.4f} of the bar, kept samples {dz:.2e}, "
          f"acceptance {ta64.mean():.3f}")
    # float32 sums of 513 terms of size ~5 carry ~1e-4 of absolute noise, a twentieth of the bar's atol: a tenth of the bar leaves the
    # kernels nine tenths of it
    assert worst <= 0.1
    assert same.mean() >= 0.97
    np.testing.assert_allclose(Zs32[same], Zs64[same], rtol=1e-5, atol=1e-6)
    assert 0.02 < ta64.mean() < 0.98                            # the device tests' "the chain moves and rejects" check still bites

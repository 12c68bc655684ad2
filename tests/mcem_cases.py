"""MCEM parity cases shared by tests/golden/make_mcem_golden.py (runs the REFERENCE) and the parity tests.
Inputs are regenerated from seeds; the fixture stores a checksum of them."""
import numpy as np

EPS = np.finfo(float).eps          # scripts/evaluate_ntcd_M2.py: eps = np.finfo(float).eps

DIMS = {
    "M1": dict(x_dim=513, y_dim=0, z_dim=16, h_dim=(128, 128)),
    "M2": dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128)),
    "M2_info": dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128)),
}

CASES = [
    dict(name="M1", model="M1", N=45, K=10, niter=2, n_e=3, b_e=4, n_wf=4, b_wf=3, seed=11, wscale=1.0),
    dict(name="M2_y1", model="M2", N=45, K=10, niter=2, n_e=3, b_e=4, n_wf=4, b_wf=3, seed=12, wscale=1.0),
    dict(name="M2v3_y1", model="M2_info", N=70, K=10, niter=2, n_e=3, b_e=4, n_wf=4, b_wf=3, seed=13, wscale=1.5),
]


def effective_counts(case):
    """(nsamples, burnin) actually run per E-step and for the Wiener filter.  MCEM_M1 passes
    (Z, nsamples, burnin) into sample_posterior(Z, y, nsamples=10, burnin=30) (mcem.py:207,297-298,314-315):
    nsamples <- its burnin argument, burnin <- the default 30."""
    if case["model"] == "M1":
        return case["b_e"], 30, case["b_wf"], 30
    return case["n_e"], case["b_e"], case["n_wf"], case["b_wf"]


def make_utterance(case):
    """Synthetic complex STFTs X (mixture), S (clean), (F, N) complex64, and labels y (y_dim, N) float32."""
    rng = np.random.default_rng(case["seed"] + 500)
    F, N = 513, case["N"]
    env = np.exp(rng.standard_normal((F, 1)) * 0.7 - 1.0) * np.exp(rng.standard_normal((1, N)) * 0.5)
    S = (np.sqrt(env / 2) * (rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N)))).astype(np.complex64)
    noise = (0.3 * (rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N)))).astype(np.complex64)
    X = (S + noise).astype(np.complex64)
    ydim = DIMS[case["model"]]["y_dim"]
    y = (rng.random((max(ydim, 1), N)) > 0.4).astype(np.float32)
    return X, S, (y if ydim else None)


def chain_inputs(model, y_dim, N, seed, wscale=1.0, soft=False):
    """Inputs of one Metropolis-Hastings chain launch over N frames, shared by the chain tests on the device (test_gpu_mcem.py)
    and the float32-against-float64 check of the oracle on the same inputs (test_mcem_oracle_chain.py).  Labels are binary, or
    with soft=True uniform in [0, 1) (what McemBatch.init_parameters(..., use="soft") hands over); both take the same number of
    draws, so everything after them is the same either way.
    -> params, decoder prefix, X2 (513, N), y (y_dim, N) or None, Z (16, N), g (N), W (513, 10), H (10, N), the generator."""
    import golden_util as gu
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, seed, wscale)
    prefix = "enc_dec_clf.decoder." if model == "M2_info" else "decoder."
    rng = np.random.default_rng(seed + 77)
    X2 = (rng.standard_normal((513, N)) ** 2 * np.exp(rng.standard_normal((513, 1)) - 1)).astype(np.float32) + 1e-4
    y = None
    if y_dim:
        u = rng.random((y_dim, N))
        y = u.astype(np.float32) if soft else (u > 0.5).astype(np.float32)
    Z = rng.standard_normal((16, N)).astype(np.float32)
    g = np.exp(0.2 * rng.standard_normal(N)).astype(np.float32)
    W = np.maximum(rng.random((513, 10)), 1e-6).astype(np.float32)
    H = np.maximum(rng.random((10, N)), 1e-6).astype(np.float32)
    return params, prefix, X2, y, Z, g, W, H, rng


# label widths between the tested 1 and 513 (zero-padded to 16 rows on the device), and fractional labels: (model, y_dim, N, soft)
LABEL_CASES = [("M2", 2, 70, False), ("M2", 7, 45, False), ("M2", 15, 70, False), ("M2", 16, 45, False),
               ("M2", 1, 70, True), ("M2", 7, 45, True), ("M2", 513, 45, True)]


def checksum(X, S, y):
    tot = float(np.abs(X).astype(np.float64).sum() + np.abs(S).astype(np.float64).sum())
    return tot + (float(y.sum()) if y is not None else 0.0)

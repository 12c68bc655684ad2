"""Geometry cases of the generic Metropolis-Hastings chain (csrc/mcem_generic.hip), shared by the CPU check of the oracle on them
(test_mcem_generic_cpu.py) and the device tests (test_gpu_mcem_generic.py).

(model, y_dim, z_dim, h_dim, N): each limit of dvae_mcem_plan_dims (z_dim 1 and 128, hidden widths 1 and 512, y_dim 0 and 513), sizes
off every multiple of 4 and 16, frame counts either side of a 16-frame tile, and the reference's own decoder.  h_dim is the
constructor's list: the decoder runs it reversed (z + y -> h_dim[1] -> h_dim[0] -> 513)."""
import functools

import numpy as np

import golden_util as gu
from oracle import mcem_oracle as mo

CASES = [
    ("M1", 0, 32, (256, 64), 45),
    ("M2", 1, 32, (256, 64), 45),
    ("M2", 1, 5, (48, 200), 33),
    ("M2", 513, 64, (16, 16), 17),
    ("M1", 0, 1, (1, 1), 33),
    ("M2", 3, 17, (129, 127), 70),
    ("M1", 0, 128, (512, 512), 17),
    ("M2", 1, 16, (128, 128), 45),
]
IDS = [f"{m}-y{y}-z{z}-h{h[0]}x{h[1]}-N{n}" for m, y, z, h, n in CASES]
NIT, BURNIN, SEED = 40, 30, 11
# what chain_kind refuses: (y_dim, z_dim, h_dim, x_dim)
REFUSED = {"three hidden layers": (1, 16, (128, 128, 128), 513), "257 bins": (1, 16, (128, 128), 257), "z_dim 129": (0, 129, (128, 128), 513),
           "h 513": (1, 16, (513, 128), 513), "h 513 (second)": (0, 16, (128, 513), 513)}


def dims_of(y_dim, z_dim, h_dim, x_dim=513):
    return dict(x_dim=x_dim, y_dim=y_dim, z_dim=z_dim, h_dim=tuple(h_dim))


@functools.lru_cache(maxsize=None)
def chain_inputs(model, y_dim, z_dim, h_dim, N, seed=SEED, nit=NIT):
    """The inputs of mcem_cases.chain_inputs (the same distributions in the same draw order) for a decoder of any size: Z has z_dim
    rows; then the chain's draws.  -> dict(params, X2, y, Z, g, Vb, noise, logu); treat as read-only (shared between tests)."""
    params = gu.make_params(model, dims_of(y_dim, z_dim, h_dim), seed)
    rng = np.random.default_rng(seed + 77)
    X2 = (rng.standard_normal((513, N)) ** 2 * np.exp(rng.standard_normal((513, 1)) - 1)).astype(np.float32) + 1e-4
    y = (rng.random((y_dim, N)) > 0.5).astype(np.float32) if y_dim else None
    Z = rng.standard_normal((z_dim, N)).astype(np.float32)
    g = np.exp(0.2 * rng.standard_normal(N)).astype(np.float32)
    W = np.maximum(rng.random((513, 10)), 1e-6).astype(np.float32)
    H = np.maximum(rng.random((10, N)), 1e-6).astype(np.float32)
    noise = rng.standard_normal((nit, z_dim, N)).astype(np.float32)
    logu = np.log(rng.random((nit, N)).astype(np.float32))
    out = dict(params=params, X2=X2, y=y, Z=Z, g=g, Vb=(W @ H).astype(np.float32), noise=noise, logu=logu)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def columns(inp, cols):
    """The same inputs on a subset of the frames (frames are independent given g and Vb)."""
    cols = np.asarray(cols)
    return dict(params=inp["params"], X2=inp["X2"][:, cols], y=None if inp["y"] is None else inp["y"][:, cols], Z=inp["Z"][:, cols], g=inp["g"][cols],
                Vb=inp["Vb"][:, cols], noise=inp["noise"][:, :, cols], logu=inp["logu"][:, cols])


def oracle32(inp, burnin=BURNIN):
    """The chain oracle in float32 -> Zs, log ratios, decisions."""
    return mo.sample_posterior(inp["params"], "decoder.", inp["Z"], inp["y"], inp["g"], inp["Vb"], inp["X2"], inp["noise"], inp["logu"], burnin,
                               return_trace=True)

"""The generic Metropolis-Hastings chain's CPU side: chain_kind on host modules, and the chain oracle against itself on the
geometry cases of mcem_generic_cases.py -- the float32 oracle held to the float64 one under the bars the device tests use
(test_gpu_mcem_stream.check_chain: log ratios rtol 2e-4 / atol 2e-3 in the same state, >= 97 % of the frames with the same decisions,
kept samples rtol 1e-5 / atol 1e-6, acceptance inside (0.02, 0.98)).  Those bars only say something about a kernel if float32
arithmetic itself sits well inside them at these sizes."""
import importlib

import numpy as np
import pytest

import mcem_generic_cases as gc
from impl_modules import build_model
from test_gpu_mcem_stream import bar_units, check_chain

mcem_dev = importlib.import_module("disentangled-vae_amd.mcem")


def test_chain_kind_reads_layer_shapes_of_host_modules():
    ref = build_model("M2", gc.dims_of(1, 16, (128, 128)))
    assert mcem_dev.chain_kind(ref.decoder, 1) == "resident" and mcem_dev.decoder_supported(ref.decoder, 1)
    assert mcem_dev.chain_kind(build_model("M1", gc.dims_of(0, 16, (128, 128))).decoder, 0) == "resident"
    for model, y_dim, z_dim, h_dim, _ in gc.CASES:
        dec = build_model(model, gc.dims_of(y_dim, z_dim, h_dim)).decoder
        want = "resident" if (z_dim, tuple(h_dim)) == (16, (128, 128)) and (y_dim <= 16 or y_dim == 513) else "generic"
        assert mcem_dev.chain_kind(dec, y_dim) == want, (model, y_dim, z_dim, h_dim)
        assert mcem_dev.decoder_supported(dec, y_dim) == (want == "resident")
    # label widths between 17 and 512 on the reference's decoder: the generic chain
    assert mcem_dev.chain_kind(build_model("M2", gc.dims_of(40, 16, (128, 128))).decoder, 40) == "generic"
    for what, (y_dim, z_dim, h_dim, x_dim) in gc.REFUSED.items():
        dec = build_model("M2" if y_dim else "M1", gc.dims_of(y_dim, z_dim, h_dim, x_dim)).decoder
        assert mcem_dev.chain_kind(dec, y_dim) is None, what
        assert not mcem_dev.decoder_supported(dec, y_dim), what


@pytest.mark.parametrize("model,y_dim,z_dim,h_dim,N", gc.CASES, ids=gc.IDS)
def test_float32_chain_oracle_stays_inside_the_device_bars(model, y_dim, z_dim, h_dim, N):
    inp = gc.chain_inputs(model, y_dim, z_dim, h_dim, N)
    Zs, tp, ta = gc.oracle32(inp)
    assert Zs.dtype == np.float32 and Zs.shape == (N, gc.NIT - gc.BURNIN, z_dim)
    check_chain(f"float32 oracle {model} y{y_dim} z{z_dim} h{h_dim}", inp["params"], inp, Zs, tp, ta, gc.BURNIN)
    # and well inside: measured log ratio <= 0.004 of its bar, kept samples <= 0.21 of theirs, the same decisions for every frame,
    # acceptance 0.56 .. 0.96.  A tenth / a half of the bars leaves the kernels the rest.
    from oracle import mcem_oracle as mo
    Zs64, tp64, ta64 = mo.sample_posterior(inp["params"], "decoder.", inp["Z"], inp["y"], inp["g"], inp["Vb"], inp["X2"], inp["noise"], inp["logu"],
                                           gc.BURNIN, dtype=np.float64, return_trace=True)
    same = (ta == ta64).all(axis=0)                             # frames whose two chains took the same decisions throughout
    assert same.mean() >= 0.97
    assert bar_units(tp[:, same], tp64[:, same], 2e-4, 2e-3) <= 0.1
    assert bar_units(Zs[same], Zs64[same], 1e-5, 1e-6) <= 0.5

"""The operand stream of the weight-gradient kernel (csrc/train_wgrad.hip, wgrad4_kernel: buffer loads through one resource per operand
matrix and plane, a ring of k-steps whose A rows are re-requested behind their own MFMAs) at every edge of its loops, against float64.

A wave of the kernel owns a quarter of its slice's k-steps (16 frames each under the bf16 policies, 8 under fp32).  Its loop runs whole
laps of the ring (2 k-steps under bf16x3, 4 under bf16 and fp32) and then the slice's remaining k-steps on the fragments the last
requests left in the ring; every request past the range re-reads the last k-step of the matrix.  The cases are the smallest shapes that
reach each edge -- frames are padded to 128, a slice to 64 frames (32 under fp32), so a wave's k-steps under bf16x3 / bf16 (fp32) are:

  frames   ksplit   k-steps per wave
  33       3        1, 1, 0     (2, 2, 0)   the third slice starts at the padded batch's end: an empty range whose prologue requests
                                            must still name a k-step of the matrix; 33 is no multiple of 16 or 32: a ragged last k-step
  100      1        2           (4)         one whole lap under bf16x3
  100      2        1           (2)         no lap: the tail alone
  300      2        3           (6)         a lap and a tail; 300 is no multiple of 16 or 32
  600      2        5           (10)        two laps and a tail (bf16 / fp32: one lap of four and a tail of one / two laps and two)
  600      3        4, 4, 2     (7, 7, 6)   slices of different length in one launch

M1 (x-fed blocks only), M2 with one label (blocks of 1, 2 and 4 B tiles, a 1-column label tile) and M2 with 513 labels (17 label tiles:
four blocks of 4 and one of 1; 513 output rows: the one-A-row blocks; the heads' one-tile block in every model).  Binary labels store
and multiply the hi plane only, real-valued labels both planes (bf16x3).

Bounds: those of tests/test_gpu_fused.py::test_fused_step_vs_oracle, unchanged -- bf16x3: losses 1e-5 relative, every gradient tensor
within X3_TOL of its maximum; fp32: 1e-4 on both; bf16: losses 2e-3, gradients within 0.3 of the tensor's maximum.  One float64 step
per (model, labels, frames) is computed once and shared by the precisions and slice counts."""
import functools
import importlib

import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_fused import X3_TOL, _oracle_step, _relmax

pytestmark = pytest.mark.gpu
trainer = importlib.import_module("disentangled-vae_amd.trainer")

# (model, y_dim, frames, ksplit, real-valued labels)
CASES = [
    ("M2", 513, 33, 3, False),
    ("M2", 513, 100, 1, False),
    ("M2", 513, 100, 2, True),
    ("M2", 513, 300, 2, True),
    ("M2", 513, 600, 2, False),
    ("M2", 513, 600, 3, True),
    ("M2", 1, 33, 3, True),
    ("M2", 1, 100, 1, True),
    ("M2", 1, 300, 2, False),
    ("M2", 1, 600, 2, True),
    ("M1", 0, 33, 3, False),
    ("M1", 0, 100, 2, False),
    ("M1", 0, 300, 2, False),
    ("M1", 0, 600, 3, False),
]


def _dims(y_dim):
    return dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))


@functools.lru_cache(maxsize=None)
def _case(model, y_dim, B, soft):
    """inputs and the float64 step of one case (read-only: shared by every test that names the case)"""
    dims = _dims(y_dim)
    params = gu.make_params(model, dims, 21)
    x, y, e = gu.make_batch(dims, B, 22 + B)
    if soft:
        y = np.random.default_rng(B).random(y.shape).astype(np.float32)      # labels in (0, 1) with full fp32 mantissas: both planes
    f64 = lambda a: None if a is None else a.astype(np.float64)
    out, grads, _ = _oracle_step(model, dims, params, f64(x), f64(y), f64(e))
    for a in (x, y, e):
        if a is not None:
            a.setflags(write=False)
    return params, (x, y, e), np.array([out["loss"], out["recon"], out["kl"]]), grads


def _step(model, y_dim, B, ksplit, precision, params, batch):
    tr = trainer.Trainer(model, _dims(y_dim), params, batch=B, precision=precision, ksplit=ksplit)
    assert tr.plan.ksplit == ksplit and tr.plan.reserved0 == 0              # the uniform slices the case was chosen for
    t = lambda a: None if a is None else torch.from_numpy(a.copy()).cuda()
    losses = tr.step(*(t(a) for a in batch)).cpu().numpy().copy()
    return losses, tr.grads_numpy()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp32"])
@pytest.mark.parametrize("model,y_dim,B,ksplit,soft", CASES, ids=[f"{m}-y{y}-B{b}-ks{k}-{'real' if s else 'binary'}" for m, y, b, k, s in CASES])
def test_operand_stream_at_its_loop_edges_vs_oracle(model, y_dim, B, ksplit, soft, precision):
    params, batch, ref, grads = _case(model, y_dim, B, soft)
    losses, g = _step(model, y_dim, B, ksplit, precision, params, batch)
    ltol, gtol = {"fp32": (1e-4, 1e-4), "bf16x3": (1e-5, X3_TOL), "bf16": (2e-3, 0.3)}[precision]
    fig = {k: _relmax(g[k], np.asarray(grads[k], np.float64).reshape(g[k].shape)) for k in grads}
    worst = max(fig, key=fig.get)
    print(f"wgrad stream[{model},y{y_dim},B{B},ks{ksplit},{'real' if soft else 'binary'},{precision}]: loss rel err "
          f"{np.max(np.abs(losses - ref) / np.abs(ref)):.2e}, worst grad relmax {fig[worst]:.2e} ({worst})")
    np.testing.assert_allclose(losses, ref, rtol=ltol)
    for k in grads:
        assert np.all(np.isfinite(g[k])), k
        assert fig[k] < gtol, (k, fig[k])


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_operand_stream_is_bitwise_reproducible(precision):
    """the same case twice, a fresh plan and workspace each time: bit-equal losses and gradients"""
    model, y_dim, B, ksplit, soft = "M2", 513, 600, 3, True
    params, batch, _, _ = _case(model, y_dim, B, soft)
    l0, g0 = _step(model, y_dim, B, ksplit, precision, params, batch)
    l1, g1 = _step(model, y_dim, B, ksplit, precision, params, batch)
    np.testing.assert_array_equal(l0, l1)
    for k in g0:
        np.testing.assert_array_equal(g0[k], g1[k], err_msg=k)

"""The fused train step's weight and bias gradients PER INPUT COLUMN against float64 (tests/grad_columns.py: statistic, restatements,
bound, inputs; tests/test_grad_columns_cpu.py shows on the CPU what the tensor-level figure of the other tests cannot see).

Every tensor, every column, worst and median column, under fp32, bf16x3 and bf16, through trainer.Trainer(...).step and grads_numpy() on
the default library and the default plan, a fresh Trainer per test.  The bound is the rule of grad_columns.py, made in the test from the
CPU restatements of that very case; a column whose float64 gradient is identically zero must be exactly zero.  Cases: the bench family
(golden_util.make_batch) at 8192 frames (M1, M2 y 513: the sliced schedule), M2 y 1 at 1000 (31.25 tiles, the 1-column label tile),
M2 y 513 at 33 (a partial tile; 513 + 513 columns = 33 column tiles, the last holding 2) and at 1 frame; the speech-like family (bins
falling 60 dB) at 1000, 8192 and 33 frames; M2_info (alpha 0.5, beta 10, gamma 1) on the speech-like family / 64, tie-free, at 1000 and
8192 frames.  The 20 000-frame tile loop stays with tests/test_gpu_fused.py.

Measured on the MI355X (33 tests, 13 s of wall time with the CPU references).  Worst ratio of a figure (worst or median column of any
tensor) to its bound, fp32 / bf16x3 / bf16 -- a device that errs exactly as the restatements do reaches 0.25:
  bench        M1 8192: 0.36 / 0.31 / 0.33     M2 y 513 8192: 0.35 / 0.33 / 0.30     M2 y 1 1000: 0.30 / 0.52 / 0.37
               M2 y 513 33: 0.36 / 0.56 / 0.28     M2 y 513 1 frame: 0.88 / 0.50 / 0.34
  speech-like  M1 1000: 0.32 / 0.41 / 0.30     M2 y 513 1000: 0.39 / 0.30 / 0.30     M2 y 1 8192: 0.35 / 0.30 / 0.29
               M2 y 513 33: 0.51 / 0.39 / 0.31
  M2_info      1000 (108 frames replaced): 0.52 / 0.88 / 0.27     8192 (989 replaced): 0.56 / 0.67 / 0.51
No ratio above 1, no zero column that is not exactly zero (35.5 % of encoder layer 1's columns and 68.8 % of decoder layer 1's at one
frame).
On encoder layer 1's weight at 8192 frames under bf16x3: bench M2 y 513 worst column 2.8e-4 of its own maximum (column 120), median
6.8e-6, where the tensor-level figure is 8.9e-6; speech-like M2 y 1 worst 9.0e-5 (column 86), median 9.7e-6, tensor-level 4.9e-6: both
at a quarter of their bounds, i.e. the device errs per column as the split-bf16 model of the fp32 x does (csrc/fused_tiles.hpp, struct X16).
The highest: 0.88 under fp32 at ONE frame (mu / log_var weight, column 74: the relative float32 error of one tanh output whose
pre-activation nearly cancels; see grad_columns.py) and 0.88 under bf16x3 on the auxiliary net's output-layer weight at 1000 frames.
Two details of the float32 restatement had to be added to close three cases of the first device run, both written out in grad_columns.py:
its second summation order (k-steps through one accumulator, slab sums: M2 y 513 at 1 frame under fp32 was at 1.94 of the one-order bound)
and the floor of 2^-24 under the float32 term (the one-element output-layer bias of M2_info's classifier: 5.8e-8 and 1.8e-7 off on the
device, under two ulps, against 4 x 9e-9).  The margin of 4 did not move; no device figure entered a bound.

Scratch breakages of the product code (one at a time, nothing of them committed; the module was run once against each library):
  a  the x operand of the layer-1 weight gradient without its lo plane under bf16x3 (csrc/rows_common.hpp, xstash_reload: fl = 0)
       11 of 33 fail: every bf16x3 case, 3.2 ... 86 x the bound (bench M2 y 513 8192: worst column 4.4e-3, median exactly at its bound)
  b  nvalid of every tensor's last column tile one short (csrc/train_fused.hip, fill_tables: addB)
       33 of 33 fail: the last column of every weight tensor is never written (figure 1.0)
test_fused_step_vs_oracle as it stood was NOT run against the two libraries; its verdict is reasoned from the tensor-level figure this
module prints beside each column figure, measured on them: under (a) encoder layer 1's weight is 1.2e-3 ... 3.4e-3 of its maximum off on
the bench cases that test shares (its bf16x3 bound is 5e-5), under (b) 0.66 ... 0.95 on some tensor of every case: it fails both, as it
should -- a whole plane or a whole column of EVERY tensor is not subtle.  What it cannot see is the same fault confined to quiet columns:
tests/test_grad_columns_cpu.py seeds those (lo plane missing from bin 256 on: 2e-5 at tensor level, 3e-3 per column; one unwritten quiet
bin; label columns x 1.01; one frame missing from bins 480 .. 511) and shows each under 5e-5 at tensor level and over the column bound.
"""
import importlib

import numpy as np
import pytest
import torch

import grad_columns as gc

pytestmark = pytest.mark.gpu
trainer = importlib.import_module("disentangled-vae_amd.trainer")

CASES = [("bench", "M1", 0, 8192), ("bench", "M2", 513, 8192), ("bench", "M2", 1, 1000), ("bench", "M2", 513, 33), ("bench", "M2", 513, 1),
         ("speech", "M1", 0, 1000), ("speech", "M2", 513, 1000), ("speech", "M2", 1, 8192), ("speech", "M2", 513, 33),
         ("info", "M2_info", 1, 1000), ("info", "M2_info", 1, 8192)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("family,model,y_dim,B", CASES, ids=["{}-{}-y{}-B{}".format(*c) for c in CASES])
def test_fused_step_gradients_per_column(family, model, y_dim, B, precision):
    r = gc.reference(family, model, y_dim, B)                    # truth and restatements: once per case, shared by the precisions
    if model == "M2_info":
        print(f"tie-free batch: {r.replaced} of {B} frames replaced, smallest ReLU margin left {r.margin:.2e}")
        assert r.margin >= gc.TIE_DELTA and r.replaced < B // 4
    kw = dict(zip(("alpha", "beta", "gamma"), gc.INFO_WEIGHTS)) if model == "M2_info" else {}
    tr = trainer.Trainer(model, r.dims, r.params, batch=B, precision=precision, **kw)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    losses = tr.step(t(r.x), t(r.y), t(r.e)).cpu().numpy()
    assert np.all(np.isfinite(losses))
    g = tr.grads_numpy()
    assert set(g) == set(r.truth)
    fails, top = gc.check(g, r, precision, label=f"[{family} {model} y{y_dim} B{B} {precision}]")
    print(f"[{family} {model} y{y_dim} B{B} {precision}] worst ratio to the bound: {top:.3f}")
    assert not fails, fails

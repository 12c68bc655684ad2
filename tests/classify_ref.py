"""The classifier stage restated in numpy, for tests/test_classify_cpu.py, tests/test_gpu_classify.py and
tests/golden/make_classify_golden.py: the network of include/dvae.h (dvae_classify_batch) in float64, the natural scale of the
rounding error of its logits, the bars that the tests hold the device to, and f1_loss's ratios from integer counts.  No GPU, no
library, no reference checkout.

Scale.  A float32 evaluation of the three layers differs from the float64 one by a sum of rounding errors, each relative to a
partial sum that is bounded by the sum of the absolute products.  Propagated through the layers (relu has slope at most 1) that sum
is the mass
    m1 = P |W1|^T + |b1|,  m2 = m1 |W2|^T + |b2|,  M = m2 |W3|^T + |b3|
per output element, and the error is c u M with u = 2^-24 and a factor c that a worst-case analysis puts near the chain length
(useless: 0.16 in logit space on the fixture's inputs) and that is in fact a small fraction of one, because the errors are many,
signed and independent.  c is therefore MEASURED, on the reference's own float32 CPU evaluation: c_ref = max |logit32_ref -
logit64| / (u M) over the fixture, recorded there.  The device adds the same products in another float32 order, so its error is
another draw from the same distribution, and over ~1e5 elements the maximum of a second draw is within a small factor of the first:
the tests allow 8 c_ref u M.  A wrong index, a dropped slab or a missing bias moves a logit by >= 1e-3 M, five orders above.

soft = sigmoid(logit) has slope <= 1/4, and a float32 sigmoid (one exp, one add, one divide, each within a few ulp of values <= 1)
adds at most 4 u: bar_soft = bar_logit / 4 + 4 u.  hard = soft > 0.5 can legitimately differ from the float64 decision only where
the logit is within the combined error of 0: |logit64| <= 2 bar_logit + 4 u; elements there are excluded, and at most 0.1 % of a case
may be."""
import numpy as np

U32 = 2.0 ** -24
BAR_FACTOR = 8.0
EXCLUDED_CAP = 1e-3


def power(X):
    """The classifier's input from complex64 frames [T, 513]: the reference's float32 `np.abs(X) ** 2`."""
    return (np.abs(np.asarray(X, np.complex64)) ** 2).astype(np.float32)


def logits64(P, w):
    """w = (W1, b1, W2, b2, W3, b3) in the state_dict layout [out][in]; P [T, 513] -> float64 logits [T, y_dim]."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float64) for a in w)
    h1 = np.maximum(np.asarray(P, np.float64) @ W1.T + b1, 0.0)
    h2 = np.maximum(h1 @ W2.T + b2, 0.0)
    return h2 @ W3.T + b3


def mass(P, w):
    W1, b1, W2, b2, W3, b3 = (np.abs(np.asarray(a, np.float64)) for a in w)
    m1 = np.abs(np.asarray(P, np.float64)) @ W1.T + b1
    m2 = m1 @ W2.T + b2
    return m2 @ W3.T + b3


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def bars(M, c_ref, factor=BAR_FACTOR):
    """(bar_logit, bar_soft, margin of the hard decision) per element."""
    bl = factor * c_ref * U32 * M
    return bl, 0.25 * bl + 4 * U32, 2 * bl + 4 * U32


def check(name, logit, soft, hard, z64, M, c_ref, factor=BAR_FACTOR):
    """Print the worst errors in units of the bars and the excluded share, then assert.  logit may be None."""
    bl, bs, margin = bars(M, c_ref, factor)
    worst_l = float(np.max(np.abs(np.asarray(logit, np.float64) - z64) / bl)) if logit is not None else float("nan")
    worst_s = float(np.max(np.abs(np.asarray(soft, np.float64) - sigmoid64(z64)) / bs))
    excluded = np.abs(z64) <= margin
    share = float(np.mean(excluded))
    wrong = int(np.sum(((np.asarray(hard) != 0) != (z64 > 0)) & ~excluded))
    print(f"{name}: worst logit error {worst_l:.3f} bars, worst soft error {worst_s:.3f} bars, excluded share {share:.2e}, "
          f"hard labels off outside it {wrong} of {excluded.size}")
    assert share <= EXCLUDED_CAP, (name, share)
    if logit is not None:
        assert worst_l <= 1.0, (name, worst_l)
    assert worst_s <= 1.0, (name, worst_s)
    assert wrong == 0, (name, wrong)
    assert set(np.unique(np.asarray(hard))) <= {0.0, 1.0}
    return worst_l, worst_s, share


def counts(pred, truth):
    """int64 (tp, tn, fp, fn) over all elements; an element counts as 1 when it is not zero."""
    p, t = np.asarray(pred) != 0, np.asarray(truth) != 0
    return np.array([np.sum(p & t), np.sum(~p & ~t), np.sum(p & ~t), np.sum(~p & t)], np.int64)


def f1_from_counts(c, epsilon=1e-8):
    """float32 (accuracy, precision, recall, f1) [..., 4] from int64 counts [..., 4] (tp, tn, fp, fn): the counts to float32, then
    f1_loss's four expressions as written, every operation in float32 (epsilon as a float32, as a tensor-scalar operation takes it)."""
    c = np.asarray(c, np.int64).astype(np.float32)
    tp, tn, fp, fn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    e, two = np.float32(epsilon), np.float32(2)
    accuracy = (tp + tn) / (tp + tn + fp + fn + e)
    precision = tp / (tp + fp + e)
    recall = tp / (tp + fn + e)
    f1 = two * (precision * recall) / (precision + recall + e)
    return np.stack([accuracy, precision, recall, f1], axis=-1).astype(np.float32)

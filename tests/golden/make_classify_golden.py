"""Golden outputs of the reference's Classifier (packages/models/models.py:41-63) and f1_loss (packages/models/utils.py:120-159) on
seeded inputs.  Build-container only (imports /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_classify_golden.py
Output: tests/golden/classify_golden.part0.npz (the frames, the truths, the y_dim 1 case) and .part1.npz (the y_dim 513 case).

Inputs: a few short synthetic utterances (the `speechlike` generator of tests/test_gpu_mix.py, peak-normalised), their 1024 / 256
periodic-Hann STFT computed here in float64 and stored as complex64 frames [sum T_u, 513].  Per case the reference's Classifier
([513, [128, 128], y_dim], default nn.Linear init after torch.manual_seed(seed)) runs on the CPU in float32 on
`(np.abs(X) ** 2).astype(np.float32)`.  The weights are NOT stored (the 513-wide set alone is 590 kB): the seed is, with each
tensor's float64 sum, and the tests rebuild them with the same construction (this repository's Classifier draws the same stream).

Recorded per case: the reference's float32 logits, soft (whole: 118 x 513 floats are 242 kB) and hard = soft > 0.5 (as bytes), f1_loss per
utterance of the hard labels against a recorded truth (an energy gate, so that both classes appear; bytes), the confusion counts, and
c_ref = max |logit32 - logit64| / (u M) with the float64 network and the mass M of tests/classify_ref.py.  Asserted here and stored:
the positive share of each case lies in [0.2, 0.8] (untrained weights can be one-sided; SEEDS were picked for that), and the
reference's own hard labels match the float64 decision outside the excluded near-threshold set, whose share stays under the cap."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import numpy as np
import torch

import classify_ref as CR
from packages.models.models import Classifier
from packages.models.utils import f1_loss

LENGTHS = [1024 + 256 * 32, 1024 + 256 * 64, 1024 + 256 * 19]         # 33, 65 and 20 frames
SEEDS = {1: 1, 513: 1}            # torch.manual_seed per y_dim: positive shares 0.38 and 0.50 (seeds 2 and 3 are one-sided at y_dim 1)
EPS = 1e-8


def speechlike(n, seed):
    rng = np.random.default_rng(seed)
    env = np.repeat((rng.random(n // 800 + 1) > 0.4).astype(np.float64), 800)[:n] + 0.05
    return env * rng.standard_normal(n) * 0.1


def frames_c64(x):
    x = x / np.max(np.abs(x))
    T = 1 + (len(x) - 1024) // 256
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    seg = np.stack([x[t * 256:t * 256 + 1024] * w for t in range(T)])
    return np.fft.rfft(seg, axis=1).astype(np.complex64)


def run_case(y_dim, seed, P):
    torch.manual_seed(seed)
    clf = Classifier([513, [128, 128], y_dim])
    with torch.no_grad():
        x = torch.from_numpy(P)
        soft = clf(x).numpy()
        h = x
        for layer in clf.hidden:
            h = torch.relu(layer(h))
        logit = clf.output_layer(h).numpy()
    w = [t.detach().numpy() for t in (clf.hidden[0].weight, clf.hidden[0].bias, clf.hidden[1].weight, clf.hidden[1].bias,
                                      clf.output_layer.weight, clf.output_layer.bias)]
    return w, logit, soft


def main():
    X = [frames_c64(speechlike(n, 11 + u)) for u, n in enumerate(LENGTHS)]
    counts = np.array([len(x) for x in X], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    frames = np.concatenate(X)
    P = CR.power(frames)
    energy = P.sum(axis=1)
    truth = {1: (energy > np.median(energy)).astype(np.float32)[:, None],
             513: (P > np.median(P, axis=0, keepdims=True)).astype(np.float32)}
    parts = [{"frames": frames, "counts": counts, "epsilon": np.array(EPS)}, {}]
    for part, y_dim in zip(parts, (1, 513)):
        seed = SEEDS[y_dim]
        w, logit, soft = run_case(y_dim, seed, P)
        share = float(np.mean(soft > 0.5))
        assert 0.2 <= share <= 0.8, f"y_dim {y_dim}, seed {seed}: positive share {share:.3f}: pick another seed"
        hard = (soft > 0.5).astype(np.float32)
        z64, M = CR.logits64(P, w), CR.mass(P, w)
        c_ref = float(np.max(np.abs(logit.astype(np.float64) - z64) / (CR.U32 * M)))
        _, _, margin = CR.bars(M, c_ref)
        excluded = np.abs(z64) <= margin
        wide = float(np.mean(np.abs(z64) <= 2 * margin))
        assert np.mean(excluded) <= CR.EXCLUDED_CAP and wide <= CR.EXCLUDED_CAP, (np.mean(excluded), wide)
        assert np.all(((hard != 0) == (z64 > 0)) | excluded)
        f1 = np.array([[float(v) for v in f1_loss(torch.from_numpy(hard[a:b].reshape(-1)), torch.from_numpy(truth[y_dim][a:b].reshape(-1)), EPS)]
                       for a, b in zip(off[:-1], off[1:])], np.float32)
        f1_raw = np.array([[v.numpy() for v in f1_loss(torch.from_numpy(hard[a:b].reshape(-1)), torch.from_numpy(truth[y_dim][a:b].reshape(-1)), EPS)]
                           for a, b in zip(off[:-1], off[1:])], np.float32)
        assert np.array_equal(f1, f1_raw)
        cnt = np.stack([CR.counts(hard[a:b], truth[y_dim][a:b]) for a, b in zip(off[:-1], off[1:])])
        print(f"y_dim {y_dim}: seed {seed}, positive share {share:.3f}, c_ref {c_ref:.4f}, excluded share {np.mean(excluded):.2e} "
              f"(twice the margin: {wide:.2e}), M in [{M.min():.3g}, {M.max():.3g}], f1 {f1[:, 3]}")
        k = f"y{y_dim}/"
        part.update({k + "seed": np.array(seed), k + "weight_sums": np.array([np.sum(a.astype(np.float64)) for a in w]),
                     k + "logit": logit, k + "soft": soft, k + "hard": hard.astype(np.uint8), k + "truth": truth[y_dim].astype(np.uint8), k + "f1": f1, k + "counts": cnt,
                     k + "c_ref": np.array(c_ref), k + "positive_share": np.array(share), k + "excluded_share": np.array(float(np.mean(excluded)))})
    # f1_loss on degenerate and large counts (no arrays above 2^24 elements: the sums are formed from blocks the reference sums exactly)
    special = []
    for name, (pred, tru) in {"all_zero_prediction": (np.zeros(50, np.float32), (np.arange(50) % 3 == 0).astype(np.float32)),
                              "all_one_truth": ((np.arange(64) % 4 != 0).astype(np.float32), np.ones(64, np.float32)),
                              "nothing_positive": (np.zeros(7, np.float32), np.zeros(7, np.float32))}.items():
        special.append((name, CR.counts(pred, tru), np.array([v.numpy() for v in f1_loss(torch.from_numpy(pred), torch.from_numpy(tru), EPS)], np.float32)))
    # counts above 2^24: f1_loss's expressions on the float32 images of given counts, through the reference's own code path -- int64
    # tensors whose sums are exact, converted by its `.to(torch.float32)`; lengths are products, the arrays are never built
    big = np.array([[2 ** 24 + 1, 3 * 2 ** 24 + 5, 2 ** 23 + 3, 2 ** 22 + 1], [2 ** 25 + 3, 7, 2 ** 24 + 1, 0]], np.int64)
    for row in big:
        tp, tn, fp, fn = (int(v) for v in row)
        special.append((f"big_{tp}_{tn}_{fp}_{fn}", row, _weighted_f1(f1_loss, tp, tn, fp, fn)))
    parts[0]["special/names"] = np.array([s[0] for s in special])
    parts[0]["special/counts"] = np.stack([s[1] for s in special])
    parts[0]["special/f1"] = np.stack([s[2] for s in special])
    for i, part in enumerate(parts):
        path = os.path.join(HERE, f"classify_golden.part{i}.npz")
        np.savez(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes;", len(part), "entries")
        assert os.path.getsize(path) < 1 << 20


def _weighted_f1(f1_loss, tp, tn, fp, fn):
    """f1_loss on counts too large to spell out as arrays: the function only ever sums products of its two arguments, so a 1-D
    stand-in class whose `*`, `1 - x` and `.sum()` carry multiplicities gives it the same four int64 sums, and everything after the
    sums (`.to(torch.float32)` and the ratios) is the reference's own code."""
    class Weighted:
        ndim = 1

        def __init__(self, v, wts):
            self.v, self.w = v, wts

        def detach(self):
            return self

        def __mul__(self, o):
            return Weighted(self.v * o.v, self.w)

        def __rsub__(self, one):
            return Weighted(one - self.v, self.w)

        def sum(self):
            return (self.v * self.w).sum()

    wts = torch.tensor([tp, tn, fp, fn], dtype=torch.int64)
    pred = Weighted(torch.tensor([1, 0, 1, 0], dtype=torch.int64), wts)
    true = Weighted(torch.tensor([1, 0, 0, 1], dtype=torch.int64), wts)
    return np.array([v.numpy() for v in f1_loss(pred, true, EPS)], np.float32)


if __name__ == "__main__":
    main()

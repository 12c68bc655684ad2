"""Golden outputs of the reference's Encoder (packages/models/models.py:91-105) inside VariationalAutoencoder / DeepGenerativeModel on
seeded inputs.  Build-container only (imports /root/reference):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encode_golden.py
Output: tests/golden/encode_golden.part0.npz.

Frames: those of tests/golden/classify_golden.part0.npz (utterances of 33, 65 and 20 frames, so that a 64-frame tile edge falls inside
an utterance), their SHA-256 asserted here and recorded.  Cases (tests/encode_ref.py: CASES): M1 (y_dim 0), M2 with y_dim 1 and with
y_dim 513, each built by encode_ref.build_model from the REFERENCE's classes under the recorded seed, biases then drawn N(0, 0.05) in
module order.  The weights are NOT stored: the seed is, with the float64 sum of every state_dict tensor, and the tests rebuild them
with this repository's classes.  Labels: the recorded truths of the classifier fixture (an energy gate per frame for y_dim 1, a
per-bin median gate for y_dim 513).  The reference's encoder runs on the CPU in float32 on torch.cat([x, y], 1).

Recorded per case: the labels (bytes), a seeded eps [N, 16], the reference's float32 mu and log_var, z = its two reparametrisation
lines (models.py:20-21: `std = log_var.mul(0.5).exp_()`, `z = mu.addcmul(std, epsilon)`) applied to the recorded eps, and c_ref per
head = max |out32 - out64| / (u M) with the float64 network and the mass M of tests/encode_ref.py."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import numpy as np
import torch

import encode_ref as ER
from packages.models import models as ref_models

SEEDS = {"m1": 1, "m2_y1": 2, "m2_y513": 3}
FRAMES_SHA256 = "7cef40db6daaf1d72781a81da414cf2f0e6df2eac0adaaa49316e20cda8dfa7e"


def main():
    assert ref_models.__file__.startswith(REF), ref_models.__file__
    with np.load(os.path.join(HERE, "classify_golden.part0.npz")) as z:
        frames, counts, truth1 = z["frames"], z["counts"], z["y1/truth"]
    with np.load(os.path.join(HERE, "classify_golden.part1.npz")) as z:
        truth513 = z["y513/truth"]
    sha = hashlib.sha256(np.ascontiguousarray(frames).tobytes()).hexdigest()
    assert sha == FRAMES_SHA256, sha
    assert counts.tolist() == [33, 65, 20]
    P = ER.power(frames)
    labels = {"m1": None, "m2_y1": truth1.astype(np.float32), "m2_y513": truth513.astype(np.float32)}
    out = {"frames_sha256": np.array(sha), "counts": counts}
    for case, y_dim in ER.CASES.items():
        seed = SEEDS[case]
        model = ER.build_model(ref_models, case, seed)
        y = labels[case]
        V = ER.inputs(P, y)
        assert V.shape[1] == 513 + y_dim and V.dtype == np.float32
        eps = np.random.default_rng(100 + seed).standard_normal((P.shape[0], 16)).astype(np.float32)
        with torch.no_grad():
            x = torch.from_numpy(P) if y is None else torch.cat([torch.from_numpy(P), torch.from_numpy(y)], 1)
            _, mu, log_var = model.encoder(x)
            std = log_var.mul(0.5).exp_()
            z = mu.addcmul(std, torch.from_numpy(eps))
        mu, log_var, z = mu.numpy(), log_var.numpy(), z.numpy()
        w = ER.encoder_weights(model.encoder)
        mu64, lv64, _, _ = ER.forward64(V, w)
        Mm, Ml = ER.masses(V, w)
        c_mu = float(np.max(np.abs(mu.astype(np.float64) - mu64) / (ER.U32 * Mm)))
        c_lv = float(np.max(np.abs(log_var.astype(np.float64) - lv64) / (ER.U32 * Ml)))
        bm, bl, bz = ER.bars(Mm, Ml, c_mu, c_lv, lv64, eps, ER.z64(mu64, lv64, eps))
        print(f"{case}: seed {seed}, c_ref mu {c_mu:.4f} log_var {c_lv:.4f}; bars mu {bm.min():.2e}..{bm.max():.2e}, log_var {bl.min():.2e}..{bl.max():.2e}, "
              f"z {bz.min():.2e}..{bz.max():.2e}; |mu| <= {np.abs(mu).max():.3g}, |log_var| <= {np.abs(log_var).max():.3g}; the reference's z at "
              f"{ER.worst(z, ER.z64(mu64, lv64, eps), bz):.3f} bars")
        k = case + "/"
        out.update({k + "seed": np.array(seed), k + "tensor_sums": ER.tensor_sums(model), k + "eps": eps, k + "mu": mu, k + "log_var": log_var, k + "z": z,
                    k + "c_ref": np.array([c_mu, c_lv])})
        if y is not None:
            out[k + "labels"] = y.astype(np.uint8)
    path = os.path.join(HERE, "encode_golden.part0.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

"""Golden outputs of the reference's Encoder and Classifier (packages/models/models.py:41-63, 91-105) at the geometries of
tests/mlp_generic_cases.py, for the generic kernel (csrc/mlp_generic.hip).  Build-container only (imports /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mlp_generic_golden.py
Output: tests/golden/mlp_generic_golden.part*.npz.

Frames: those of tests/golden/classify_golden.part0.npz (118 frames, utterances of 33, 65 and 20), their SHA-256 asserted here and
recorded.  Every case builds its seeded model from the REFERENCE's classes (mlp_generic_cases.build_encoder_model / build_classifier:
the construction, then every Linear bias drawn N(0, 0.05) in module order) and runs the reference's own float32 CPU forward.  The
weights are NOT stored: the seed is, with the float64 sum of every state_dict tensor, and the tests rebuild them with this
repository's classes.  Labels: the classifier fixture's truths (mlp_generic_cases.labels_for), recorded as bytes.

Recorded per encoder case: seed, tensor sums, labels, a seeded eps [118, z], the reference's float32 mu, log_var and z (its two
reparametrisation lines applied to the recorded eps), c_ref per head = max |out32 - out64| / (u M) with forward64 / masses of
tests/encode_ref.py.  Per classifier case: seed, tensor sums, float32 logits and soft, hard as bytes, c_ref with logits64 / mass of
tests/classify_ref.py, the excluded share.

Asserted here, so that a test cannot hide a failure:
  * the floor the tests put under a small c_ref (mlp_generic_cases.C_FLOOR) is the smallest c_ref of the committed encode / classify
    fixtures; it is recorded, and every bar here is formed with c_eff = max(c_ref, floor) as the tests form it;
  * for every classifier case the share of elements within the hard-decision margin |logit64| <= 2 bar_logit + 4 u is at most
    classify_ref.EXCLUDED_CAP on the reference's own run (none of the 118 at y_dim 1), the reference's hard labels match the float64
    decision outside it, and the logits are not constant (a dead relu stack would show nothing).  The seed of a classifier case is the
    first from 1 up for which this holds."""
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

from packages.models import models as ref_models          # before golden_util, which puts this repository in front of the path

import classify_ref as CR
import encode_ref as ER
import golden_util as gu
import mlp_generic_cases as MC

FRAMES_SHA256 = "7cef40db6daaf1d72781a81da414cf2f0e6df2eac0adaaa49316e20cda8dfa7e"
ENCODER_SEED0 = 21                   # encoder case i is built under seed 21 + i


def encoder_case(case, seed, P, y):
    model = MC.build_encoder_model(ref_models, case, seed)
    z_dim = case[1]
    V = ER.inputs(P, y)
    assert V.shape[1] == 513 + case[0] and V.dtype == np.float32
    eps = np.random.default_rng(100 + seed).standard_normal((P.shape[0], z_dim)).astype(np.float32)
    with torch.no_grad():
        _, mu, log_var = model.encoder(torch.from_numpy(V))
        std = log_var.mul(0.5).exp_()
        z = mu.addcmul(std, torch.from_numpy(eps))
    mu, log_var, z = mu.numpy(), log_var.numpy(), z.numpy()
    assert mu.shape == (P.shape[0], z_dim)
    w = ER.encoder_weights(model.encoder)
    mu64, lv64, _, _ = ER.forward64(V, w)
    Mm, Ml = ER.masses(V, w)
    c_mu = float(np.max(np.abs(mu.astype(np.float64) - mu64) / (ER.U32 * Mm)))
    c_lv = float(np.max(np.abs(log_var.astype(np.float64) - lv64) / (ER.U32 * Ml)))
    zz = ER.z64(mu64, lv64, eps)
    bm, bl, bz = ER.bars(Mm, Ml, MC.c_eff(c_mu), MC.c_eff(c_lv), lv64, eps, zz)
    print(f"{MC.enc_id(case)}: seed {seed}, c_ref mu {c_mu:.4f} log_var {c_lv:.4f} (floor {MC.C_FLOOR:.4f}); bars mu {bm.min():.2e}..{bm.max():.2e}, "
          f"log_var {bl.min():.2e}..{bl.max():.2e}; |mu| <= {np.abs(mu).max():.3g}, |log_var| <= {np.abs(log_var).max():.3g}; the reference's z at "
          f"{ER.worst(z, zz, bz):.3f} bars")
    assert np.std(mu) > 0 and np.std(log_var) > 0
    out = {"seed": np.array(seed), "tensor_sums": ER.tensor_sums(model), "eps": eps, "mu": mu, "log_var": log_var, "z": z, "c_ref": np.array([c_mu, c_lv])}
    if y is not None:
        out["labels"] = y.astype(np.uint8)
    return out


def classifier_try(case, seed, P):
    clf = MC.build_classifier(ref_models, case, seed)
    with torch.no_grad():
        x = torch.from_numpy(P)
        soft = clf(x).numpy()
        h = x
        for layer in clf.hidden:
            h = torch.relu(layer(h))
        logit = clf.output_layer(h).numpy()
    w = MC.classifier_weights(clf)
    z64, M = CR.logits64(P, w), CR.mass(P, w)
    c_ref = float(np.max(np.abs(logit.astype(np.float64) - z64) / (CR.U32 * M)))
    _, _, margin = CR.bars(M, MC.c_eff(c_ref))
    excluded = np.abs(z64) <= margin
    hard = (soft > 0.5).astype(np.float32)
    ok = (float(np.mean(excluded)) <= CR.EXCLUDED_CAP and bool(np.all(((hard != 0) == (z64 > 0)) | excluded)) and float(np.std(z64)) > 1e-3
          and bool(np.all(np.std(z64, axis=0) > 0)))
    return ok, clf, logit, soft, hard, c_ref, float(np.mean(excluded))


def main():
    assert ref_models.__file__.startswith(REF), ref_models.__file__
    c0, c1 = (dict(np.load(os.path.join(HERE, f"classify_golden.part{i}.npz"))) for i in (0, 1))
    frames, counts, truth1, truth513 = c0["frames"], c0["counts"], c0["y1/truth"], c1["y513/truth"]
    sha = hashlib.sha256(np.ascontiguousarray(frames).tobytes()).hexdigest()
    assert sha == FRAMES_SHA256, sha
    assert counts.tolist() == MC.COUNTS
    enc_gold = gu.load_golden("encode_golden")
    committed = [float(v) for k in enc_gold if k.endswith("/c_ref") for v in np.ravel(enc_gold[k])] + [float(c0["y1/c_ref"]), float(c1["y513/c_ref"])]
    assert MC.C_FLOOR == min(committed) and 0.0 < MC.C_FLOOR < 1.0, (MC.C_FLOOR, committed)
    P = ER.power(frames)
    out = {"frames_sha256": np.array(sha), "counts": counts, "c_floor": np.array(MC.C_FLOOR)}
    for i, case in enumerate(MC.ENCODER_CASES):
        y = MC.labels_for(case[0], truth1, truth513)
        out.update({MC.enc_id(case) + "/" + k: v for k, v in encoder_case(case, ENCODER_SEED0 + i, P, y).items()})
    for case in MC.CLASSIFIER_CASES:
        for seed in range(1, 200):
            ok, clf, logit, soft, hard, c_ref, share = classifier_try(case, seed, P)
            if ok:
                break
        assert ok, (case, "no seed up to 200 keeps the margin share under the cap with logits that vary")
        if case[1] == 1:
            assert share == 0.0
        print(f"{MC.clf_id(case)}: seed {seed}, c_ref {c_ref:.4f} (floor {MC.C_FLOOR:.4f}), excluded share {share:.2e}, positive share {np.mean(hard):.3f}, "
              f"|logit| <= {np.abs(logit).max():.3g}")
        k = MC.clf_id(case) + "/"
        out.update({k + "seed": np.array(seed), k + "tensor_sums": MC.state_sums(clf), k + "logit": logit, k + "soft": soft, k + "hard": hard.astype(np.uint8),
                    k + "c_ref": np.array(c_ref), k + "excluded_share": np.array(share)})
    for path in gu.save_golden(MC.STEM, out):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

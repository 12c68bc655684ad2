"""The encoder stage without a GPU: the rebuilt weights against the fixture's recorded sums, the numpy restatement
(tests/encode_ref.py) against the reference's recorded float32 outputs (tests/golden/encode_golden.part*.npz, made by
tests/golden/make_encode_golden.py), what encoder_supported accepts, and the table refusals on host tensors.

The restatement's float64 mu and log_var are held to the recorded float32 ones within c_ref u M per head (c_ref is the maximum of
exactly that ratio, so this pins the restatement, the rebuilt weights and the fixture to each other), the recorded z within the z
bar at factor 1."""
import glob
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch

import encode_ref as ER
from test_classify_cpu import GOLD as CLASSIFY_GOLD

E = importlib.import_module("disentangled-vae_amd.encode")
from packages.models import models as PM

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


def load_golden():
    g = {}
    for path in sorted(glob.glob(os.path.join(GOLD_DIR, "encode_golden.part*.npz"))):
        with np.load(path) as z:
            g.update({k: z[k] for k in z.files})
    return g


GOLD = load_golden()
FRAMES = CLASSIFY_GOLD["frames"]
_built = {}


def rebuild(case):
    """(model, encoder weights) of a fixture case from this repository's classes, checked against the recorded sums; built once."""
    if case not in _built:
        model = ER.build_model(PM, case, int(GOLD[case + "/seed"]))
        assert np.array_equal(ER.tensor_sums(model), GOLD[case + "/tensor_sums"]), "the seeded construction no longer gives the fixture's weights"
        _built[case] = (model, ER.encoder_weights(model.encoder))
    return _built[case]


def labels_of(case):
    return GOLD[case + "/labels"].astype(np.float32) if ER.CASES[case] else None


def test_frames_are_the_classifier_fixtures():
    assert hashlib.sha256(np.ascontiguousarray(FRAMES).tobytes()).hexdigest() == str(GOLD["frames_sha256"])
    assert GOLD["counts"].tolist() == CLASSIFY_GOLD["counts"].tolist() == [33, 65, 20]


@pytest.mark.parametrize("case", list(ER.CASES))
def test_rebuilt_weights_match_the_recorded_sums(case):
    model, w = rebuild(case)
    y_dim = ER.CASES[case]
    assert [a.shape for a in w] == [(128, 513 + y_dim), (128,), (128, 128), (128,), (16, 128), (16,), (16, 128), (16,)]
    assert all(np.any(a != 0) for a in w), "a bias left at zero would hide a dropped bias"
    assert E.encoder_supported(model.encoder, y_dim)


@pytest.mark.parametrize("case", list(ER.CASES))
def test_restatement_reproduces_the_reference(case):
    k = case + "/"
    _, w = rebuild(case)
    V = ER.inputs(ER.power(FRAMES), labels_of(case))
    c_mu, c_lv = (float(c) for c in GOLD[k + "c_ref"])
    mu64, lv64, _, _ = ER.forward64(V, w)
    Mm, Ml = ER.masses(V, w)
    wm = ER.worst(GOLD[k + "mu"], mu64, c_mu * ER.U32 * Mm)
    wl = ER.worst(GOLD[k + "log_var"], lv64, c_lv * ER.U32 * Ml)
    print(f"{case}: c_ref {c_mu:.4f} / {c_lv:.4f}; recorded mu at most {wm:.6f}, log_var {wl:.6f} c_ref u M from the restatement")
    assert wm <= 1.0 + 1e-12 and wl <= 1.0 + 1e-12
    assert 0.01 < c_mu < 1.0 and 0.01 < c_lv < 1.0
    ER.check(f"reference {case}", GOLD[k + "mu"], GOLD[k + "log_var"], GOLD[k + "z"], V, w, c_mu, c_lv, GOLD[k + "eps"], factor=1.0)


def test_encoder_supported_accepts_and_refuses():
    assert E.encoder_supported(PM.Encoder([513, [128, 128], 16]), 0)
    assert E.encoder_supported(PM.Encoder([514, [128, 128], 16]), 1)
    assert E.encoder_supported(PM.Encoder([1026, [128, 128], 16]), 513)
    assert E.encoder_supported(PM.DeepGenerativeModel_v5([513, 1, 16, [128, 128]]).enc_dec_clf.encoder, 0)
    with_bn = PM.Encoder([513, [128, 128], 16])
    with_bn.hidden.insert(1, torch.nn.BatchNorm1d(128))
    refused = {"width 64": (PM.Encoder([513, [64, 64], 16]), 0), "one hidden layer": (PM.Encoder([513, [128], 16]), 0),
               "three hidden layers": (PM.Encoder([513, [128, 128, 128], 16]), 0), "batch norm": (with_bn, 0),
               "latent 8": (PM.Encoder([513, [128, 128], 8]), 0), "257 bins": (PM.Encoder([257, [128, 128], 16]), 0),
               "y_dim 7": (PM.Encoder([520, [128, 128], 16]), 7), "label width mismatch": (PM.Encoder([513, [128, 128], 16]), 1),
               "a classifier": (PM.Classifier([513, [128, 128], 16]), 0)}
    for name, (enc, y_dim) in refused.items():
        assert not E.encoder_supported(enc, y_dim), name
        with pytest.raises(TypeError) as e:
            E.EncoderPack(enc, y_dim)
        assert type(enc).__name__ in str(e.value), (name, str(e.value))
    with pytest.raises(TypeError, match="BatchNorm1d"):
        E.EncoderPack(with_bn, 0)
    with pytest.raises(TypeError, match=r"520->128.*y_dim 7"):
        E.EncoderPack(refused["y_dim 7"][0], 7)


def test_table_refusals_name_the_utterance():
    off = E.frame_table("encode_batch", [33, 65, 20], 118)
    assert off.tolist() == [0, 33, 98, 118]
    assert E.column_table("op", off, [0, 64, 160], 192).tolist() == [0, 64, 160]
    with pytest.raises(ValueError, match="utterance 2 .*leaves the 100 rows"):
        E.frame_table("encode_batch", [33, 65, 20], 100)
    with pytest.raises(ValueError, match="utterance 1 starts at column 32, 33 are taken"):
        E.column_table("op", off, [0, 32, 160], 192)
    with pytest.raises(ValueError, match="utterance 2 .*leaves the 170 columns"):
        E.column_table("op", off, [0, 64, 160], 170)
    with pytest.raises(ValueError, match="2 first columns for 3 utterances"):
        E.column_table("op", off, [0, 64], 192)


def test_latent_batch_views():
    mu = torch.arange(6 * 16, dtype=torch.float32).reshape(6, 16)
    lat = E.LatentBatch(mu, -mu, None, [2, 4])
    assert len(lat) == 2 and lat.frame_off.tolist() == [0, 2, 6]
    assert lat.view(1).shape == (16, 4) and torch.equal(lat.view(1), mu[2:6].T) and torch.equal(lat.view(0, "log_var"), -mu[:2].T)
    assert [a.shape for a in lat.numpy()] == [(16, 2), (16, 4)]
    with pytest.raises(ValueError, match="no z"):
        lat.view(0, "z")
    with pytest.raises(ValueError, match="'mu', 'log_var' or 'z'"):
        lat.view(0, "sigma")

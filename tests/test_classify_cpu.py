"""The classifier stage without a GPU: the numpy restatement (tests/classify_ref.py) against the reference's recorded outputs
(tests/golden/classify_golden.part*.npz, made by tests/golden/make_classify_golden.py), the F1 finishing against the recorded
f1_loss values bit for bit, what classifier_supported accepts, the table refusals and f1_loss_many on host tensors.

The restatement's float64 logits are held to the recorded float32 logits within c_ref u M (c_ref is the maximum of exactly that
ratio, so this pins the restatement, the rebuilt weights and the fixture to each other), soft within c_ref u M / 4 + 4 u (the float32
sigmoid's own rounding: c_ref u M alone is below the spacing of float32 near 0.5 wherever M < 100), hard outside the excluded set."""
import importlib
import os

import numpy as np
import pytest
import torch

import classify_ref as CR

C = importlib.import_module("disentangled-vae_amd.classify")
from packages.models import models as PM
from packages.models import utils as PU

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


def load_golden():
    g = {}
    for i in range(2):
        with np.load(os.path.join(GOLD_DIR, f"classify_golden.part{i}.npz")) as z:
            g.update({k: z[k] for k in z.files})
    return g


def rebuild(g, y_dim):
    """The classifier of a fixture case: the seeded construction the fixture script used, checked against the recorded sums."""
    torch.manual_seed(int(g[f"y{y_dim}/seed"]))
    clf = PM.Classifier([513, [128, 128], y_dim])
    w = weights(clf)
    sums = np.array([np.sum(a.astype(np.float64)) for a in w])
    assert np.array_equal(sums, g[f"y{y_dim}/weight_sums"]), "the seeded construction no longer gives the fixture's weights"
    return clf, w


def weights(clf):
    return [t.detach().cpu().numpy() for t in (clf.hidden[0].weight, clf.hidden[0].bias, clf.hidden[1].weight, clf.hidden[1].bias,
                                                clf.output_layer.weight, clf.output_layer.bias)]


GOLD = load_golden()


@pytest.mark.parametrize("y_dim", [1, 513])
def test_restatement_reproduces_the_reference(y_dim):
    k = f"y{y_dim}/"
    _, w = rebuild(GOLD, y_dim)
    P = CR.power(GOLD["frames"])
    z64, M = CR.logits64(P, w), CR.mass(P, w)
    c_ref = float(GOLD[k + "c_ref"])
    assert 0.2 <= float(GOLD[k + "positive_share"]) <= 0.8 and float(np.mean(GOLD[k + "hard"])) == pytest.approx(float(GOLD[k + "positive_share"]))
    worst = float(np.max(np.abs(GOLD[k + "logit"].astype(np.float64) - z64) / (c_ref * CR.U32 * M)))
    print(f"y_dim {y_dim}: c_ref {c_ref:.4f}, recorded logits at most {worst:.6f} c_ref u M from the restatement")
    assert worst <= 1.0 + 1e-12
    CR.check(f"reference y_dim {y_dim}", None, GOLD[k + "soft"], GOLD[k + "hard"], z64, M, c_ref, factor=1.0)
    # the device's bars: the excluded set stays under the cap for them too
    _, _, margin = CR.bars(M, c_ref)
    assert np.mean(np.abs(z64) <= margin) <= CR.EXCLUDED_CAP
    off = np.concatenate([[0], np.cumsum(GOLD["counts"])])
    cnt = np.stack([CR.counts(GOLD[k + "hard"][a:b], GOLD[k + "truth"][a:b]) for a, b in zip(off[:-1], off[1:])])
    assert np.array_equal(cnt, GOLD[k + "counts"])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_f1_finishing_equals_f1_loss_bit_for_bit():
    names = [str(n) for n in GOLD["special/names"]]
    assert {"all_zero_prediction", "all_one_truth"} <= set(names) and any(n.startswith("big_") for n in names)
    assert GOLD["special/counts"].max() > 2 ** 24
    cases = [(n, c, f) for n, c, f in zip(names, GOLD["special/counts"], GOLD["special/f1"])]
    for y_dim in (1, 513):
        cases += [(f"y{y_dim} utterance {u}", c, f) for u, (c, f) in enumerate(zip(GOLD[f"y{y_dim}/counts"], GOLD[f"y{y_dim}/f1"]))]
    eps = float(GOLD["epsilon"])
    for name, c, f in cases:
        got_np = CR.f1_from_counts(c, eps)
        got_t = C.f1_from_counts(torch.from_numpy(np.asarray(c, np.int64)), eps).numpy()
        print(name, c.tolist(), f.tolist())
        assert same_bits(got_np, f), (name, got_np, f)
        assert same_bits(got_t, f), (name, got_t, f)
    table = C.f1_from_counts(torch.from_numpy(np.stack([c for _, c, _ in cases])), eps).numpy()
    assert same_bits(table, np.stack([f for _, _, f in cases]))


def test_classifier_supported_accepts_and_refuses():
    assert C.classifier_supported(PM.Classifier([513, [128, 128], 1]))
    assert C.classifier_supported(PM.Classifier([513, [128, 128], 513]))
    refused = {"batch norm": PM.Classifier([513, [128, 128], 1], batch_norm=True), "one hidden layer": PM.Classifier([513, [128], 1]),
               "three hidden layers": PM.Classifier([513, [128, 128, 128], 1]), "width 64": PM.Classifier([513, [64, 64], 1]),
               "257 bins": PM.Classifier([257, [128, 128], 1]), "y_dim 2": PM.Classifier([513, [128, 128], 2]),
               "two classes": PM.Classifier2Classes([513, [128, 128], 1]), "a Linear": torch.nn.Linear(513, 1)}
    for name, clf in refused.items():
        assert not C.classifier_supported(clf), name
        with pytest.raises(TypeError) as e:
            C.ClassifierPack(clf)
        assert type(clf).__name__ in str(e.value), (name, str(e.value))
    with pytest.raises(TypeError, match="BatchNorm1d"):
        C.classify_batch(refused["batch norm"], torch.zeros(4, 513))
    with pytest.raises(TypeError, match=r"128->2"):
        C.classify_batch(refused["y_dim 2"], torch.zeros(4, 513))


def test_table_refusals_name_the_utterance():
    assert C.frame_table("op", [3, 4, 5], 12).tolist() == [0, 3, 7, 12]
    assert C.frame_table("op", [3, 4], 12, first=5).tolist() == [5, 8, 12]
    with pytest.raises(ValueError, match="utterance 1 has 0 frames"):
        C.frame_table("op", [3, 0, 5], 12)
    with pytest.raises(ValueError, match="utterance 2 .*leaves the 10 rows"):
        C.frame_table("op", [3, 4, 5], 10)
    with pytest.raises(ValueError, match="no utterances"):
        C.frame_table("op", [], 10)


def test_label_batch_views():
    soft = torch.arange(12, dtype=torch.float32).reshape(6, 2) / 12
    lb = C.LabelBatch(soft, (soft > 0.5).float(), [2, 4])
    assert len(lb) == 2 and lb.frame_off.tolist() == [0, 2, 6] and lb.y_dim == 2
    assert lb[1].shape == (2, 4) and torch.equal(lb[1], lb.hard[2:6].T) and torch.equal(lb.view(0, "soft"), soft[:2].T)
    assert [a.shape for a in lb.numpy()] == [(2, 2), (2, 4)] and np.array_equal(lb.numpy("soft")[1], soft[2:].numpy().T)


def test_f1_loss_many_on_host_tensors_equals_the_loop():
    rng = np.random.default_rng(5)
    preds = [torch.from_numpy((rng.random(n) > 0.5).astype(np.float32)) for n in (1, 17, 300)] + [torch.from_numpy(rng.random((9, 2)).astype(np.float32))]
    truths = [torch.from_numpy((rng.random(n) > 0.3).astype(np.float32)) for n in (1, 17, 300)] + [torch.from_numpy((rng.random(9) > 0.5).astype(np.int64))]
    many = PU.f1_loss_many(preds, truths, 1e-8)
    assert len(many) == 4
    for got, p, t in zip(many, preds, truths):
        want = PU.f1_loss(p, t, 1e-8)
        assert all(same_bits(a.numpy(), b.numpy()) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        PU.f1_loss_many(preds, truths[:2])

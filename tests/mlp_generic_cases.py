"""The geometry cases of the generic encoder / classifier kernel (csrc/mlp_generic.hip), shared by tests/golden/make_mlp_generic_golden.py,
tests/test_mlp_generic_cpu.py and tests/test_gpu_mlp_generic.py: the case lists, the seeded construction of their models from a
`packages.models.models` module (the reference's in the fixture script, this repository's in the tests), their labels, and the floor
of c_ref.  No GPU, no library, no reference checkout.

The float64 restatements, masses and bars are those of tests/encode_ref.py and tests/classify_ref.py, which are shape-agnostic.

Floor.  c_ref is a maximum over the case's output elements; over a handful of elements (z 1: 118 of them) a maximum underestimates
the factor a second draw can reach.  Where a case's c_ref lies below the smallest c_ref recorded in the committed encode / classify
fixtures (cases of ~2e3 .. 6e4 elements each), the tests use that smallest committed value instead: c_eff = max(c_ref, C_FLOOR)."""
import numpy as np

import golden_util as gu

# (y_dim, z, (h1, h2)): every limit, sizes off every multiple of 4 and 16, the reference's geometry
ENCODER_CASES = [(0, 32, (256, 64)), (1, 32, (256, 64)), (1, 5, (48, 200)), (513, 64, (16, 16)), (0, 1, (1, 1)), (3, 17, (129, 127)),
                 (513, 128, (512, 512)), (1, 16, (128, 128))]
# ((h1, h2), y_dim)
CLASSIFIER_CASES = [((256, 64), 1), ((48, 200), 2), ((129, 127), 17), ((1, 1), 1), ((512, 512), 513), ((128, 128), 513)]
STEM = "mlp_generic_golden"
COUNTS = [33, 65, 20]


def enc_id(case):
    y, z, (h1, h2) = case
    return f"enc_y{y}_z{z}_h{h1}x{h2}"


def clf_id(case):
    (h1, h2), y = case
    return f"clf_h{h1}x{h2}_y{y}"


def _draw_biases(model):
    import torch
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    return model


def build_encoder_model(models, case, seed):
    """encode_ref.build_model at any size: the seeded construction, then every Linear bias drawn N(0, 0.05) in module order."""
    import torch
    y, z, h = case
    torch.manual_seed(int(seed))
    model = models.VariationalAutoencoder([513, z, list(h)]) if y == 0 else models.DeepGenerativeModel([513, y, z, list(h)], None)
    return _draw_biases(model)


def build_classifier(models, case, seed):
    import torch
    h, y = case
    torch.manual_seed(int(seed))
    return _draw_biases(models.Classifier([513, list(h), y]))


def classifier_weights(clf):
    return [t.detach().cpu().numpy() for l in (*clf.hidden, clf.output_layer) for t in (l.weight, l.bias)]


def state_sums(module):
    return np.array([np.sum(v.detach().cpu().numpy().astype(np.float64)) for v in module.state_dict().values()])


def labels_for(y_dim, truth1, truth513):
    """Label rows [118, y_dim] from the classifier fixture's truths: the energy gate for y_dim 1, else y_dim of the 513 per-bin gates
    spread over the bins (all of them at 513)."""
    if y_dim == 0:
        return None
    if y_dim == 1:
        return np.asarray(truth1, np.float32)
    return np.ascontiguousarray(np.asarray(truth513, np.float32)[:, (np.arange(y_dim) * 513) // y_dim])


def committed_floor():
    """The smallest c_ref of the committed encode / classify fixtures."""
    e, c = gu.load_golden("encode_golden"), gu.load_golden("classify_golden")
    vals = [float(v) for k in e if k.endswith("/c_ref") for v in np.ravel(e[k])] + [float(c["y1/c_ref"]), float(c["y513/c_ref"])]
    return min(vals)


C_FLOOR = committed_floor()


def c_eff(c_ref):
    return max(float(c_ref), C_FLOOR)


_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = gu.load_golden(STEM)
    return _gold


def frames():
    return gu.load_golden("classify_golden")["frames"]

"""Labels for a ragged batch on the device: the classifier stage of the reference's M2_info evaluation and the score of its labels.

classify_batch runs `model.classifier` (packages/models/models.py: Classifier, 513 -> 128 -> 128 -> y_dim) over every frame of a
SpecBatch in ONE launch (include/dvae.h: dvae_classify_batch) -- the reference's `y_hat_soft = model.classifier(torch.t(S_abs_2))`,
`y_hat_hard = y_hat_soft > 0.5` (scripts/evaluate_ntcd_M2_info_vad.py:175-219, scripts/reconstruct_M2_info.py:194), |X|^2 formed in
the kernel with the bits of McemBatch.X2.  The LabelBatch it returns goes to McemBatch.init_parameters as it is, device to device.
f1_batch scores hard labels against a truth per utterance (packages/models/utils.py:120-159 f1_loss, called per utterance in a process
pool by scripts/run_metrics_classif.py:136): integer confusion counts from one launch (dvae_label_counts_batch), the four ratios on the
[U, 4] table in f1_loss's own float32 order.  No CPU arithmetic exists here: without the library or a GPU the batch ops raise;
classifier_supported, frame_table and f1_from_counts on host tensors need neither.
"""
import numpy as np
import torch
from torch import nn

from . import native as N
from . import ragged as R
from . import stft as STFT
from . import target as TGT

F_BINS, H_DIM = 513, 128
Y_DIMS = (1, F_BINS)
H_MAX = 512                                     # limit of the generic kernel (csrc/mlp_generic.hip), that of dvae_mcem_plan_dims


def _shape(clf):
    """What classifier_supported looks at, as a string for the refusal."""
    hidden = getattr(clf, "hidden", None)
    out = getattr(clf, "output_layer", None)
    if hidden is None or out is None:
        return f"{type(clf).__name__} (no hidden / output_layer)"
    parts = [f"{l.in_features}->{l.out_features}" if isinstance(l, nn.Linear) else type(l).__name__ for l in hidden]
    parts.append(f"{out.in_features}->{out.out_features}" if isinstance(out, nn.Linear) else type(out).__name__)
    return f"{type(clf).__name__} [{', '.join(parts)}]"


def classifier_supported(clf):
    """The kernel covers the classifier the reference's scripts build: Classifier([513, [128, 128], y_dim]) without batch norm,
    y_dim 1 or 513 (relu, relu, sigmoid)."""
    from packages.models.models import Classifier
    if not isinstance(clf, Classifier):
        return False
    hs = list(clf.hidden)
    out = clf.output_layer
    return (len(hs) == 2 and all(isinstance(l, nn.Linear) and l.bias is not None for l in hs + [out])
            and hs[0].in_features == F_BINS and hs[0].out_features == H_DIM and hs[1].in_features == H_DIM and hs[1].out_features == H_DIM
            and out.in_features == H_DIM and out.out_features in Y_DIMS)


def _generic_dims(clf):
    """(h1, h2, y_dim) where the generic kernel covers the classifier, else None: a Classifier without batch norm, two hidden Linear
    layers with biases, 513 -> h1 -> h2 -> y_dim within the limits."""
    from packages.models.models import Classifier
    if not isinstance(clf, Classifier):
        return None
    hs = list(clf.hidden)
    out = clf.output_layer
    if len(hs) != 2 or not all(isinstance(l, nn.Linear) and l.bias is not None for l in hs + [out]):
        return None
    h1, h2, y = hs[0].out_features, hs[1].out_features, out.out_features
    if hs[0].in_features != F_BINS or hs[1].in_features != h1 or out.in_features != h2:
        return None
    if not (1 <= h1 <= H_MAX and 1 <= h2 <= H_MAX and 1 <= y <= F_BINS):
        return None
    return h1, h2, y


def classifier_kind(clf):
    """Which kernel serves `clf`: "resident" (classify.hip: the reference's geometry, classifier_supported), "generic"
    (csrc/mlp_generic.hip: two hidden layers, hidden widths 1..512, y_dim 1..513, 513 bins, no batch norm, fp32) or None.  Reads
    layer shapes only: works on CPU modules."""
    if _generic_dims(clf) is None:
        return None
    return "resident" if classifier_supported(clf) else "generic"


class ClassifierPack:
    """The six state_dict tensors of a Classifier in one contiguous float32 device buffer, the layout of dvae_classify_batch:
    W1 [128][513] | b1 | W2 [128][128] | b2 | W3 [y_dim][128] | b3.  repack(clf) after training.  generic=True: the fragment-order
    copy of dvae_classify_generic_pack for the generic kernel, which covers every geometry classifier_kind names (the reference's
    too); h1, h2, y_dim: the geometry."""

    def __init__(self, clf, generic=False):
        self.generic = bool(generic)
        if self.generic:
            dims = _generic_dims(clf)
            if dims is None:
                raise TypeError(f"classify_batch: the generic kernel covers Classifier [513->h1, h1->h2, h2->y_dim] without batch norm, "
                                f"h1 / h2 1..{H_MAX}, y_dim 1..{F_BINS}, got {_shape(clf)}")
            self.h1, self.h2, self.y_dim = dims
        else:
            if not classifier_supported(clf):
                raise TypeError(f"classify_batch: the kernel covers Classifier [513->128, 128->128, 128->1 or 513] without batch norm, "
                                f"got {_shape(clf)}")
            self.h1, self.h2, self.y_dim = H_DIM, H_DIM, clf.output_layer.out_features
        self.weights = None
        self.repack(clf)

    def repack(self, clf):
        ts = [p.detach() for l in (*clf.hidden, clf.output_layer) for p in (l.weight, l.bias)]
        if not all(t.is_cuda for t in ts):
            raise RuntimeError("classify_batch: the classifier's parameters must be CUDA tensors (no CPU fallback)")
        if any(t.dtype != torch.float32 for t in ts):
            raise TypeError("classify_batch: the HIP path computes in float32")
        if self.generic:
            if _generic_dims(clf) != (self.h1, self.h2, self.y_dim):
                raise TypeError(f"classify_batch: repack: {_shape(clf)} is not the geometry this pack was made for")
            lib = N.load()
            want = lib.dvae_classify_generic_weights_floats(self.h1, self.h2, self.y_dim)
            dev = ts[0].device
            if self.weights is None or self.weights.device != dev:
                self.weights = torch.empty(want, dtype=torch.float32, device=dev)
            ts = [t.contiguous() for t in ts]
            with torch.cuda.device(dev):
                N.check(lib.dvae_classify_generic_pack(self.h1, self.h2, self.y_dim, N.ptr(ts[0]), ts[0].stride(0), N.ptr(ts[1]), N.ptr(ts[2]),
                                                       ts[2].stride(0), N.ptr(ts[3]), N.ptr(ts[4]), ts[4].stride(0), N.ptr(ts[5]),
                                                       N.ptr(self.weights), N.stream()), "dvae_classify_generic_pack")
            self._keep = ts                  # the pack kernels read them on the stream
            return
        flat = torch.cat([t.reshape(-1) for t in ts])
        want = N.load().dvae_classify_weights_floats(self.y_dim)
        if flat.numel() != want:
            raise RuntimeError(f"classify_batch: packed {flat.numel()} floats, the kernel reads {want}")
        if self.weights is None or self.weights.device != flat.device:
            self.weights = flat
        else:
            self.weights.copy_(flat)


def pack_classifier(clf):
    """The pack of `clf` by classifier_kind: the resident pack wherever it applies, the generic one for every other covered
    geometry; TypeError naming the shape and the limits for a classifier no kernel covers."""
    return ClassifierPack(clf, generic=classifier_kind(clf) != "resident")


def frame_table(op, counts, n_rows, first=0):
    """The int64 frame prefix [U + 1] of utterances of counts[u] rows laid end to end from row `first` in a buffer of n_rows rows.
    ValueError naming the utterance for one without frames and for one that leaves the rows."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    if counts.size == 0:
        raise ValueError(f"{op}: no utterances")
    bad = np.flatnonzero(counts < 1)
    if bad.size:
        raise ValueError(f"{op}: utterance {int(bad[0])} has {int(counts[bad[0]])} frames: at least one is needed")
    if first < 0:
        raise ValueError(f"{op}: the first row is {first}")
    off = R.prefix(counts) + int(first)
    over = np.flatnonzero(off[1:] > int(n_rows))
    if over.size:
        u = int(over[0])
        raise ValueError(f"{op}: utterance {u} (rows [{int(off[u])}, {int(off[u + 1])})) leaves the {int(n_rows)} rows given")
    return off


class LabelBatch:
    """The labels of a ragged batch on the device, in the training layout: soft and hard float32 [N, y_dim] (hard: 0 / 1), utterance
    u at rows frame_off[u] : frame_off[u + 1]; counts: T_u; logits [N, y_dim] or None.  lb[u]: the (y_dim, T_u) view of the hard
    labels, the orientation the reference hands to MCEM (lb.view(u, "soft"): the soft ones)."""

    def __init__(self, soft, hard, counts, frame_off=None, logits=None):
        self.soft, self.hard, self.logits = soft, hard, logits
        self.counts = [int(c) for c in counts]
        self.frame_off = R.prefix(self.counts) if frame_off is None else np.asarray(frame_off, np.int64)
        self.y_dim = int(hard.shape[1])

    def __len__(self):
        return len(self.counts)

    def view(self, u, use="hard"):
        if use not in ("hard", "soft"):
            raise ValueError(f"LabelBatch: use 'hard' or 'soft', got {use!r}")
        return getattr(self, use)[int(self.frame_off[u]):int(self.frame_off[u + 1])].T

    def __getitem__(self, u):
        return self.view(u)

    def numpy(self, use="hard"):
        """Every utterance as a host array (y_dim, T_u) (views of one host copy)."""
        h = getattr(self, use).cpu().numpy()
        return [h[a:b].T for a, b in zip(self.frame_off[:-1], self.frame_off[1:])]


def _rows(op, t, name, width=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.dtype == torch.float32):
        raise TypeError(f"{op}: {name}: float32 CUDA rows [N, {'y_dim' if width is None else width}] are required")
    if width is not None and t.shape[1] != width:
        raise ValueError(f"{op}: {name} has {t.shape[1]} columns, {width} are needed")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def classify_rows(pack, src, frame_off, soft, hard, logits=None):
    """dvae_classify_batch on device buffers: src complex64 [N, 513] frames or float32 [N, >= 513 by stride] power rows, frame_off the
    host prefix [U + 1], soft / hard / logits float32 [N, y_dim] written in place for the rows inside the table and nowhere else.
    With a generic pack the same through dvae_classify_generic_batch."""
    lib = N.load()
    is_complex = src.dtype == torch.complex64
    ld = F_BINS if is_complex else N.ld(src)
    off = np.ascontiguousarray(frame_off, np.int64)
    for name, o in (("soft", soft), ("hard", hard), ("logits", logits)):
        if o is not None and not (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (src.shape[0], pack.y_dim)):
            raise ValueError(f"classify_batch: {name} must be contiguous float32 CUDA rows [{src.shape[0]}, {pack.y_dim}]")
    with torch.cuda.device(src.device):
        if pack.generic:
            N.check(lib.dvae_classify_generic_batch(N.ptr(src), int(is_complex), ld, src.shape[0], off.size - 1, off.ctypes.data, N.ptr(pack.weights),
                                                    pack.y_dim, pack.h1, pack.h2, N.ptr(soft), N.ptr(hard), N.ptr(logits), N.stream()),
                    "dvae_classify_generic_batch")
            return
        N.check(lib.dvae_classify_batch(N.ptr(src), int(is_complex), ld, src.shape[0], off.size - 1, off.ctypes.data, N.ptr(pack.weights), pack.y_dim,
                                        N.ptr(soft), N.ptr(hard), N.ptr(logits), N.stream()), "dvae_classify_batch")


def classify_batch(clf_or_pack, spec_or_rows, counts=None, want_logits=False):
    """The classifier's labels for every frame of a ragged batch -> LabelBatch.

    clf_or_pack: a Classifier on the device (packed here) or its ClassifierPack of either kind (pack once, label many batches;
    pack_classifier picks the kernel).  spec_or_rows: a
    SpecBatch of complex frames (layout 2: |X|^2 is formed in the kernel, McemBatch.X2's bits) or of power frames (layout 1); a
    FrameBatch (its X rows); or float32 CUDA power rows [N, 513] (any row stride >= 513, e.g. DeviceFrames.x) with counts, the
    frames of each utterance laid end to end from row 0 (counts=None: one utterance of all rows).  TypeError naming the shape for a
    classifier the kernel does not cover; ValueError naming the utterance for a table that does not fit the rows."""
    op = "classify_batch"
    pack = clf_or_pack if isinstance(clf_or_pack, ClassifierPack) else ClassifierPack(clf_or_pack)
    if isinstance(spec_or_rows, STFT.SpecBatch):
        if spec_or_rows.layout not in (1, 2):
            raise TypeError(f"{op}: a SpecBatch of power frames (layout 1) or complex frames (layout 2) is required")
        src, counts = spec_or_rows.frames, spec_or_rows.counts
        if not (src.is_cuda and src.dim() == 2 and src.shape[1] == F_BINS and src.dtype == (torch.complex64 if spec_or_rows.layout == 2 else torch.float32)):
            raise TypeError(f"{op}: the SpecBatch's frames must be [sum T_u, 513] on the device, complex64 (layout 2) or float32 (layout 1)")
        src = src.contiguous() if spec_or_rows.layout == 2 else _rows(op, src, "frames", F_BINS)
    else:
        if isinstance(spec_or_rows, TGT.FrameBatch):
            spec_or_rows, counts = spec_or_rows.X, spec_or_rows.counts
        src = _rows(op, spec_or_rows, "rows", F_BINS)
        if counts is None:
            counts = [src.shape[0]]
    off = frame_table(op, counts, src.shape[0])
    if pack.weights.device != src.device:
        raise ValueError(f"{op}: the classifier lives on {pack.weights.device}, the frames on {src.device}")
    soft, hard = (torch.empty((src.shape[0], pack.y_dim), dtype=torch.float32, device=src.device) for _ in range(2))
    logits = torch.empty_like(soft) if want_logits else None
    classify_rows(pack, src, off, soft, hard, logits)
    return LabelBatch(soft, hard, counts, off, logits)


def _label_rows(op, x, name, counts):
    """(rows [N, y_dim], counts) of a LabelBatch (its hard labels), a FrameBatch (its Y) or rows with counts."""
    if isinstance(x, LabelBatch):
        return _rows(op, x.hard, name), x.counts
    if isinstance(x, TGT.FrameBatch):
        return _rows(op, x.Y, name), x.counts
    if torch.is_tensor(x) and x.dim() == 1:
        x = x[:, None]
    return _rows(op, x, name), counts


def label_counts_batch(pred, truth, counts=None):
    """The confusion counts of hard labels per utterance -> int64 CUDA tensor [U, 4] of tp, tn, fp, fn over all y_dim * T_u elements
    (an element counts as 1 when it is not zero).  pred / truth: LabelBatches, FrameBatches (their label rows) or float32 CUDA rows
    [N, y_dim] with counts."""
    op = "f1_batch"
    p, cp = _label_rows(op, pred, "pred", counts)
    t, ct = _label_rows(op, truth, "truth", counts)
    if cp is None or ct is None:
        raise ValueError(f"{op}: rows need the utterances' frame counts")
    if list(cp) != list(ct):
        bad = next((u for u, (a, b) in enumerate(zip(cp, ct)) if a != b), min(len(cp), len(ct)))
        raise ValueError(f"{op}: utterance {bad}: pred and truth differ in their frame counts ({len(cp)} and {len(ct)} utterances)")
    if p.shape[1] != t.shape[1]:
        raise ValueError(f"{op}: pred has y_dim {p.shape[1]}, truth {t.shape[1]}")
    if p.device != t.device:
        raise ValueError(f"{op}: pred lives on {p.device}, truth on {t.device}")
    off = frame_table(op, cp, min(p.shape[0], t.shape[0]))
    U = off.size - 1
    with torch.cuda.device(p.device):
        out = torch.empty((U, 4), dtype=torch.int64, device=p.device)
        off_dev = R.upload(off, p.device)
        N.check(N.load().dvae_label_counts_batch(N.ptr(p), N.ld(p), N.ptr(t), N.ld(t), min(p.shape[0], t.shape[0]), p.shape[1], U, off.ctypes.data,
                                                 N.ptr(off_dev), N.ptr(out), N.stream()), "dvae_label_counts_batch")
    return out


def f1_from_counts(counts, epsilon=1e-8):
    """f1_loss's ratios from its four sums: counts [..., 4] integer tensor of tp, tn, fp, fn -> float32 [..., 4] of accuracy,
    precision, recall, F1: `.to(torch.float32)`, then the four expressions as the reference writes them (utils.py:147-156)."""
    c = counts.to(torch.float32)
    tp, tn, fp, fn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    accuracy = (tp + tn) / (tp + tn + fp + fn + epsilon)
    precision = tp / (tp + fp + epsilon)
    recall = tp / (tp + fn + epsilon)
    f1 = 2 * (precision * recall) / (precision + recall + epsilon)
    return torch.stack([accuracy, precision, recall, f1], dim=-1)


def f1_batch(pred, truth, epsilon=1e-8, counts=None):
    """f1_loss(pred_u.flatten(), truth_u.flatten(), epsilon) of every utterance -> float32 CUDA tensor [U, 4] of accuracy, precision,
    recall, F1, bit for bit.  pred / truth as for label_counts_batch; a FrameBatch from clean_speech_VAD_many / clean_speech_IBM_many
    serves as the truth of a LabelBatch from classify_batch on the same utterances, nothing crossing to the host."""
    return f1_from_counts(label_counts_batch(pred, truth, counts), epsilon)

"""Fused train step for the label classifier alone (include/dvae_train.h: dvae_train_clf_*; csrc/train_classifier.hip):
Classifier([513, [h1, h2], y_dim]) forward, binary cross entropy, backward, weight gradients and Adam in three HIP launches per step,
with the confusion counts of `y_hat_soft > 0.5` from the same pass -- the loop body the reference sketches in
scripts/train_audio_net.py (noisy frames, the clean speech's VAD / IBM labels, BCE, Adam at 1e-4, F1 per batch).  Hidden widths 1..512,
y_dim 1..513, exact fp32: every classifier `classify.pack_classifier` accepts.

`ClassifierTrainer` offers the surface of `trainer_generic.GenericTrainer` where it has meaning here.  PyTorch is plumbing: it owns the
buffers and the stream.  No fallback: a geometry outside the limits or another precision raises with the limits named, before anything
touches the device.
"""
import ctypes

import numpy as np
import torch

from . import clip
from . import native as N
from .trainer import MAXT, PREC_CODE

LIMITS = ("the classifier train step covers Classifier([513, [h1, h2], y_dim]) at x_dim 513, two hidden widths 1..512, y_dim 1..513, "
          "precision fp32, one GPU")
NAMES = ["hidden.0.weight", "hidden.0.bias", "hidden.1.weight", "hidden.1.bias", "output_layer.weight", "output_layer.bias"]
INFO_PREFIX = "enc_dec_clf.classifier."        # the keys scripts/training_M2_info_vad_pretrain.py:102-113 filters a checkpoint for


class ClassifierPlan(ctypes.Structure):
    _fields_ = [("h1", ctypes.c_int32), ("h2", ctypes.c_int32), ("y_dim", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("ksplit", ctypes.c_int32), ("n_tensors", ctypes.c_int32), ("B", ctypes.c_int64), ("n_params", ctypes.c_int64),
                ("tensor_offset", ctypes.c_int64 * MAXT), ("tensor_rows", ctypes.c_int32 * MAXT), ("tensor_cols", ctypes.c_int32 * MAXT),
                ("workspace_bytes", ctypes.c_int64), ("grad_offset_bytes", ctypes.c_int64), ("Bp", ctypes.c_int64), ("rows_grid", ctypes.c_int64),
                ("slice_frames", ctypes.c_int64), ("wgrad_items", ctypes.c_int64), ("lds_bytes", ctypes.c_int64), ("loss_accum", ctypes.c_uint64),
                ("count_accum", ctypes.c_uint64), ("row_index", ctypes.c_uint64), ("row_count", ctypes.c_int64), ("bad_row_counter", ctypes.c_uint64)]


def _dims_of(dims_or_module):
    """[x_dim, [h1, h2], y_dim] from the reference's dims list, or from a Classifier's layers (None where it has another shape)."""
    if isinstance(dims_or_module, torch.nn.Module):
        from .classify import _generic_dims
        d = _generic_dims(dims_or_module)
        return None if d is None else [513, [d[0], d[1]], d[2]]
    try:
        x, h, y = dims_or_module
        return [int(x), [int(v) for v in h], int(y)]
    except (TypeError, ValueError):
        return None


def covered(dims):
    """The geometry limits (host logic only): dims = [513, [h1, h2], y_dim] or a Classifier."""
    d = _dims_of(dims)
    return d is not None and d[0] == 513 and len(d[1]) == 2 and all(1 <= v <= 512 for v in d[1]) and 1 <= d[2] <= 513


def make_plan(dims, batch, precision="fp32", ksplit=0):
    """dvae_train_clf_plan for (dims, batch): host only.  Raises NotImplementedError / ValueError with the library's message."""
    lib = N.load()
    d = _dims_of(dims)
    if d is None or d[0] != 513 or len(d[1]) != 2 or precision not in PREC_CODE:
        raise NotImplementedError(f"{LIMITS}; got {dims if d is None else d} {precision}")
    plan = ClassifierPlan()
    rc = lib.dvae_train_clf_plan(d[1][0], d[1][1], d[2], PREC_CODE[precision], int(batch), int(ksplit), ctypes.byref(plan))
    if rc != 0:
        msg = lib.dvae_last_error().decode("utf-8", "replace")
        raise (NotImplementedError if rc == 1003 else ValueError)(f"{msg} (got {d}, precision {precision})")
    return plan


class ClassifierTrainer:
    """One object = one classifier on one GPU.  step(x, y) enqueues one full train step and returns the device tensor [BCE] (no host
    sync); `counts` then holds the batch's tp, tn, fp, fn (classify.f1_from_counts(tr.counts): accuracy, precision, recall, F1)."""

    def __init__(self, dims_or_module, params=None, batch=128, device="cuda:0", lr=1e-4, betas=(0.9, 0.999), adam_eps=1e-8, bce_eps=1e-8,
                 seed=None, ksplit=0, share=None, precision="fp32", std_norm=None):
        if std_norm is not None:
            raise NotImplementedError("std_norm exists on the generic M1 / M2 step only (trainer_generic.GenericTrainer): the reference never "
                                      f"standardises the classifier's input; {LIMITS}")
        self.plan = make_plan(dims_or_module, batch, precision, ksplit)          # refuses before anything touches the device
        if not torch.cuda.is_available():
            raise RuntimeError("ClassifierTrainer needs the MI355X HIP path (no CPU fallback)")
        self.lib = N.load()
        self.B = int(batch)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.precision, self.ksplit = "fp32", int(ksplit)
        self.lr, self.betas, self.adam_eps, self.bce_eps = lr, betas, adam_eps, bce_eps
        self.y_dim, self.h_dim = self.plan.y_dim, (self.plan.h1, self.plan.h2)
        self.dims = [513, list(self.h_dim), self.y_dim]
        self.names = NAMES
        P = self.plan.n_params
        with torch.cuda.device(self.device):
            if share is None:
                self._params = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._m = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._v = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._shared = {"step_count": 0, "version": 0}
            else:                       # same parameters / Adam state, another batch size (see fork())
                self._params, self._m, self._v, self._shared = share._params, share._m, share._v, share._shared
            self.ws = torch.empty(self.plan.workspace_bytes, dtype=torch.uint8, device=self.device)
            self._losses3 = torch.zeros(3, dtype=torch.float32, device=self.device)       # {BCE, BCE, 0}: the apply kernel's three scalars
            self.losses = self._losses3[:1]
            self.counts = torch.zeros(4, dtype=torch.int64, device=self.device)
            self.bad_rows = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.plan.bad_row_counter = self.bad_rows.data_ptr()
        self._copy_version = self._shared["version"]
        if share is None:
            if params is None:
                params = self._module_params(dims_or_module) if isinstance(dims_or_module, torch.nn.Module) else self._reference_init(seed)
            self._write_params(params)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_init(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()), "dvae_train_clf_init")

    # ---- shared state ----
    params = property(lambda self: self._params)
    m = property(lambda self: self._m)
    v = property(lambda self: self._v)

    @property
    def step_count(self):
        return self._shared["step_count"]

    @step_count.setter
    def step_count(self, v):
        self._shared["step_count"] = v

    def fork(self, batch):
        """A trainer for another batch size over the SAME parameters and Adam moments (the last, shorter batch of an epoch, the
        validation batch size).  Each trainer has its own packed weight copies; they are rebuilt when the other one has stepped."""
        return ClassifierTrainer(self.dims, batch=batch, device=self.device, lr=self.lr, betas=self.betas, adam_eps=self.adam_eps,
                                 bce_eps=self.bce_eps, ksplit=self.ksplit, share=self)

    def _repack(self):
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_repack(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()), "dvae_train_clf_repack")
        self._copy_version = self._shared["version"]

    def _sync_copies(self):
        if self._copy_version != self._shared["version"]:
            self._repack()

    # ---- parameters under Classifier.state_dict()'s names ----
    def _reference_init(self, seed):
        """xavier_normal_ weights / zero bias drawn exactly like constructing Classifier(dims) under the same torch.manual_seed
        (the reference initialises a stand-alone classifier nowhere; this is the init of every model that holds one, models.py:137-141)."""
        from packages.models.models import Classifier, _xavier_reset
        if seed is not None:
            torch.manual_seed(seed)
        m = Classifier(self.dims)
        _xavier_reset(m)
        return {k: v.detach() for k, v in m.state_dict().items()}

    @staticmethod
    def _module_params(module):
        return {k: v.detach() for k, v in module.state_dict().items()}

    def tensor_view(self, i):
        o, r, c = self.plan.tensor_offset[i], self.plan.tensor_rows[i], self.plan.tensor_cols[i]
        v = self._params[o:o + r * c]
        return v.view(r, c) if self.names[i].endswith("weight") else v

    def _write_params(self, sd, strict=True, prefix=""):
        if prefix:                                       # the pretrain script's filter: keys outside the prefix are not ours
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        unknown = [k for k in sd if k not in self.names]
        if strict and unknown:
            raise KeyError(f"unexpected keys in state_dict: {unknown[:4]}")
        for i, name in enumerate(self.names):
            if name not in sd:
                if strict:
                    raise KeyError(f"missing key in state_dict: {prefix}{name}")
                continue
            t = sd[name]
            t = torch.from_numpy(np.array(t)) if isinstance(t, np.ndarray) else t.detach()      # (a copy: the caller's array may be read-only)
            view = self.tensor_view(i)
            if tuple(t.shape) != tuple(view.shape):
                raise ValueError(f"{prefix}{name}: shape {tuple(t.shape)} != {tuple(view.shape)}")
            view.copy_(t.to(torch.float32))

    def load_state_dict(self, sd, strict=True, prefix=""):
        """strict=False overwrites only the tensors present.  prefix="enc_dec_clf.classifier." reads the classifier out of an M2_info
        state_dict (keys outside the prefix are ignored, as the pretrain script's filter ignores them)."""
        self._write_params(sd, strict, prefix)
        self._shared["version"] += 1
        self._repack()

    def state_dict(self, prefix=""):
        """prefix="enc_dec_clf.classifier.": the keys Trainer("M2_info", ...).load_state_dict(sd, strict=False) takes."""
        return {prefix + name: self.tensor_view(i).clone() for i, name in enumerate(self.names)}

    def state_dict_numpy(self, prefix=""):
        return {k: v.cpu().numpy() for k, v in self.state_dict(prefix).items()}

    def to_module(self):
        """A packages.models.models.Classifier on the device with the current weights (classify.pack_classifier / classify_batch)."""
        from packages.models.models import Classifier
        m = Classifier(self.dims).to(self.device)
        m.load_state_dict(self.state_dict(), strict=True)
        return m.eval()

    def losses_host(self):
        """The last step's BCE on the host (synchronises)."""
        return self.losses.cpu().numpy().copy()

    def grads_numpy(self):
        """Gradient of the last step per tensor, as numpy: the frame-slice slabs summed in slab order, as the apply kernel sums them."""
        P, ks, go = self.plan.n_params, self.plan.ksplit, self.plan.grad_offset_bytes
        slabs = self.ws[go:go + 4 * P * ks].view(torch.float32).view(ks, P)
        flat = slabs[0].clone()
        for k in range(1, ks):
            flat += slabs[k]
        flat = flat.cpu().numpy()
        out = {}
        for i, name in enumerate(self.names):
            o, r, c = self.plan.tensor_offset[i], self.plan.tensor_rows[i], self.plan.tensor_cols[i]
            g = flat[o:o + r * c].copy()
            out[name] = g.reshape(r, c) if name.endswith("weight") else g
        return out

    # ---- one train step ----
    def _check_inputs(self, x, y, rows):
        """rows=None: x [B, 513], y [B, y_dim] are the batch.  rows = int64 CUDA tensor [B]: x / y are a whole frame store (e.g.
        DeviceFrames.x / .y) and frame b of the step is row rows[b], gathered inside the kernels: no copy."""
        B = self.B
        n = B if rows is None else x.shape[0]
        if x.ndim != 2 or x.shape != (n, 513) or x.dtype != torch.float32 or x.device != self.device or n < 1:
            raise ValueError(f"x must be a float32 tensor [{n if rows is not None else B}, 513] on {self.device}")
        if y is None or y.shape != (n, self.y_dim) or y.dtype != torch.float32 or y.device != self.device:
            raise ValueError(f"y must be a float32 tensor [{n}, {self.y_dim}] on {self.device}")
        if rows is not None and not (rows.device == self.device and rows.dtype == torch.int64 and rows.shape == (B,) and rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous int64 tensor [{B}] on {self.device}")
        N.check_row_stride(x, 513, "x")                 # here, before a step is counted: the library would refuse only after
        N.check_row_stride(y, self.y_dim, "y")
        self.plan.row_index = 0 if rows is None else rows.data_ptr()
        self.plan.row_count = 0 if rows is None else n
        return (x if x.stride(1) == 1 else x.contiguous()), (y if y.stride(1) == 1 else y.contiguous())

    def bad_row_count(self):
        """Gather indices outside the frame store seen since the last call (synchronises); the affected frames were trained on row 0
        instead.  No kernel reads memory through such an index."""
        n = int(self.bad_rows.item())
        if n:
            self.bad_rows.zero_()
        return n

    def step(self, x, y, rows=None, max_norm=None):
        """max_norm=None: three launches.  A positive number: the global gradient norm is clipped to it on the device
        (torch.nn.utils.clip_grad_norm_ over the six tensors at once; a non-finite gradient skips the update and is counted: clip.py)
        -- rows, weight gradients, reduce into a private flat gradient, norm, guarded apply: five launches, still no host sync."""
        if max_norm is not None:
            max_norm = clip.check_max_norm(max_norm)
            flat = clip.step_flat(self)
            self._micro(flat, 0, 1.0, x, y, rows)
            self._apply_flat_clipped(flat, 1.0, max_norm)
            return self.losses
        x, y = self._check_inputs(x, y, rows)
        self._sync_copies()
        self.step_count += 1
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_step(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v), N.ptr(self.ws),
                                                 N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), self.bce_eps, self.step_count, self.lr, self.betas[0],
                                                 self.betas[1], self.adam_eps, N.ptr(self._losses3), N.ptr(self.counts), N.stream()),
                    "dvae_train_clf_step")
        return self.losses

    def evaluate(self, x, y, rows=None, counts=None):
        """Validation pass: forward, BCE and counts on a batch of the trainer's size, no backward, no update.  Returns a NEW device
        tensor [BCE]; `counts` (this object's) holds the batch's tp, tn, fp, fn.  counts=buf: an int64 CUDA tensor [4] the batch's
        counts are ADDED to on the device -- one buffer over a whole validation set."""
        x, y = self._check_inputs(x, y, rows)
        if counts is not None and not (torch.is_tensor(counts) and counts.device == self.device and counts.dtype == torch.int64
                                       and tuple(counts.shape) == (4,) and counts.is_contiguous()):
            raise ValueError(f"evaluate: counts must be a contiguous int64 tensor [4] on {self.device}")
        self._sync_copies()
        out = torch.zeros_like(self._losses3)
        self.plan.count_accum = 0 if counts is None else counts.data_ptr()
        try:
            with torch.cuda.device(self.device):
                N.check(self.lib.dvae_train_clf_eval(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), self.bce_eps,
                                                     N.ptr(out), N.ptr(self.counts), N.stream()), "dvae_train_clf_eval")
        finally:
            self.plan.count_accum = 0
        return out[:1]

    def grads_only(self, x, y, reduce=False):
        """rows + weight-gradient kernels without the optimizer (tests / gradient inspection; read them with grads_numpy()).
        `reduce` is accepted for the signature of Trainer.grads_only: the slabs are summed on reading either way."""
        x, y = self._check_inputs(x, y, None)
        self._sync_copies()
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), self.bce_eps,
                                                  N.stream()), "dvae_train_clf_grads")

    # ---- accumulate.AccumulatedStep ----
    def _micro(self, flat, accumulate, weight, x, y, rows):
        """One micro-batch: rows + weight-gradient + reduce launches; the slabs go into `flat` (accumulate 0: overwritten), the
        micro-batch's BCE into self.losses and its counts into self.counts."""
        x, y = self._check_inputs(x, y, rows)
        self._sync_copies()
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), self.bce_eps,
                                                  N.stream()), "dvae_train_clf_grads")
            N.check(self.lib.dvae_train_clf_reduce(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(flat), int(accumulate), float(weight),
                                                   N.ptr(self._losses3), N.ptr(self.counts), N.stream()), "dvae_train_clf_reduce")
        return self.losses

    def _apply_flat(self, flat, grad_scale):
        """One Adam step on g = grad_scale * flat; counts as a step exactly as step() does."""
        self.step_count += 1
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]          # the apply kernel rewrites every element of this trainer's packed copies
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_clf_apply_flat(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v),
                                                       N.ptr(self.ws), N.ptr(flat), self.step_count, self.lr, self.betas[0], self.betas[1],
                                                       self.adam_eps, float(grad_scale), N.stream()), "dvae_train_clf_apply_flat")

    def _apply_flat_clipped(self, flat, grad_scale, max_norm):
        """_apply_flat with the global norm of grad_scale * flat clipped to max_norm on the device (clip.py)."""
        clip.apply_flat_clipped(self, "clf", flat, grad_scale, max_norm)

    grad_norm = property(lambda self: clip.state(self)["grad_norm"],
                         doc="Device float32 [total_norm, coef] of the last clipped step of this trainer or a fork (no host sync).")

    def skipped_step_count(self):
        """Clipped steps the device skipped for a non-finite gradient since the last call (synchronises; shared with forks).  A skipped
        step leaves parameters, moments and packed copies untouched but still counts in step_count."""
        return clip.skipped_step_count(self)

    def accumulate_losses(self, buf):
        """Running sum for epoch logging without a host sync per step: `buf` is a float64 CUDA tensor of 8 elements (or None to stop);
        every step() / evaluate() adds its BCE to buf[0] on the device (buf[1] receives it too: the apply kernel's second scalar)."""
        if buf is not None and not (buf.is_cuda and buf.dtype == torch.float64 and buf.numel() >= 8 and buf.is_contiguous()):
            raise ValueError("accumulate_losses: need a contiguous float64 CUDA tensor with >= 8 elements")
        self._accum = buf
        self.plan.loss_accum = 0 if buf is None else buf.data_ptr()

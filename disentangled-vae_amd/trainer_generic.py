"""Fused train step for M1 / M2 models of any covered size (include/dvae_train.h: dvae_train_generic_*; csrc/train_generic.hip):
forward, elbo, backward, weight gradients and Adam in three HIP launches per step whatever the geometry -- x 513, y_dim 0 (M1) or
1..513 (M2), hidden widths 1..512, z_dim 1..128, two tanh layers a side, exact fp32.

`GenericTrainer` offers the surface of `trainer.Trainer` where it has meaning here; `trainer.make_trainer` chooses between the two.
PyTorch is plumbing: it owns the buffers and the stream, and draws the reparametrisation noise when none is passed.  No fallback:
a geometry outside the limits, another model or a 16-bit operand policy raises with the limits named.
"""
import ctypes

import numpy as np
import torch

from . import clip
from . import kl_weight as KL
from . import native as N
from .trainer import MAXT, MODEL_CODE, PREC_CODE, TENSOR_NAMES

LIMITS = ("the generic train step covers M1 (y_dim 0) and M2 (y_dim 1..513) at x_dim 513, two hidden widths 1..512, z_dim 1..128, "
          "precision fp32, one GPU")


class GenericPlan(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("y_dim", ctypes.c_int32), ("z_dim", ctypes.c_int32), ("h1", ctypes.c_int32), ("h2", ctypes.c_int32),
                ("precision", ctypes.c_int32), ("ksplit", ctypes.c_int32), ("n_tensors", ctypes.c_int32), ("B", ctypes.c_int64),
                ("n_params", ctypes.c_int64), ("tensor_offset", ctypes.c_int64 * MAXT), ("tensor_rows", ctypes.c_int32 * MAXT),
                ("tensor_cols", ctypes.c_int32 * MAXT), ("workspace_bytes", ctypes.c_int64), ("grad_offset_bytes", ctypes.c_int64),
                ("Bp", ctypes.c_int64), ("rows_grid", ctypes.c_int64), ("slice_frames", ctypes.c_int64), ("wgrad_items", ctypes.c_int64),
                ("lds_bytes", ctypes.c_int64), ("loss_accum", ctypes.c_uint64), ("row_index", ctypes.c_uint64), ("row_count", ctypes.c_int64),
                ("bad_row_counter", ctypes.c_uint64), ("std_norm", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("norm_mean", ctypes.c_uint64),
                ("norm_div", ctypes.c_uint64), ("kl_weight", ctypes.c_double), ("kl_floor", ctypes.c_double)]


def covered(model, dims):
    """The geometry limits (host logic only)."""
    h = tuple(dims.get("h_dim", ()))
    y = dims.get("y_dim", 0) or 0
    return (model in ("M1", "M2") and dims.get("x_dim") == 513 and len(h) == 2 and all(1 <= int(v) <= 512 for v in h)
            and 1 <= int(dims.get("z_dim", 0)) <= 128 and ((model == "M1" and y == 0) or (model == "M2" and 1 <= int(y) <= 513)))


def check_std_norm(std_norm, norm_eps=1e-8, who="std_norm"):
    """(mean, div) float32 numpy vectors [513] of std_norm=(mean, std): div = fl32(std + fl32(norm_eps)), formed here once in float32 as
    torch forms `std + eps`.  mean, std: 513 finite floats each, std >= 0, numpy arrays or tensors on any device (shape [513] or the
    file's (513, 1)).  ValueError otherwise; host only."""
    try:
        mean, std = std_norm
    except (TypeError, ValueError):
        raise ValueError(f"{who}: a pair (mean, std) of 513 floats each is expected") from None
    out = []
    for name, t in (("mean", mean), ("std", std)):
        if torch.is_tensor(t):
            t = t.detach().cpu().numpy()
        try:
            a = np.asarray(t)
            if a.dtype.kind not in "fiu":
                raise TypeError
            a = a.astype(np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {name} must be 513 floats (a numpy array or a tensor)") from None
        if a.size != 513 or not np.all(np.isfinite(a)):
            raise ValueError(f"{who}: {name} must be 513 finite floats, got {a.size} values" + ("" if a.size != 513 else ", some not finite"))
        out.append(a)
    mean, std = out
    if np.any(std < 0):
        raise ValueError(f"{who}: std must be >= 0")
    eps = np.float32(norm_eps)
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"{who}: norm_eps {norm_eps!r} (a finite number >= 0)")
    div = (std + eps).astype(np.float32)
    if np.any(div == 0):
        raise ValueError(f"{who}: std + norm_eps is zero in {int(np.sum(div == 0))} bins: the encoder input would not be finite")
    return mean, div, std


def make_plan(model, dims, batch, precision="fp32", ksplit=0, std_norm=False):
    """dvae_train_generic_plan[_norm] for (model, dims, batch): host only.  Raises NotImplementedError / ValueError with the library's message."""
    lib = N.load()
    if model not in MODEL_CODE or precision not in PREC_CODE:
        raise NotImplementedError(f"{LIMITS}; got {model} {precision}")
    h = tuple(dims["h_dim"])
    if dims.get("x_dim") != 513 or len(h) != 2:
        raise NotImplementedError(f"{LIMITS}; got {model} {dims}")
    plan = GenericPlan()
    args = (MODEL_CODE[model], 0 if model == "M1" else int(dims["y_dim"]), int(dims["z_dim"]), int(h[0]), int(h[1]), PREC_CODE[precision],
            int(batch), int(ksplit))
    if std_norm:
        rc = lib.dvae_train_generic_plan_norm(*args, 1, ctypes.byref(plan))
    else:                               # the entry point, and so the plan, of a trainer without the switch is the one it always was
        rc = lib.dvae_train_generic_plan(*args, ctypes.byref(plan))
    if rc != 0:
        msg = lib.dvae_last_error().decode("utf-8", "replace")
        raise (NotImplementedError if rc == 1003 else ValueError)(f"{msg} (got {model} {dims}, precision {precision})")
    return plan


class GenericTrainer(KL.KLOptions):
    """One object = one model replica on one GPU.  step(x, y, eps_noise) enqueues one full train step and returns a device tensor
    [ELBO, recon, KL] (no host sync).

    kl_weight, kl_warmup, kl_floor (kl_weight.py): the objective is recon + w_s * mean_b sum_j max(k_bj, kl_floor) with
    w_s = kl_weight * min(1, s / kl_warmup) at optimizer step s; the ELBO slot is that objective, the recon and KL slots stay the raw
    means; evaluate() uses the target kl_weight.  The defaults (1, 0, 0) are the unweighted step, bit for bit.  kl_weight may be
    reassigned between steps, kl_weight_next is the weight the next optimizer step will use; forks share the options and the schedule;
    none of the three is part of state_dict().

    std_norm=(mean, std) (513 floats each; check_std_norm) is the scripts' switch of that name: the encoder reads
    [(x - mean) / (std + norm_eps) | y], the float32 bits of torch's expression, while the loss is scored against the raw x
    (scripts/training_M2.py:136-144).  Every method works as without it; state_dict() keeps the reference's keys only -- the tables
    are data of the train set, read back with .std_norm."""

    def __init__(self, model, dims, params=None, batch=128, device="cuda:0", lr=1e-4, betas=(0.9, 0.999), adam_eps=1e-8, elbo_eps=1e-8,
                 seed=None, ksplit=0, share=None, precision="fp32", world=1, std_norm=None, norm_eps=1e-8, kl_weight=1.0, kl_warmup=0,
                 kl_floor=0.0):
        KL.check_options(kl_weight, kl_warmup, kl_floor, "GenericTrainer")      # ValueError before anything touches the device
        if int(world) != 1:
            raise NotImplementedError(f"data-parallel training is not built on the generic step ({LIMITS}); got world={world}: wrap a "
                                      "one-GPU trainer per rank in accumulate.AccumulatedStep(trainer, process_group)")
        tables = check_std_norm(std_norm, norm_eps, "GenericTrainer: std_norm") if std_norm is not None and share is None else None
        self.plan = make_plan(model, dims, batch, precision, ksplit,          # refuses before anything touches the device
                              std_norm=tables is not None or (share is not None and share._norm is not None))
        if not torch.cuda.is_available():
            raise RuntimeError("GenericTrainer needs the MI355X HIP path (no CPU fallback)")
        self.lib = N.load()
        self.model, self.dims, self.B = model, dict(dims), int(batch)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.precision, self.world, self.ksplit = "fp32", 1, int(ksplit)
        self.lr, self.betas, self.adam_eps, self.elbo_eps = lr, betas, adam_eps, elbo_eps
        self.y_dim, self.z_dim, self.h_dim = self.plan.y_dim, self.plan.z_dim, (self.plan.h1, self.plan.h2)
        self.names = TENSOR_NAMES
        P = self.plan.n_params
        with torch.cuda.device(self.device):
            if share is None:
                self._params = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._m = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._v = torch.zeros(P, dtype=torch.float32, device=self.device)
                self._shared = {"step_count": 0, "version": 0}
            else:                       # same parameters / Adam state, another batch size (see fork())
                self._params, self._m, self._v, self._shared = share._params, share._m, share._v, share._shared
            self._kl_init(kl_weight, kl_warmup, kl_floor, share)
            self.ws = torch.empty(self.plan.workspace_bytes, dtype=torch.uint8, device=self.device)
            self.losses = torch.zeros(3, dtype=torch.float32, device=self.device)
            self.bad_rows = torch.zeros(1, dtype=torch.int32, device=self.device)
            if share is not None:
                self._norm = share._norm                    # (mean, div, std) on the device: a fork carries the tables
            elif tables is not None:
                self._norm = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in tables)
            else:
                self._norm = None
        self.norm_eps = share.norm_eps if share is not None else norm_eps
        self.plan.bad_row_counter = self.bad_rows.data_ptr()
        if self._norm is not None:
            self.plan.norm_mean, self.plan.norm_div = self._norm[0].data_ptr(), self._norm[1].data_ptr()
        self.seed = int(seed) if seed is not None else (share.seed if share is not None else int(torch.initial_seed()))
        self._copy_version = self._shared["version"]
        if share is None:
            if params is None:
                params = self._reference_init(seed)
            self._write_params(params)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_init(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()),
                    "dvae_train_generic_init")

    # ---- shared state ----
    params = property(lambda self: self._params)
    m = property(lambda self: self._m)
    v = property(lambda self: self._v)

    @property
    def step_count(self):
        return self._shared["step_count"]

    @property
    def std_norm(self):
        """(mean, std) as given, float32 device tensors [513], or None."""
        return None if self._norm is None else (self._norm[0], self._norm[2])

    @step_count.setter
    def step_count(self, v):
        self._shared["step_count"] = v

    def fork(self, batch):
        """A trainer for another batch size over the SAME parameters and Adam moments (the last, shorter batch of an epoch, the
        validation batch size).  Each trainer has its own packed weight copies; they are rebuilt when the other one has stepped."""
        return GenericTrainer(self.model, self.dims, batch=batch, device=self.device, lr=self.lr, betas=self.betas, adam_eps=self.adam_eps,
                              elbo_eps=self.elbo_eps, ksplit=self.ksplit, share=self)

    def _repack(self):
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_repack(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()),
                    "dvae_train_generic_repack")
        self._copy_version = self._shared["version"]

    def _sync_copies(self):
        if self._copy_version != self._shared["version"]:
            self._repack()

    # ---- parameters under the reference's state_dict names ----
    def _reference_init(self, seed):
        """xavier_normal_ weights / zero bias drawn exactly like the drop-in module of the same dims constructs them."""
        from .synth import build_model
        if seed is not None:
            torch.manual_seed(seed)
        m = build_model(self.model, dict(self.dims, y_dim=self.y_dim))
        return {k: v.detach() for k, v in m.state_dict().items()}

    def tensor_view(self, i):
        o, r, c = self.plan.tensor_offset[i], self.plan.tensor_rows[i], self.plan.tensor_cols[i]
        v = self._params[o:o + r * c]
        return v.view(r, c) if self.names[i].endswith("weight") else v

    def _write_params(self, sd, strict=True):
        unknown = [k for k in sd if k not in self.names]
        if strict and unknown:
            raise KeyError(f"unexpected keys in state_dict: {unknown[:4]}")
        for i, name in enumerate(self.names):
            if name not in sd:
                if strict:
                    raise KeyError(f"missing key in state_dict: {name}")
                continue
            t = sd[name]
            t = torch.from_numpy(np.array(t)) if isinstance(t, np.ndarray) else t.detach()      # (a copy: the caller's array may be read-only)
            view = self.tensor_view(i)
            if tuple(t.shape) != tuple(view.shape):
                raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(view.shape)}")
            view.copy_(t.to(torch.float32))

    def load_state_dict(self, sd, strict=True):
        """strict=False overwrites only the tensors present."""
        self._write_params(sd, strict)
        self._shared["version"] += 1
        self._repack()

    def state_dict(self):
        return {name: self.tensor_view(i).clone() for i, name in enumerate(self.names)}

    def state_dict_numpy(self):
        return {k: v.cpu().numpy() for k, v in self.state_dict().items()}

    def losses_host(self):
        """The last step's loss scalars on the host (synchronises)."""
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
    def _check_inputs(self, x, y, rows, eps_noise):
        """rows=None: x [B, 513], y [B, y_dim] are the batch.  rows = int64 CUDA tensor [B]: x / y are a whole frame store and frame b
        of the step is row rows[b], gathered inside the kernels: no copy."""
        B = self.B
        n = B if rows is None else x.shape[0]
        if x.ndim != 2 or x.shape != (n, 513) or x.dtype != torch.float32 or x.device != self.device or n < 1:
            raise ValueError(f"x must be a float32 tensor [{n if rows is not None else B}, 513] on {self.device}")
        if self.y_dim:
            if y is None or y.shape != (n, self.y_dim) or y.dtype != torch.float32 or y.device != self.device:
                raise ValueError(f"y must be a float32 tensor [{n}, {self.y_dim}] on {self.device}")
        if eps_noise is not None and (eps_noise.shape != (B, self.z_dim) or eps_noise.dtype != torch.float32 or eps_noise.device != self.device):
            raise ValueError(f"eps_noise must be a float32 tensor [{B}, {self.z_dim}] on {self.device}")
        if rows is not None and not (rows.device == self.device and rows.dtype == torch.int64 and rows.shape == (B,) and rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous int64 tensor [{B}] on {self.device}")
        N.check_row_stride(x, 513, "x")                 # here, before a step is counted: the library would refuse only after
        if self.y_dim:
            N.check_row_stride(y, self.y_dim, "y")
        self.plan.row_index = 0 if rows is None else rows.data_ptr()
        self.plan.row_count = 0 if rows is None else n

    def bad_row_count(self):
        """Gather indices outside the frame store seen since the last call (synchronises); the affected frames were trained on row 0
        instead.  No kernel reads memory through such an index."""
        n = int(self.bad_rows.item())
        if n:
            self.bad_rows.zero_()
        return n

    def noise(self, step):
        """The [B, z_dim] noise step() / evaluate() use when none is passed: torch.randn on the device from a generator seeded with
        (seed, step); the k-th evaluate() without noise draws noise(2**40 + k)."""
        g = torch.Generator(device=self.device).manual_seed((self.seed * 0x9E3779B97F4A7C15 + int(step)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randn((self.B, self.z_dim), generator=g, device=self.device, dtype=torch.float32)

    def _inputs(self, x, y, eps_noise):
        x = x if x.stride(1) == 1 else x.contiguous()
        yp, ldy = (None, 0)
        if self.y_dim:
            y = y if y.stride(1) == 1 else y.contiguous()
            yp, ldy = N.ptr(y), N.ld(y)
        return x, y, yp, ldy, eps_noise.contiguous()

    def step(self, x, y=None, eps_noise=None, rows=None, max_norm=None):
        """max_norm=None: three launches.  A positive number: the global gradient norm is clipped to it on the device
        (torch.nn.utils.clip_grad_norm_ over all tensors at once; a non-finite gradient skips the update and is counted: clip.py) --
        rows, weight gradients, reduce into a private flat gradient, norm, guarded apply: five launches, still no host sync."""
        if max_norm is not None:
            max_norm = clip.check_max_norm(max_norm)
            if eps_noise is None:
                eps_noise = self.noise(self.step_count + 1)
            flat = clip.step_flat(self)
            self._micro(flat, 0, 1.0, x, y, eps_noise, rows)
            self._apply_flat_clipped(flat, 1.0, max_norm)
            return self.losses
        self._check_inputs(x, y, rows, eps_noise)
        self._sync_copies()
        self.step_count += 1
        if eps_noise is None:
            eps_noise = self.noise(self.step_count)
        x, y, yp, ldy, eps_noise = self._inputs(x, y, eps_noise)
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]
        self._kl_plan(self.step_count)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_step(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v), N.ptr(self.ws),
                                                     N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps_noise), self.elbo_eps, self.step_count, self.lr,
                                                     self.betas[0], self.betas[1], self.adam_eps, N.ptr(self.losses), N.stream()),
                    "dvae_train_generic_step")
        return self.losses

    def evaluate(self, x, y=None, eps_noise=None, rows=None):
        """Validation pass: forward + elbo on a batch of the trainer's size, no backward, no update.  Returns a NEW device tensor
        [ELBO, recon, KL]."""
        self._check_inputs(x, y, rows, eps_noise)
        self._sync_copies()
        if eps_noise is None:
            self._shared["eval_count"] = self._shared.get("eval_count", 0) + 1
            eps_noise = self.noise((1 << 40) + self._shared["eval_count"])
        x, y, yp, ldy, eps_noise = self._inputs(x, y, eps_noise)
        out = torch.zeros_like(self.losses)
        self._kl_plan(None)                             # the target weight: validation curves are comparable across epochs
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_eval(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps_noise),
                                                     self.elbo_eps, N.ptr(out), N.stream()), "dvae_train_generic_eval")
        return out

    def grads_only(self, x, y, eps_noise, reduce=False):
        """rows + weight-gradient kernels without the optimizer (tests / gradient inspection; read them with grads_numpy()).
        `reduce` is accepted for the signature of Trainer.grads_only: the slabs are summed on reading either way."""
        self._check_inputs(x, y, None, eps_noise)
        self._sync_copies()
        x, y, yp, ldy, eps_noise = self._inputs(x, y, eps_noise)
        self._kl_plan(self.step_count + 1)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps_noise),
                                                      self.elbo_eps, N.stream()), "dvae_train_generic_grads")

    # ---- accumulate.AccumulatedStep ----
    def _micro(self, flat, accumulate, weight, x, y, eps_noise, rows):
        """One micro-batch: rows + weight-gradient + reduce launches; the slabs go into `flat` (accumulate 0: overwritten) and the
        micro-batch's losses into self.losses."""
        self._check_inputs(x, y, rows, eps_noise)
        self._sync_copies()
        x, y, yp, ldy, eps_noise = self._inputs(x, y, eps_noise)
        self._kl_plan(self.step_count + 1)              # the weight of the optimizer step this micro-batch ends in
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps_noise),
                                                      self.elbo_eps, N.stream()), "dvae_train_generic_grads")
            N.check(self.lib.dvae_train_generic_reduce(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(flat), int(accumulate), float(weight),
                                                       N.ptr(self.losses), N.stream()), "dvae_train_generic_reduce")
        return self.losses

    def _apply_flat(self, flat, grad_scale):
        """One Adam step on g = grad_scale * flat; counts as a step exactly as step() does."""
        self.step_count += 1
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]          # the apply kernel rewrites every element of this trainer's packed copies
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_generic_apply_flat(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v),
                                                           N.ptr(self.ws), N.ptr(flat), self.step_count, self.lr, self.betas[0], self.betas[1],
                                                           self.adam_eps, float(grad_scale), N.stream()), "dvae_train_generic_apply_flat")

    def _apply_flat_clipped(self, flat, grad_scale, max_norm):
        """_apply_flat with the global norm of grad_scale * flat clipped to max_norm on the device (clip.py)."""
        clip.apply_flat_clipped(self, "generic", flat, grad_scale, max_norm)

    grad_norm = property(lambda self: clip.state(self)["grad_norm"],
                         doc="Device float32 [total_norm, coef] of the last clipped step of this trainer or a fork (no host sync).")

    def skipped_step_count(self):
        """Clipped steps the device skipped for a non-finite gradient since the last call (synchronises; shared with forks).  A skipped
        step leaves parameters, moments and packed copies untouched but still counts in step_count."""
        return clip.skipped_step_count(self)

    def accumulate_losses(self, buf):
        """Running sums for epoch logging without a host sync per step: `buf` is a float64 CUDA tensor of 8 elements (or None to stop);
        every step() / evaluate() adds its loss scalars to its first three on the device."""
        if buf is not None and not (buf.is_cuda and buf.dtype == torch.float64 and buf.numel() >= 8 and buf.is_contiguous()):
            raise ValueError("accumulate_losses: need a contiguous float64 CUDA tensor with >= 8 elements")
        self._accum = buf
        self.plan.loss_accum = 0 if buf is None else buf.data_ptr()

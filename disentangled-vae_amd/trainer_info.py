"""Fused train step for M2_info models of any covered size (include/dvae_train.h: dvae_train_info_*; csrc/train_info.hip): the loop
body of scripts/training_M2_info_vad.py:159-198 on DeepGenerativeModel_v5 -- encoder on x, decoder on [z | y], a relu classifier on x, an
adversarial auxiliary relu classifier on z; enc_loss = ELBO + alpha BCE(clf(x), y) - beta BCE(aux(z), y), aux_loss = gamma BCE(aux(z), y),
the auxiliary net stepped with (gamma - beta) dBCE, one Adam update over all 26 tensors -- in three HIP launches per step whatever the
geometry: x 513, y_dim 1..513, hidden widths 1..512, z_dim 1..128, exact fp32, one GPU.

Two independent options give the other loop bodies the reference trains M2_info with (include/dvae_train.h: dvae_train_info_plan_mode):
`dec_label="classifier"` feeds the decoder [z | clf(x)] instead of [z | y], so that the reconstruction gradient trains the classifier
(scripts/training_M2_info_vad_pretrain.py:162-163), and `aux_enc="uniform"` / `"entropy"` replace the adversarial cross entropy on the
encoder by binary_cross_entropy_v2 / _v3 of aux(z) (line 175; the caller passes gamma = beta for that script).  The defaults,
"truth" and "bce", are the step described above, bit for bit.

`InfoTrainer` offers the surface of `trainer_generic.GenericTrainer` where it has meaning here; `make_info_trainer` chooses between it and
the resident `trainer.Trainer("M2_info", ...)`, which stays the default at the reference geometry and is the only home of the 16-bit
operand policies and of data-parallel training.  PyTorch is plumbing: it owns the buffers and the stream, and draws the reparametrisation
noise when none is passed.  No fallback: a geometry outside the limits raises with the limits named, before anything touches the device.
"""
import ctypes

import numpy as np
import torch

from . import clip
from . import kl_weight as KL
from . import native as N
from .trainer import INFO_NAMES, MAXT, Trainer, supported

LIMITS = ("the generic M2_info train step covers DeepGenerativeModel_v5 at x_dim 513, y_dim 1..513, two hidden widths 1..512, z_dim 1..128, "
          "precision fp32, one GPU")


class InfoPlan(ctypes.Structure):
    _fields_ = [("y_dim", ctypes.c_int32), ("z_dim", ctypes.c_int32), ("h1", ctypes.c_int32), ("h2", ctypes.c_int32), ("ksplit", ctypes.c_int32),
                ("n_tensors", ctypes.c_int32), ("launches_per_step", ctypes.c_int32), ("info_mode", ctypes.c_int32), ("B", ctypes.c_int64),
                ("n_params", ctypes.c_int64), ("tensor_offset", ctypes.c_int64 * MAXT), ("tensor_rows", ctypes.c_int32 * MAXT),
                ("tensor_cols", ctypes.c_int32 * MAXT), ("workspace_bytes", ctypes.c_int64), ("grad_offset_bytes", ctypes.c_int64),
                ("Bp", ctypes.c_int64), ("rows_grid", ctypes.c_int64), ("slice_frames", ctypes.c_int64), ("wgrad_items", ctypes.c_int64),
                ("lds_bytes", ctypes.c_int64), ("info_alpha", ctypes.c_double), ("info_beta", ctypes.c_double), ("info_gamma", ctypes.c_double),
                ("loss_accum", ctypes.c_uint64), ("row_index", ctypes.c_uint64), ("row_count", ctypes.c_int64), ("bad_row_counter", ctypes.c_uint64),
                ("kl_weight", ctypes.c_double), ("kl_floor", ctypes.c_double)]


def covered(dims):
    """The geometry limits (host logic only)."""
    try:
        h = tuple(dims.get("h_dim", ()))
        return (dims.get("x_dim") == 513 and len(h) == 2 and all(1 <= int(v) <= 512 for v in h) and 1 <= int(dims.get("z_dim", 0)) <= 128
                and 1 <= int(dims.get("y_dim", 0) or 0) <= 513)
    except (TypeError, ValueError):
        return False


DEC_LABELS = {"truth": 0, "classifier": 1}              # the DVAE_INFO_* bits of include/dvae_train.h
AUX_ENCS = {"bce": 0, "uniform": 2, "entropy": 4}


def mode_bits(dec_label="truth", aux_enc="bce"):
    """The mode of dvae_train_info_plan_mode for the two options; ValueError naming the choices for any other value (host logic only)."""
    if dec_label not in DEC_LABELS:
        raise ValueError(f"dec_label {dec_label!r}: the choices are {sorted(DEC_LABELS)}")
    if aux_enc not in AUX_ENCS:
        raise ValueError(f"aux_enc {aux_enc!r}: the choices are {sorted(AUX_ENCS)}")
    return DEC_LABELS[dec_label] | AUX_ENCS[aux_enc]


def make_plan(dims, batch, ksplit=0, dec_label="truth", aux_enc="bce"):
    """dvae_train_info_plan_mode for (dims, batch) and the two options: host only.  Raises NotImplementedError / ValueError with the
    library's message."""
    mode = mode_bits(dec_label, aux_enc)
    lib = N.load()
    h = tuple(dims.get("h_dim", ()))
    if dims.get("x_dim") != 513 or len(h) != 2:
        raise NotImplementedError(f"{LIMITS}; got {dims}")
    plan = InfoPlan()
    rc = lib.dvae_train_info_plan_mode(int(dims.get("y_dim", 0) or 0), int(dims["z_dim"]), int(h[0]), int(h[1]), int(batch), int(ksplit), mode,
                                       ctypes.byref(plan))
    if rc != 0:
        msg = lib.dvae_last_error().decode("utf-8", "replace")
        raise (NotImplementedError if rc == 1003 else ValueError)(f"{msg} (got {dims})")
    return plan


class InfoTrainer(KL.KLOptions):
    """One object = one M2_info replica on one GPU.  step(x, y, eps_noise) enqueues one full train step and returns the device tensor
    [ELBO, recon, KL, enc_loss, classif_loss, aux_loss, aux_enc_loss, 0] (no host sync).

    kl_weight, kl_warmup, kl_floor (kl_weight.py; `beta` is the adversarial weight here): the ELBO of the VAE body is
    recon + w_s * mean_b sum_j max(k_bj, kl_floor), in the ELBO slot and inside enc_loss; the recon and KL slots stay the raw means;
    evaluate() uses the target kl_weight.  The defaults (1, 0, 0) are the unweighted step, bit for bit; forks share the options and
    the schedule; they are not part of state_dict()."""

    model = "M2_info"

    def __init__(self, dims, params=None, batch=128, device="cuda:0", lr=1e-4, betas=(0.9, 0.999), adam_eps=1e-8, elbo_eps=1e-8,
                 alpha=0.0, beta=10.0, gamma=1.0, seed=None, ksplit=0, share=None, dec_label="truth", aux_enc="bce", std_norm=None,
                 kl_weight=1.0, kl_warmup=0, kl_floor=0.0):
        if std_norm is not None:
            raise NotImplementedError(STD_NORM_REFUSAL)
        KL.check_options(kl_weight, kl_warmup, kl_floor, "InfoTrainer")         # ValueError before anything touches the device
        self.plan = make_plan(dims, batch, ksplit, dec_label, aux_enc)      # refuses before anything touches the device
        self.dec_label, self.aux_enc = dec_label, aux_enc
        self.plan.info_alpha, self.plan.info_beta, self.plan.info_gamma = float(alpha), float(beta), float(gamma)
        if not torch.cuda.is_available():
            raise RuntimeError("InfoTrainer needs the MI355X HIP path (no CPU fallback)")
        self.lib = N.load()
        self.dims, self.B = dict(dims), int(batch)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.precision, self.world, self.ksplit = "fp32", 1, int(ksplit)
        self.lr, self.betas, self.adam_eps, self.elbo_eps = lr, betas, adam_eps, elbo_eps
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), float(gamma)
        self.y_dim, self.z_dim, self.h_dim = self.plan.y_dim, self.plan.z_dim, (self.plan.h1, self.plan.h2)
        self.names = INFO_NAMES
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
            self.losses = torch.zeros(8, dtype=torch.float32, device=self.device)
            self.bad_rows = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.plan.bad_row_counter = self.bad_rows.data_ptr()
        self.seed = int(seed) if seed is not None else (share.seed if share is not None else int(torch.initial_seed()))
        self._copy_version = self._shared["version"]
        if share is None:
            if params is None:
                params = self._reference_init(seed)
            self._write_params(params)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_init(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()), "dvae_train_info_init")

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
        return InfoTrainer(self.dims, batch=batch, device=self.device, lr=self.lr, betas=self.betas, adam_eps=self.adam_eps,
                           elbo_eps=self.elbo_eps, alpha=self.alpha, beta=self.beta, gamma=self.gamma, ksplit=self.ksplit, share=self,
                           dec_label=self.dec_label, aux_enc=self.aux_enc)

    def _repack(self):
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_repack(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self.ws), N.stream()),
                    "dvae_train_info_repack")
        self._copy_version = self._shared["version"]

    def _sync_copies(self):
        if self._copy_version != self._shared["version"]:
            self._repack()

    # ---- parameters under the reference's state_dict names ----
    def _reference_init(self, seed):
        """xavier_normal_ weights / zero bias drawn exactly like synth.build_model("M2_info", dims) constructs them."""
        from .synth import build_model
        if seed is not None:
            torch.manual_seed(seed)
        m = build_model("M2_info", dict(self.dims, y_dim=self.y_dim))
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
        """strict=False overwrites only the tensors present (the pretrain flow of scripts/training_M2_info_vad_pretrain.py:102-112, e.g.
        ClassifierTrainer.state_dict(prefix="enc_dec_clf.classifier."))."""
        self._write_params(sd, strict)
        self._shared["version"] += 1
        self._repack()

    def state_dict(self):
        return {name: self.tensor_view(i).clone() for i, name in enumerate(self.names)}

    def state_dict_numpy(self):
        return {k: v.cpu().numpy() for k, v in self.state_dict().items()}

    def losses_host(self):
        """The last step's eight loss scalars on the host (synchronises)."""
        return self.losses.cpu().numpy().copy()

    def grads_numpy(self):
        """Gradient of the last step per tensor, as numpy: the frame-slice slabs summed in slab order, as the apply kernel sums them.
        The auxiliary tensors hold (gamma - beta) dBCE -- gamma dBCE - beta dV under aux_enc "uniform" / "entropy" --, what the script's
        second optimizer steps with, as on the resident trainer."""
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
        if y is None or y.shape != (n, self.y_dim) or y.dtype != torch.float32 or y.device != self.device:
            raise ValueError(f"y must be a float32 tensor [{n}, {self.y_dim}] on {self.device}")
        if eps_noise is not None and (eps_noise.shape != (B, self.z_dim) or eps_noise.dtype != torch.float32 or eps_noise.device != self.device):
            raise ValueError(f"eps_noise must be a float32 tensor [{B}, {self.z_dim}] on {self.device}")
        if rows is not None and not (rows.device == self.device and rows.dtype == torch.int64 and rows.shape == (B,) and rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous int64 tensor [{B}] on {self.device}")
        N.check_row_stride(x, 513, "x")                 # here, before a step is counted: the library would refuse only after
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

    @staticmethod
    def _inputs(x, y, eps_noise):
        return (x if x.stride(1) == 1 else x.contiguous()), (y if y.stride(1) == 1 else y.contiguous()), eps_noise.contiguous()

    def step(self, x, y, eps_noise=None, rows=None, max_norm=None):
        """max_norm=None: three launches.  A positive number: the global gradient norm is clipped to it on the device
        (torch.nn.utils.clip_grad_norm_ over all 26 tensors at once; a non-finite gradient skips the update and is counted: clip.py)
        -- rows, weight gradients, reduce into a private flat gradient, norm, guarded apply: five launches, still no host sync."""
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
        x, y, eps_noise = self._inputs(x, y, eps_noise)
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]
        self._kl_plan(self.step_count)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_step(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v), N.ptr(self.ws),
                                                  N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), N.ptr(eps_noise), self.elbo_eps, self.step_count, self.lr,
                                                  self.betas[0], self.betas[1], self.adam_eps, N.ptr(self.losses), N.stream()),
                    "dvae_train_info_step")
        return self.losses

    def evaluate(self, x, y, eps_noise=None, rows=None):
        """Validation pass: the forward passes and the losses on a batch of the trainer's size, no backward, no update.  Returns a NEW
        device tensor of the eight loss scalars."""
        self._check_inputs(x, y, rows, eps_noise)
        self._sync_copies()
        if eps_noise is None:
            self._shared["eval_count"] = self._shared.get("eval_count", 0) + 1
            eps_noise = self.noise((1 << 40) + self._shared["eval_count"])
        x, y, eps_noise = self._inputs(x, y, eps_noise)
        out = torch.zeros_like(self.losses)
        self._kl_plan(None)                             # the target weight: validation curves are comparable across epochs
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_eval(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), N.ptr(eps_noise),
                                                  self.elbo_eps, N.ptr(out), N.stream()), "dvae_train_info_eval")
        return out

    def grads_only(self, x, y, eps_noise, reduce=False):
        """rows + weight-gradient kernels without the optimizer (tests / gradient inspection; read them with grads_numpy()).
        `reduce` is accepted for the signature of Trainer.grads_only: the slabs are summed on reading either way."""
        self._check_inputs(x, y, None, eps_noise)
        self._sync_copies()
        x, y, eps_noise = self._inputs(x, y, eps_noise)
        self._kl_plan(self.step_count + 1)
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), N.ptr(eps_noise),
                                                   self.elbo_eps, N.stream()), "dvae_train_info_grads")

    # ---- accumulate.AccumulatedStep ----
    def _micro(self, flat, accumulate, weight, x, y, eps_noise, rows):
        """One micro-batch: rows + weight-gradient + reduce launches; the slabs go into `flat` (accumulate 0: overwritten) and the
        micro-batch's eight losses into self.losses."""
        self._check_inputs(x, y, rows, eps_noise)
        self._sync_copies()
        x, y, eps_noise = self._inputs(x, y, eps_noise)
        self._kl_plan(self.step_count + 1)              # the weight of the optimizer step this micro-batch ends in
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_grads(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(x), N.ld(x), N.ptr(y), N.ld(y), N.ptr(eps_noise),
                                                   self.elbo_eps, N.stream()), "dvae_train_info_grads")
            N.check(self.lib.dvae_train_info_reduce(ctypes.byref(self.plan), N.ptr(self.ws), N.ptr(flat), int(accumulate), float(weight),
                                                    N.ptr(self.losses), N.stream()), "dvae_train_info_reduce")
        return self.losses

    def _apply_flat(self, flat, grad_scale):
        """One Adam step on g = grad_scale * flat; counts as a step exactly as step() does."""
        self.step_count += 1
        self._shared["version"] += 1
        self._copy_version = self._shared["version"]          # the apply kernel rewrites every element of this trainer's packed copies
        with torch.cuda.device(self.device):
            N.check(self.lib.dvae_train_info_apply_flat(ctypes.byref(self.plan), N.ptr(self._params), N.ptr(self._m), N.ptr(self._v),
                                                        N.ptr(self.ws), N.ptr(flat), self.step_count, self.lr, self.betas[0], self.betas[1],
                                                        self.adam_eps, float(grad_scale), N.stream()), "dvae_train_info_apply_flat")

    def _apply_flat_clipped(self, flat, grad_scale, max_norm):
        """_apply_flat with the global norm of grad_scale * flat clipped to max_norm on the device (clip.py)."""
        clip.apply_flat_clipped(self, "info", flat, grad_scale, max_norm)

    grad_norm = property(lambda self: clip.state(self)["grad_norm"],
                         doc="Device float32 [total_norm, coef] of the last clipped step of this trainer or a fork (no host sync).")

    def skipped_step_count(self):
        """Clipped steps the device skipped for a non-finite gradient since the last call (synchronises; shared with forks).  A skipped
        step leaves parameters, moments and packed copies untouched but still counts in step_count."""
        return clip.skipped_step_count(self)

    def accumulate_losses(self, buf):
        """Running sums for epoch logging without a host sync per step: `buf` is a float64 CUDA tensor of 8 elements (or None to stop);
        every step() / evaluate() adds its loss scalars to its first seven on the device."""
        if buf is not None and not (buf.is_cuda and buf.dtype == torch.float64 and buf.numel() >= 8 and buf.is_contiguous()):
            raise ValueError("accumulate_losses: need a contiguous float64 CUDA tensor with >= 8 elements")
        self._accum = buf
        self.plan.loss_accum = 0 if buf is None else buf.data_ptr()


STD_NORM_REFUSAL = ("std_norm exists on the generic M1 / M2 step only (trainer_generic.GenericTrainer): the M2_info step's classifier and encoder "
                    "read one x tile, and the reference's M2_info script loads the statistics without using them; " + LIMITS)


def info_trainer_kind(dims, dec_label="truth", aux_enc="bce", kl_weight=None, kl_warmup=None, kl_floor=None):
    """Which fused train step serves M2_info at `dims`: "resident" (the hand-tuned kernels of the reference's geometry,
    trainer.supported), "generic" (csrc/train_info.hip) or None.  The resident step has the default options only, so any other
    -- a weighted KL term included (kl_weight / kl_warmup / kl_floor other than 1 / 0 / 0) -- goes to the generic step at the
    reference geometry too.  Host logic only."""
    default = mode_bits(dec_label, aux_enc) == 0 and KL.is_default(kl_weight, kl_warmup, kl_floor)
    try:
        if default and supported("M2_info", dims):
            return "resident"
    except (KeyError, TypeError):       # a dims dict without one of the keys names no geometry of the resident step
        pass
    return "generic" if covered(dims) else None


def make_info_trainer(dims, generic=False, dec_label="truth", aux_enc="bce", std_norm=None, kl_weight=None, kl_warmup=None, kl_floor=None,
                      **kw):
    """The resident Trainer("M2_info", ...) where trainer.supported holds (the default there: the faster step, the 16-bit operand policies,
    data-parallel training), otherwise an InfoTrainer; generic=True, an option other than dec_label="truth" / aux_enc="bce", or a
    weighted KL term (kl_weight / kl_warmup / kl_floor other than 1 / 0 / 0: kl_weight.py) puts the reference geometry on the generic
    step too.  Raises with the limits named when neither covers `dims`, and for a 16-bit policy or
    world != 1 on the generic step; ValueError naming the choices for an unknown option, before anything touches the device."""
    if std_norm is not None:
        raise NotImplementedError(STD_NORM_REFUSAL)
    if not KL.is_default(kl_weight, kl_warmup, kl_floor):
        kw.update(zip(("kl_weight", "kl_warmup", "kl_floor"), KL.check_options(1.0 if kl_weight is None else kl_weight, kl_warmup or 0,
                                                                                kl_floor or 0.0, "make_info_trainer")))
    kind = info_trainer_kind(dims, dec_label, aux_enc, kl_weight, kl_warmup, kl_floor)
    if kind is None or (generic and not covered(dims)):
        raise NotImplementedError(f"no fused M2_info train step for {dims}: the resident step covers x 513, z 16, h [128, 128], y 1; {LIMITS}")
    if kind == "resident" and not generic:
        return Trainer("M2_info", dims, **kw)
    if kw.get("precision", "fp32") != "fp32":
        raise NotImplementedError(f"precision {kw['precision']!r} exists on the resident step only; {LIMITS}")
    if int(kw.get("world", 1)) != 1 or kw.get("process_group") is not None:
        raise NotImplementedError(f"data-parallel training is not built on the generic step (got world={kw.get('world', 1)}); {LIMITS}: wrap a "
                                  "one-GPU trainer per rank in accumulate.AccumulatedStep(trainer, process_group)")
    for k in ("precision", "world", "process_group"):
        kw.pop(k, None)
    return InfoTrainer(dims, dec_label=dec_label, aux_enc=aux_enc, **kw)

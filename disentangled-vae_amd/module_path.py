"""Whole-model autograd path of the drop-in modules.

`packages.models.models.VariationalAutoencoder.forward` / `DeepGenerativeModel.forward` on CUDA tensors at the reference
geometry (x 513, h [128, 128], z 16, y 0 / 1 / 513) run as ONE autograd Function instead of one Function per nn.Linear, and so
does the VAE body of M2_info -- `DeepGenerativeModel_v3.forward` / `DeepGenerativeModel_v5.forward` (encoder on x alone, decoder on
[z | y], y 1; "M2_DEC"): the script's `model(x, y)` call (scripts/training_M2_info_vad.py:161) with z an output that the
auxiliary classifier's loss differentiates through.  Its classifier / auxiliary MLP calls stay per-layer Functions:

    forward : dvae_module_forward  = weight-copy refresh + the 8-wave rows kernel in forward mode   (2 launches)
    backward: dvae_module_backward = rows kernel in backward mode (forward recomputed on chip, then the backward from the
              upstream gradients of r, z, mu, log_var) + weight-gradient kernel + slab sum             (3 launches)

The training scripts keep `loss.backward()` and their own stock `torch.optim.Adam` (scripts/training_M2.py:122, 142-147).
To make that cheap the engine keeps the module's 14 parameters as views of ONE flat fp32 buffer in the fused kernels'
plan layout (they stay ordinary nn.Parameters: state_dict, load_state_dict, optimizers see nothing new).  The Function's
backward RETURNS the 14 parameter gradients -- views of one flat buffer allocated per backward pass -- so everything
autograd does with a gradient stays autograd's: AccumulateGrad takes the views as `.grad` without a copy when there is
none yet (the scripts' zero_grad() sets them to None every step) and adds otherwise, tensor hooks and post-accumulate
hooks run, `torch.autograd.grad(loss, params)` works.  The forward is recomputed on chip in the backward from the CURRENT
parameters, so a parameter changed in place between forward and backward raises, like autograd's version check does.

Only grad-mode forwards take this path: inference (no_grad, or every parameter frozen -- scripts/reconstruct_M2.py:111-113)
runs the per-layer Functions of ops.py on the exact fp32 matrix cores, like direct `model.encoder(...)` /
`model.decoder(...)` calls (packages/models/mcem.py) do, so the two agree to fp32 rounding and no per-batch-size
workspace is ever built for a forward-only call.  DVAE_MODULE_PATH=layers takes the per-layer path everywhere.

MFMA operand policy: DVAE_MODULE_PRECISION (default bf16x3, the parity-grade split-bf16 policy; bf16 = fast and loose).

Any other covered size (opt-in).  An M1 / M2 module of another geometry -- `h_dim = [256, 64]`, `z_dim = 32` edited into the script --
takes one Function per nn.Linear by default, as it always did.  With the switch on it runs as ONE Function as well, on
`GenericModuleEngine`: the generic rows kernel (csrc/train_generic.hip) in its two module modes,

    forward : dvae_module_generic_forward  = packed-copy refresh + rows kernel, forward chain with the outputs written   (2 launches)
    backward: dvae_module_generic_backward = rows kernel (forward recomputed, backward from the upstream gradients)
              + weight-gradient kernel + reduce into one flat gradient                                               (3 launches)

within `trainer_generic.covered`: M1 / M2, x 513, y 0..513, two hidden widths 1..512, z 1..128, no flow.  Any loss written in torch on
(r, z, mu, log_var) -- a weighted or warmed-up KL term, free bits (the fused steps take those too, per element: kl_weight.py; the
batch-mean form lives here), a regulariser on z -- becomes the upstream gradients of that one
backward.  The switch:
    DVAE_MODULE_GENERIC unset / 0   off: every call keeps the path and the bits it had
    DVAE_MODULE_GENERIC=1           on for the sizes the resident engine does not serve
    DVAE_MODULE_GENERIC=force       on, and the reference geometry goes through the generic engine too (tests, A/B runs)
    set_generic(module, mode)       the same per module (None: follow the environment); engine_kind(module, model) tells the outcome
DVAE_MODULE_PRECISION does not apply there: the generic path is exact fp32 (the f32 MFMA), whatever it says.  The rules above hold
unchanged: inference stays on the per-layer kernels, DVAE_MODULE_PATH=layers wins.  Whether the generic engine should be the default is
left to the measurement in DESIGN 4b.

The M2_info body of any covered size (opt-in, a switch of its own).  `DeepGenerativeModel_v3` / `_v5` ("M2_DEC": encoder on x alone, decoder
on [z | y]) with an edited geometry, or with IBM labels (y 513) at the reference widths, runs per layer by default as well.  With
    DVAE_MODULE_INFO_BODY unset / 0 / off   as ever: the resident engine at 128 / 128 / 16 / y 1, per-layer elsewhere
    DVAE_MODULE_INFO_BODY=1 / on            resident where it serves, else the generic engine on a plan of dvae_module_generic_plan: two hidden
                                            layers, x 513, y 1..513, h 1..512, z 1..128, biases, no flow
    DVAE_MODULE_INFO_BODY=force             the generic engine wherever covered (tests, A/B runs)
    set_info_body(module, mode)             the same per module, on a _v3 or a _v5 (forwarded to its enc_dec_clf); None: the environment
the body is ONE Function on the DEC variant of the generic rows kernel's module modes.  DVAE_MODULE_GENERIC says nothing about this body,
and this switch nothing about M1 / M2.  On the generic engine of this body -- and there only -- the label input may carry a gradient:
`model(x, classifier(x))` of scripts/training_M2_info_vad_pretrain.py:162-163 stays on the fused path, and the Function's backward returns
d loss / d y = dpre_d1 D1[:, z:] in the slot of y (dvae_module_generic_backward_y: computed beside dz in the rows kernel, no further
launch).  A gradient with respect to x, and with respect to y on M2 or on the resident engine, stays a layer-path feature.
"""
import ctypes
import os

import torch

from . import native as N
from . import trainer_generic as TG
from .trainer import MODEL_CODE, PREC_CODE, TENSOR_NAMES, TrainPlan


def enabled():
    return os.environ.get("DVAE_MODULE_PATH", "fused") != "layers"


def _precision():
    p = os.environ.get("DVAE_MODULE_PRECISION", "bf16x3")
    if p not in ("bf16x3", "bf16"):
        raise ValueError("DVAE_MODULE_PRECISION must be bf16x3 or bf16 (the fused module path has no fp32-MFMA kernel; use DVAE_MODULE_PATH=layers)")
    return p


def vae_parameters(module, model):
    """The 14 (name, parameter) pairs of the VAE in plan order.  M2_DEC (a _v3 module): encoder + decoder, not the classifier."""
    if model == "M2_DEC":
        return list(module.encoder.named_parameters(prefix="encoder")) + list(module.decoder.named_parameters(prefix="decoder"))
    return list(module.named_parameters())


class ModuleEngine:
    """Fused kernels bound to one module instance (M1, M2, or the encoder + decoder of a _v3: M2_DEC)."""

    kind = "resident"

    def __init__(self, module, model, y_dim):
        self.precision = _precision()
        self.z_dim = 16
        self._bind(module, model, y_dim)

    def _bind(self, module, model, y_dim):
        self.lib = N.load()
        self.model, self.y_dim = model, int(y_dim)
        named = vae_parameters(module, model)
        sd_names = [n for n, _ in named]
        if sd_names != TENSOR_NAMES:
            raise RuntimeError(f"unexpected parameter set for the fused module path: {sd_names}")
        self.params = [p for _, p in named]
        # where the module keeps each of them (submodule._parameters[name]): `current()` checks the 14 slots instead of walking
        # named_parameters() on every forward (35 us of a 400 us step at the scripts' batch size)
        mods = dict(module.named_modules())
        self.slots = []
        for n, _ in named:
            owner, _, leaf = n.rpartition(".")
            self.slots.append((mods[owner]._parameters, leaf))
        self.device = self.params[0].device
        self.plans = {}
        p0 = self._plan(128)[0]
        self.n_params = int(p0.n_params)
        self.spans = [(int(p0.tensor_offset[i]), int(p0.tensor_rows[i]) * int(p0.tensor_cols[i])) for i in range(len(self.params))]
        with torch.cuda.device(self.device):
            self.flat = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.pptrs = [self.flat.data_ptr() + 4 * o for o, _ in self.spans]
        self._alias()

    def __deepcopy__(self, memo):          # a copied module rebuilds its own engine on first use
        return None

    # ---- plans (one per batch size; each holds a training workspace: stash, gradient slabs, weight copies).  At most
    # MAX_PLANS are kept, least recently used first out (a training loop sees its batch size and the last, shorter batch)
    MAX_PLANS = 4

    def _plan(self, B):
        got = self.plans.pop(B, None)
        if got is not None:
            self.plans[B] = got                    # most recently used last
        if got is None:
            while len(self.plans) >= self.MAX_PLANS:
                self.plans.pop(next(iter(self.plans)))
            plan = TrainPlan()
            N.check(self.lib.dvae_train_plan(MODEL_CODE[self.model], self.y_dim, PREC_CODE[self.precision], int(B), 0, ctypes.byref(plan)),
                    "dvae_train_plan")
            if plan.rows_kernel != 2:
                raise RuntimeError("fused module path needs the 8-wave rows kernel (unset DVAE_ROWS)")
            ws = None
            got = [plan, ws, False]
            self.plans[B] = got
        return got

    def _ready(self, B):
        ent = self._plan(B)
        if not ent[2]:
            with torch.cuda.device(self.device):
                ent[1] = torch.empty(ent[0].workspace_bytes, dtype=torch.uint8, device=self.device)
                N.check(self.lib.dvae_train_init(ctypes.byref(ent[0]), N.ptr(self.flat), N.ptr(ent[1]), N.stream()), "dvae_train_init")
            ent[2] = True
        return ent[0], ent[1]

    # ---- parameters as views of the flat buffer ----
    def _alias(self):
        for p, (o, n), want in zip(self.params, self.spans, self.pptrs):
            if p.data_ptr() != want:
                view = self.flat[o:o + n].view(p.shape)
                with torch.no_grad():
                    view.copy_(p.detach().to(device=self.device, dtype=torch.float32))
                p.data = view

    def usable(self, x):
        return all(p.is_cuda and p.device == x.device and p.dtype == torch.float32 for p in self.params)

    def current(self):
        """The module still holds the parameter objects this engine was built on (a replaced nn.Parameter rebuilds the engine)."""
        for (d, leaf), p in zip(self.slots, self.params):
            if d.get(leaf) is not p:
                return False
        return True

    # ---- launches ----
    def forward(self, x, y, eps):
        B = x.shape[0]
        if self.params[0].device != self.device:
            raise RuntimeError("module moved to another device after the fused engine was built")
        self._alias()
        plan, ws = self._ready(B)
        with torch.cuda.device(self.device):
            r = torch.empty((B, 513), dtype=torch.float32, device=self.device)
            mlz = torch.empty((3, B, 16), dtype=torch.float32, device=self.device)
            yp, ldy = (N.ptr(y), N.ld(y)) if self.y_dim else (None, 0)
            m0 = mlz.data_ptr()                      # mu | log_var | z, [B, 16] fp32 each
            N.check(self.lib.dvae_module_forward(ctypes.byref(plan), N.ptr(self.flat), N.ptr(ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps),
                                                 N.ptr(r), 513, m0, m0 + 64 * B, m0 + 128 * B, 1, N.stream()), "dvae_module_forward")
        mu, lv, z = mlz.unbind(0)
        return r, z, mu, lv

    def backward(self, x, y, eps, gr, gz, gmu, glv, needs):
        """-> list of 14 parameter gradients (None where `needs` is False): views of one flat buffer of this call."""
        B = x.shape[0]
        plan, ws = self._ready(B)
        f32c = lambda t: None if t is None else _rows_ok(t.to(torch.float32))
        gr_, gz, gmu, glv = f32c(gr), f32c(gz), f32c(gmu), f32c(glv)
        if gz is not None: gz = gz.contiguous()
        if gmu is not None: gmu = gmu.contiguous()
        if glv is not None: glv = glv.contiguous()
        with torch.cuda.device(self.device):
            dst = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
            yp, ldy = (N.ptr(y), N.ld(y)) if self.y_dim else (None, 0)
            N.check(self.lib.dvae_module_backward(ctypes.byref(plan), N.ptr(self.flat), N.ptr(ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps),
                                                  N.ptr(gr_), 0 if gr_ is None else N.ld(gr_), N.ptr(gmu), N.ptr(glv), N.ptr(gz),
                                                  N.ptr(dst), 0, N.stream()), "dvae_module_backward")
        # one view op per gradient (as_strided on the flat buffer: contiguous [out, in] / [out] at the tensor's offset)
        return [dst.as_strided(shp, std, o) if need else None for (shp, std, o), need in zip(self._grad_views(), needs)]

    def _grad_views(self):
        gv = self.__dict__.get("_gv")
        if gv is None:
            gv = self._gv = [(tuple(p.shape), (p.shape[1], 1) if p.dim() == 2 else (1,), o) for p, (o, n) in zip(self.params, self.spans)]
        return gv


def _rows_ok(t):
    """A [B, C] operand the kernels can address: unit column stride and a row stride that covers the row (an expanded /
    broadcast tensor -- the gradient of r.sum(0), an expanded input row -- has stride 0 and is materialised)."""
    if t.dim() != 2 or (t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


class GenericModuleEngine(ModuleEngine):
    """The same surface on the generic kernels (module docstring): an M1 / M2 module of any covered size, exact fp32.  The 14 parameters
    are views of one flat buffer in the generic plan's tensor_offset layout; a plan per batch size holds its workspace (packed copies,
    stash, slabs)."""
    kind = "generic"

    def __init__(self, module, model, dims):
        self.precision = "fp32"
        self.dims = dict(dims)
        self.z_dim = int(dims["z_dim"])
        self._bind(module, model, dims.get("y_dim", 0) if model != "M1" else 0)

    def _plan(self, B):
        got = self.plans.pop(B, None)
        if got is None:
            while len(self.plans) >= self.MAX_PLANS:
                self.plans.pop(next(iter(self.plans)))
            got = [TG.make_plan(self.model, self.dims, B) if self.model != "M2_DEC" else make_body_plan(self.dims, B), None, False]
        self.plans[B] = got                        # most recently used last
        return got

    def _ready(self, B):
        ent = self._plan(B)
        if not ent[2]:
            with torch.cuda.device(self.device):
                ent[1] = torch.empty(ent[0].workspace_bytes, dtype=torch.uint8, device=self.device)
                N.check(self.lib.dvae_train_generic_init(ctypes.byref(ent[0]), N.ptr(self.flat), N.ptr(ent[1]), N.stream()), "dvae_train_generic_init")
            ent[2] = True
        return ent[0], ent[1]

    def forward(self, x, y, eps):
        B, Z = x.shape[0], self.z_dim
        if self.params[0].device != self.device:
            raise RuntimeError("module moved to another device after the fused engine was built")
        self._alias()
        plan, ws = self._ready(B)
        with torch.cuda.device(self.device):
            r = torch.empty((B, 513), dtype=torch.float32, device=self.device)
            mlz = torch.empty((3, B, Z), dtype=torch.float32, device=self.device)
            yp, ldy = (N.ptr(y), N.ld(y)) if self.y_dim else (None, 0)
            m0 = mlz.data_ptr()                      # mu | log_var | z, [B, z_dim] fp32 each
            N.check(self.lib.dvae_module_generic_forward(ctypes.byref(plan), N.ptr(self.flat), N.ptr(ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps),
                                                         N.ptr(r), 513, m0, m0 + 4 * B * Z, m0 + 8 * B * Z, 1, N.stream()),
                    "dvae_module_generic_forward")
        mu, lv, z = mlz.unbind(0)
        return r, z, mu, lv

    def backward(self, x, y, eps, gr, gz, gmu, glv, needs, need_y=False):
        """-> list of 14 parameter gradients (None where `needs` is False): views of one flat buffer of this call.  need_y (the M2_DEC
        body only): the list and the label gradient, a fresh [B, y] tensor."""
        B = x.shape[0]
        plan, ws = self._ready(B)
        f32c = lambda t: None if t is None else _rows_ok(t.to(torch.float32))
        gr_ = f32c(gr)
        gz, gmu, glv = (None if t is None else t.to(torch.float32).contiguous() for t in (gz, gmu, glv))
        with torch.cuda.device(self.device):
            dst = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
            yp, ldy = (N.ptr(y), N.ld(y)) if self.y_dim else (None, 0)
            head = (ctypes.byref(plan), N.ptr(self.flat), N.ptr(ws), N.ptr(x), N.ld(x), yp, ldy, N.ptr(eps), N.ptr(gr_),
                    0 if gr_ is None else N.ld(gr_), N.ptr(gmu), N.ptr(glv), N.ptr(gz), N.ptr(dst), 0)
            if need_y:
                gy = torch.empty((B, self.y_dim), dtype=torch.float32, device=self.device)
                N.check(self.lib.dvae_module_generic_backward_y(*head, N.ptr(gy), self.y_dim, N.stream()), "dvae_module_generic_backward_y")
            else:
                N.check(self.lib.dvae_module_generic_backward(*head, N.stream()), "dvae_module_generic_backward")
        grads = [dst.as_strided(shp, std, o) if need else None for (shp, std, o), need in zip(self._grad_views(), needs)]
        return (grads, gy) if need_y else grads


class VaeFunction(torch.autograd.Function):
    """(r, z, mu, log_var) = model(x, y) with reparametrisation noise eps; the parameters are inputs of the Function and
    backward returns their gradients (module docstring)."""

    @staticmethod
    def forward(ctx, engine, x, y, eps, *params):
        r, z, mu, lv = engine.forward(x, y, eps)
        ctx.engine = engine
        ctx.has_y = y is not None
        ctx.versions = [p._version for p in params]
        ctx.save_for_backward(x, y if y is not None else x.new_empty(0), eps)
        ctx.set_materialize_grads(False)
        return r, z, mu, lv

    @staticmethod
    def backward(ctx, gr, gz, gmu, glv):
        x, y, eps = ctx.saved_tensors
        eng = ctx.engine
        # the backward kernel recomputes the forward from the flat parameter buffer as it is NOW
        for p, v0, name in zip(eng.params, ctx.versions, TENSOR_NAMES):
            if p._version != v0:
                raise RuntimeError(f"one of the variables needed for gradient computation has been modified by an inplace operation: parameter "
                                   f"'{name}' is at version {p._version}, the forward saw version {v0} (an optimizer step or load_state_dict "
                                   f"between forward and backward); run the forward again")
        if any(p.data_ptr() != want for p, want in zip(eng.params, eng.pptrs)):
            raise RuntimeError("a parameter's storage was replaced between forward and backward (module.to() / .data assignment): run the forward again")
        if ctx.has_y and ctx.needs_input_grad[2]:       # engine_for lets a label input with a gradient through to the generic M2_DEC engine alone
            grads, gy = eng.backward(x, y, eps, gr, gz, gmu, glv, ctx.needs_input_grad[4:], need_y=True)
            return (None, None, gy, None, *grads)
        grads = eng.backward(x, y if ctx.has_y else None, eps, gr, gz, gmu, glv, ctx.needs_input_grad[4:])
        return (None, None, None, None, *grads)


GENERIC_MODES = {"": "off", "0": "off", "off": "off", "1": "on", "on": "on", "force": "force"}


def generic_mode(module=None):
    """"off" | "on" | "force": the module's own setting (set_generic) or else DVAE_MODULE_GENERIC (module docstring)."""
    m = module.__dict__.get("_dvae_generic") if module is not None else None
    if m is None:
        m = os.environ.get("DVAE_MODULE_GENERIC", "0")
    try:
        return GENERIC_MODES[str(m).lower()]
    except KeyError:
        raise ValueError(f"DVAE_MODULE_GENERIC / set_generic: {m!r} (0 / off, 1 / on, force)") from None


def set_generic(module, mode):
    """The switch of the generic engine for this module alone: "off" / 0, "on" / 1, "force", or None to follow DVAE_MODULE_GENERIC again.
    Takes effect at the next forward (an engine of the other kind is rebuilt on the same parameters)."""
    if mode is not None:
        mode = "on" if mode is True else "off" if mode is False else str(mode).lower()
        if mode not in GENERIC_MODES:
            raise ValueError(f"set_generic: mode {mode!r} (0 / off, 1 / on, force, or None)")
    object.__setattr__(module, "_dvae_generic", mode)


def info_body_mode(module=None):
    """"off" | "on" | "force": the module's own setting (set_info_body) or else DVAE_MODULE_INFO_BODY (module docstring)."""
    m = module.__dict__.get("_dvae_info_body") if module is not None else None
    if m is None:
        m = os.environ.get("DVAE_MODULE_INFO_BODY", "0")
    try:
        return GENERIC_MODES[str(m).lower()]
    except KeyError:
        raise ValueError(f"DVAE_MODULE_INFO_BODY / set_info_body: {m!r} (0 / off, 1 / on, force)") from None


def set_info_body(module, mode):
    """The switch of the generic engine for the M2_info body of this module alone -- a DeepGenerativeModel_v3, or a _v5 (forwarded to its
    enc_dec_clf): "off" / 0, "on" / 1, "force", or None to follow DVAE_MODULE_INFO_BODY again.  Takes effect at the next forward."""
    if mode is not None:
        mode = "on" if mode is True else "off" if mode is False else str(mode).lower()
        if mode not in GENERIC_MODES:
            raise ValueError(f"set_info_body: mode {mode!r} (0 / off, 1 / on, force, or None)")
    body = module.__dict__.get("_modules", {}).get("enc_dec_clf", module)
    object.__setattr__(body, "_dvae_info_body", mode)


def _mode_of(module, model):
    """the switch that speaks for this model: DVAE_MODULE_INFO_BODY for the M2_info body, DVAE_MODULE_GENERIC for M1 / M2"""
    return info_body_mode(module) if model == "M2_DEC" else generic_mode(module)


def make_body_plan(dims, batch, ksplit=0):
    """dvae_module_generic_plan for the M2_DEC body (dims, batch): host only.  Raises NotImplementedError / ValueError with the library's message."""
    lib = N.load()
    h = tuple(dims["h_dim"])
    if dims.get("x_dim") != 513 or len(h) != 2:
        raise NotImplementedError(f"the generic module engine covers x_dim 513 and two hidden widths; got M2_DEC {dims}")
    plan = TG.GenericPlan()
    rc = lib.dvae_module_generic_plan(MODEL_CODE["M2_DEC"], int(dims["y_dim"]), int(dims["z_dim"]), int(h[0]), int(h[1]), int(batch), int(ksplit),
                                      ctypes.byref(plan))
    if rc != 0:
        msg = lib.dvae_last_error().decode("utf-8", "replace")
        raise (NotImplementedError if rc == 1003 else ValueError)(f"{msg} (got M2_DEC {dims})")
    return plan


def body_covered(dims):
    """The geometry limits of the M2_DEC body on the generic engine (host logic only)."""
    h = tuple(dims.get("h_dim", ()))
    return (dims.get("x_dim") == 513 and len(h) == 2 and all(1 <= int(v) <= 512 for v in h) and 1 <= int(dims.get("z_dim", 0)) <= 128
            and 1 <= int(dims.get("y_dim", 0) or 0) <= 513)


def _resident_geometry(module, model):
    return (module.z_dim == 16 and module.flow is None
            and [tuple(l.weight.shape) for l in module.encoder.hidden] == [(128, 513 + (module.y_dim if model == "M2" else 0)), (128, 128)]
            and [tuple(l.weight.shape) for l in module.decoder.hidden] == [(128, 16 + (module.y_dim if model != "M1" else 0)), (128, 128)]
            and tuple(module.decoder.reconstruction.weight.shape) == (513, 128)
            and (model == "M1" or module.y_dim in ((1, 513) if model == "M2" else (1,))))


def generic_dims(module, model):
    """dims of an M1 / M2 module, or of the M2_DEC body of a _v3, the generic engine covers (trainer_generic.covered / body_covered and every
    layer of the plan's shape), else None.  Host logic only."""
    if model not in ("M1", "M2", "M2_DEC") or module.flow is not None:
        return None
    enc, dec = list(module.encoder.hidden), list(module.decoder.hidden)
    if len(enc) != 2 or len(dec) != 2 or not all(isinstance(l, torch.nn.Linear) and l.bias is not None for l in enc + dec):
        return None
    y = int(module.y_dim) if model != "M1" else 0
    ye = y if model == "M2" else 0                   # the label columns of encoder layer 1
    z, h1, h2 = int(module.z_dim), enc[0].out_features, enc[1].out_features
    dims = dict(x_dim=enc[0].in_features - ye, y_dim=y, z_dim=z, h_dim=(h1, h2))
    sample, rec = module.encoder.sample, module.decoder.reconstruction
    shapes = [tuple(l.weight.shape) for l in (enc[0], enc[1], getattr(sample, "mu", rec), getattr(sample, "log_var", rec), dec[0], dec[1], rec)]
    ok = body_covered(dims) if model == "M2_DEC" else TG.covered(model, dims)
    if not ok or shapes != [(h1, 513 + ye), (h2, h1), (z, h2), (z, h2), (h2, z + y), (h1, h2), (513, h1)]:
        return None
    return dims


def engine_kind(module, model):
    """"resident", "generic" or None: the engine a grad-mode forward of this module on CUDA float32 tensors would take as the switches
    stand (DVAE_MODULE_PATH; DVAE_MODULE_GENERIC / set_generic for M1 / M2; DVAE_MODULE_INFO_BODY / set_info_body, and that switch only,
    for the M2_DEC body).  Host logic only: nothing is built and no device is touched."""
    if not enabled():
        return None
    mode = _mode_of(module, model)
    dims = generic_dims(module, model) if mode != "off" else None
    if _resident_geometry(module, model) and not (mode == "force" and dims is not None):
        return "resident"
    return "generic" if dims is not None else None


def engine_for(module, model, x, y):
    """The module's engine when this call can take the fused path, else None.  model: "M1" | "M2" | "M2_DEC" (module: a _v3)."""
    if not (enabled() and x.is_cuda and x.dim() == 2 and x.shape[1] == 513 and x.dtype == torch.float32 and x.shape[0] > 0):
        return None
    y_grad = y is not None and y.requires_grad
    if x.requires_grad or (y_grad and model != "M2_DEC"):
        return None                                  # gradients with respect to the data are a layer-path feature (but see y_grad below)
    if not torch.is_grad_enabled():
        return None                                  # inference: the exact-fp32 per-layer kernels (module docstring)
    mode = _mode_of(module, model)
    eng = module.__dict__.get("_dvae_engine")
    if eng is not None and not (eng.current() and eng.mode == mode):
        eng = None                                   # a parameter object was replaced, or the switch moved: a new engine on the set
        module.__dict__.pop("_dvae_engine", None)
    if not any(p.requires_grad for p in (eng.params if eng is not None else [p for _, p in vae_parameters(module, model)])):
        return None                                  # every parameter frozen: inference as well
    if eng is None:
        if module.__dict__.get("_dvae_engine_off") == mode:
            return None
        kind = engine_kind(module, model)
        ok = (kind is not None and all(p.is_cuda and p.dtype == torch.float32 for _, p in vae_parameters(module, model))
              and [n for n, _ in vae_parameters(module, model)] == TENSOR_NAMES)
        if not ok:
            object.__setattr__(module, "_dvae_engine_off", mode)
            return None
        if kind == "generic":
            eng = GenericModuleEngine(module, model, generic_dims(module, model))
        else:
            eng = ModuleEngine(module, model, module.y_dim if model != "M1" else 0)
        eng.mode = mode
        object.__setattr__(module, "_dvae_engine", eng)
    if not eng.usable(x):
        return None
    if y_grad and eng.kind != "generic":
        return None                                  # the label gradient exists on the generic engine of the M2_DEC body alone
    if model != "M1" and (y is None or y.dim() != 2 or y.shape != (x.shape[0], eng.y_dim) or y.dtype != torch.float32 or y.device != x.device):
        return None
    return eng


def run(eng, x, y, eps):
    """-> (r, z, mu, log_var).  eps: [B, z_dim] float32 on x's device (z_dim 16 on the resident engine)."""
    x = _rows_ok(x)
    if y is not None:
        y = _rows_ok(y)
    eps = eps.to(device=x.device, dtype=torch.float32).contiguous()
    if eps.shape != (x.shape[0], eng.z_dim):
        raise RuntimeError(f"reparametrisation noise must be [{x.shape[0]}, {eng.z_dim}], got {tuple(eps.shape)}")
    return VaeFunction.apply(eng, x, y, eps, *eng.params)

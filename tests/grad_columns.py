"""Weight gradients of the fused train step PER INPUT COLUMN against float64: the statistic, the CPU restatements of the operand
policies, the bound and the inputs (numpy only; tests/test_grad_columns_cpu.py and tests/test_gpu_fused_columns.py use it).

Why per column.  Every other gradient check measures a tensor against its own largest element.  The columns of encoder layer 1's weight
are input features whose scales differ by orders of magnitude (power-spectrum bins against each other, 0/1 labels against spectra up to
1e4), so a column that is wrong by 1 % -- or never written -- moves that figure by 1e-5 or less.  Adam normalises every element by its own
history: each column matters at its own scale.

Statistic.  For g[out, in] and its float64 truth G: c_k = max_n |g[n,k] - G[n,k]| / max_n |G[n,k]|; a bias counts as one column.  A column
whose truth is identically zero (a label that is 0 in every frame, a unit that is dead in every frame) must be exactly zero in g and takes
no part in the figures.  Per tensor: the worst column and the median column.

Truth.  oracle/vae_oracle.py in float64; M2_info: g1 + g2 on the auxiliary net (what the second backward accumulates).

Restatements: what a correct implementation of an operand policy deviates by, from the oracle and never from the library.
  float32   the oracle run in float32, in two summation orders: numpy's own, and every reduction through one float32 accumulator in
            k-steps of 8 with the frame sums formed per slab (KStepOrderF32: the order of an MFMA loop and of the slab sums).  Its
            figure is the larger of the two draws.  Added because the device needed it: at ONE frame a column of the mu / log_var
            weight gradient is dmu x h2[k], so its figure IS the relative float32 error of one tanh output, and a unit whose
            pre-activation nearly cancels (bench, M2 y 513, 1 frame: unit 74) takes 4.5e-5 in numpy's order, 9.9e-5 in k-steps and
            3.5e-4 on the device -- three draws of the same sum of 128 float32 products.
  bf16x3    the float64 oracle with every GEMM operand (forward products, dpre.T @ inp, the bias sum's dpre, dpre @ W) rounded to fp32,
            then hi = bf16(v), lo = bf16(v - hi), operand hi + lo; the x block of encoder layer 1 (and of the M2_info classifier's
            layer 1) in the forward as csrc/fused_tiles.hpp (struct X16) has it: x * 2^-3 and W * 2^6 in two fp16 planes each
            (subnormals kept), hi*hi + lo*hi + hi*lo, the sum * 2^-3.
  bf16      the same with bf16(v) alone and no fp16 block.
They enter through the oracle's optional operand hook (vae_oracle.gemm_hook); everything that is not a GEMM operand stays float64 there,
the float32 restatement carries the elementwise arithmetic.

Bound (a rule, not a number), per tensor and precision:
    worst column  <= 4 x (worst column of the float32 restatement + worst column of the policy's restatement)
    median column <= 4 x (median of the float32 restatement      + median of the policy's restatement)
with the second term zero under the fp32 policy.  4 = 2 x 2: two equally valid summation orders or roundings are two draws whose errors
can oppose each other against float64, and the worst of ~1000 columns is a tail statistic of one draw.  The restatements are those of the
very case under test; nothing is taken from a device run.  One floor, from the number format: the float32 term is never taken below
2^-24, the rounding unit of float32.  A one-element tensor (M2_info's output-layer biases at y_dim 1) is one column of one element, both
float32 draws return the float32 NEAREST to the float64 value (9e-9 and 4e-9 off, by luck of where it lies between two floats), and
4 x that would ask a float32 result for 4e-8: less than the format holds.  The device is 5.8e-8 and 1.8e-7 off there, under two ulps.

Inputs.  bench: golden_util.make_batch (params seed 11, batch seed 12).  speech-like (31, 32): bins falling 60 dB across the spectrum,
a per-frame level, see make_speech_batch.  M2_info: the speech-like family / 64 (unscaled the classifier saturates and float32 and
float64 differ by 0.1 ... 0.9 on its tensors), made tie-free as test_fused_m2info_tie_free_batch_vs_oracle does it.
"""
import contextlib
import functools

import numpy as np

import golden_util as gu
from oracle import vae_oracle as vo

XD = 513
MARGIN = 4.0
INFO_WEIGHTS = (0.5, 10.0, 1.0)                      # alpha, beta, gamma of the M2_info cases
L1X = ("encoder.hidden.0", "enc_dec_clf.encoder.hidden.0", "enc_dec_clf.classifier.hidden.0")    # layers whose input starts with x
SEEDS = {"bench": (11, 12), "speech": (31, 32), "info": (31, 32)}
TIE_DELTA = 1e-4


def dims_of(y_dim):
    return dict(x_dim=XD, y_dim=y_dim, z_dim=16, h_dim=(128, 128))


# ---------------------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------------------

def f32(v):
    return np.ascontiguousarray(np.asarray(v, np.float64).astype(np.float32))


def bf16(v32):
    """float32 -> nearest-even bf16, as float32"""
    u = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return r.view(np.float32)


def round_bf16(v):
    return bf16(f32(v)).astype(np.float64)


def split_bf16(v):
    """fp32 first, hi = bf16(v), lo = bf16(v - hi) (the difference is exact in fp32): hi + lo"""
    v32 = f32(v)
    hi = bf16(v32)
    return hi.astype(np.float64) + bf16(v32 - hi).astype(np.float64)


def split_f16(v, scale):
    """the two fp16 planes of fp32(v) * scale (a power of two), subnormals kept, as float64"""
    vs = f32(v) * np.float32(scale)
    hi = vs.astype(np.float16)
    lo = (vs - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


class OperandPolicy:
    """The operand hook of vae_oracle for the 16-bit policies.  planes 2: split bf16 (bf16x3), 1: one bf16.  f16_block: the x block of
    L1X in the forward as struct X16.  wgrad_x is a SEEDED FAULT for the CPU tests: the x operand of the layer-1 weight gradient, from
    column wgrad_x_from on, without its lo plane ("bf16") or rebuilt from the forward's fixed-scale fp16 planes ("f16")."""

    def __init__(self, planes, f16_block, wgrad_x=None, wgrad_x_from=0):
        self.op = split_bf16 if planes == 2 else round_bf16
        self.f16_block, self.wgrad_x, self.wgrad_x_from = f16_block, wgrad_x, wgrad_x_from

    def fwd(self, name, x, W):
        if self.f16_block and name in L1X:
            xh, xl = split_f16(x[:, :XD], 2.0 ** -3)
            wh, wl = split_f16(W[:, :XD], 2.0 ** 6)
            out = (xh @ wh.T + xl @ wh.T + xh @ wl.T) * 2.0 ** -3
            if x.shape[1] > XD:
                out = out + self.op(x[:, XD:]) @ self.op(W[:, XD:]).T
            return out
        return self.op(x) @ self.op(W).T

    def wgrad(self, name, dpre, inp):
        a = self.op(inp)
        if self.wgrad_x is not None and name in L1X:
            k0 = self.wgrad_x_from
            if self.wgrad_x == "bf16":
                a[:, k0:XD] = round_bf16(inp[:, k0:XD])
            else:
                hi, lo = split_f16(inp[:, k0:XD], 2.0 ** -3)
                a[:, k0:XD] = split_bf16((hi + lo) * 8.0)
        return self.op(dpre).T @ a

    def bias(self, name, dpre):
        return self.op(dpre).sum(axis=0)

    def bwd(self, name, dpre, W):
        return self.op(dpre) @ self.op(W)


class KStepOrderF32:
    """The float32 restatement's second summation order (a hook for the oracle run in float32): every reduction goes through ONE float32
    accumulator in steps of 8 terms, in index order, as a loop of MFMA k-steps does (csrc/fused_tiles.hpp: PolF32::KSTEP), and the frame
    sums of the weight and bias gradients are formed per slab of frames (16 slabs of whole 32-frame tiles) and the slabs added at the end,
    as the weight-gradient launch and the optimizer launch do.  numpy's own order (blocked GEMMs, pairwise sums) is the first."""
    STEP, SLABS, TILE = 8, 16, 32

    def _chain(self, a, b):
        """a @ b, the reduction axis in steps of STEP through one float32 accumulator"""
        acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
        for k in range(0, a.shape[1], self.STEP):
            acc = acc + a[:, k:k + self.STEP] @ b[k:k + self.STEP]
        return acc

    def _slabbed(self, dpre, inp):
        B = dpre.shape[0]
        per = -(-(-(-B // self.SLABS)) // self.TILE) * self.TILE
        total = None
        for b0 in range(0, B, per):
            part = self._chain(np.ascontiguousarray(dpre[b0:b0 + per].T), inp[b0:b0 + per])
            total = part if total is None else total + part
        return total

    def fwd(self, name, x, W):
        return self._chain(x, np.ascontiguousarray(W.T))

    def wgrad(self, name, dpre, inp):
        return self._slabbed(dpre, inp)

    def bias(self, name, dpre):
        return self._slabbed(dpre, np.ones((dpre.shape[0], 1), np.float32))[:, 0]

    def bwd(self, name, dpre, W):
        return self._chain(dpre, W)


F32_UNIT = 2.0 ** -24            # rounding unit of float32, the format every gradient is delivered in


POLICIES = {"bf16x3": lambda: OperandPolicy(2, True), "bf16": lambda: OperandPolicy(1, False)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle under a dtype / a hook
# ---------------------------------------------------------------------------------------------------------------------------------

def oracle_grads(model, params, x, y, e, dtype=np.float64, hook=None):
    """Every parameter's gradient (float64 arrays) of one step; M2_info: g1 + g2 on the auxiliary net."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    p = {k: c(v) for k, v in params.items()}
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
        if model == "M2_info":
            a, b, g = INFO_WEIGHTS
            _, g1, g2 = vo.m2info_losses_and_grads(p, c(x), c(y), c(e), a, b, g)
            grads = {k: g1[k] + (g2[k] if k in g2 else 0.0) for k in g1}
        else:
            _, grads = vo.vae_loss_and_grads(model, p, c(x), c(y), c(e))
    return {k: np.asarray(grads[k], np.float64).reshape(params[k].shape) for k in params}


# ---------------------------------------------------------------------------------------------------------------------------------
# statistic and bound
# ---------------------------------------------------------------------------------------------------------------------------------

def column_figures(g, G):
    """dict(worst, median, arg, zero_share, zero_ok, tensor) of g against the truth G; `tensor` is the figure the other tests use:
    max |g - G| / max |G| over the whole tensor."""
    G = np.asarray(G, np.float64)
    g = np.asarray(g, np.float64).reshape(G.shape)
    if G.ndim == 1:
        G, g = G[:, None], g[:, None]
    err, top = np.abs(g - G).max(axis=0), np.abs(G).max(axis=0)
    zero = top == 0
    live = np.flatnonzero(~zero)
    c = err[live] / top[live]
    return dict(worst=float(c.max()) if c.size else 0.0, median=float(np.median(c)) if c.size else 0.0,
                arg=int(live[np.argmax(c)]) if c.size else -1, zero_share=float(zero.mean()), zero_ok=bool(np.all(g[:, zero] == 0)),
                tensor=float(err.max() / (top.max() + 1e-300)))


def bound(fig32, figpol=None):
    """(worst, median) a correct implementation may reach: 4 x (float32 restatement + the policy's restatement).  The float32 term is
    never taken below the rounding unit of float32 (see the module docstring)."""
    w = max(fig32["worst"], F32_UNIT) + (figpol["worst"] if figpol else 0.0)
    m = max(fig32["median"], F32_UNIT) + (figpol["median"] if figpol else 0.0)
    return MARGIN * w, MARGIN * m


def merge_figures(a, b):
    """the figures of a restatement that has two draws: the larger worst column (with its index) and the larger median"""
    top = a if a["worst"] >= b["worst"] else b
    return dict(top, median=max(a["median"], b["median"]), zero_ok=a["zero_ok"] and b["zero_ok"], tensor=max(a["tensor"], b["tensor"]))


def check(grads, ref, precision, label=""):
    """Every tensor of `grads` against ref (a Reference) under `precision`.  Prints one line per tensor, returns the list of failures
    (empty: pass) and the worst ratio to the bound."""
    fails, top = [], 0.0
    for k, G in ref.truth.items():
        f = column_figures(grads[k], G)
        bw, bm = bound(ref.figures["fp32"][k], None if precision == "fp32" else ref.figures[precision][k])
        rw, rm = f["worst"] / (bw + 1e-300), f["median"] / (bm + 1e-300)
        top = max(top, rw, rm)
        print(f"{label} {k:46s} worst {f['worst']:.2e} ({rw:5.2f} of bound) at column {f['arg']:4d}   median {f['median']:.2e} ({rm:5.2f})   "
              f"zero columns {100 * f['zero_share']:.1f} %   tensor-level {f['tensor']:.1e}")
        if not f["zero_ok"]:
            fails.append((k, "a column whose float64 gradient is identically zero is not exactly zero"))
        if not f["worst"] <= bw:
            fails.append((k, f"worst column {f['arg']}: {f['worst']:.3e} > {bw:.3e}"))
        if not f["median"] <= bm:
            fails.append((k, f"median column: {f['median']:.3e} > {bm:.3e}"))
    return fails, top


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------

def make_speech_batch(dims, B, seed, scale=1.0):
    """x[b,k] = clip(10^(-6k/512) exp(1.5 n_b + n1[b,k]) (n2^2 + n3^2) / 2, 1e-12, 1e4) * scale: bins falling 60 dB across the spectrum,
    one level per frame; labels and noise as make_batch draws them."""
    rng = np.random.default_rng(seed)
    xd, yd, zd = dims["x_dim"], dims["y_dim"], dims["z_dim"]
    nb = rng.standard_normal((B, 1))
    n1, n2, n3 = (rng.standard_normal((B, xd)) for _ in range(3))
    x = 10.0 ** (-6.0 * np.arange(xd) / 512.0) * np.exp(1.5 * nb + n1) * (n2 ** 2 + n3 ** 2) / 2
    x = (np.clip(x, 1e-12, 1e4) * scale).astype(np.float32)
    y = None if yd == 0 else (rng.random((B, yd)) < (0.6 if yd == 1 else 0.3)).astype(np.float32)
    return x, y, rng.standard_normal((B, zd)).astype(np.float32)


def relu_margins(params, x, e):
    """float64: per frame, the smallest |pre| / (sum_k |w_k in_k| + |b|) over the hidden units of M2_info's four ReLU layers
    (the measure of test_fused_m2info_tie_free_batch_vs_oracle)."""
    p = {k: v.astype(np.float64) for k, v in params.items()}
    x = x.astype(np.float64)
    enc = vo.encoder_fwd(p, "enc_dec_clf.encoder.", x, e.astype(np.float64))
    worst = np.full(x.shape[0], np.inf)
    for prefix, inp in (("enc_dec_clf.classifier.", x), ("auxiliary.", enc["z"])):
        h = inp
        for name in vo._hidden_names(p, prefix):
            W, b = p[name + ".weight"], p[name + ".bias"]
            pre = h @ W.T + b
            worst = np.minimum(worst, (np.abs(pre) / (np.abs(h) @ np.abs(W).T + np.abs(b) + 1e-300)).min(axis=1))
            h = np.maximum(pre, 0)
    return worst


def make_tie_free(params, x, y, e, delta=TIE_DELTA):
    """Frames with a ReLU margin < delta replaced by frames with margin >= 4 delta (in place); returns (replaced, smallest margin left)."""
    replaced = 0
    for _ in range(4):                                   # a replaced frame brings its own noise, hence its own z: iterate
        worst = relu_margins(params, x, e)
        risky = np.flatnonzero(worst < delta)
        if risky.size == 0:
            break
        safe = np.flatnonzero(worst >= 4 * delta)
        src = safe[(np.arange(risky.size) * 7919) % safe.size]
        x[risky], y[risky], e[risky] = x[src], y[src], e[src]
        replaced += risky.size
    return replaced, float(relu_margins(params, x, e).min())


# ---------------------------------------------------------------------------------------------------------------------------------
# a case: inputs, truth, restatements (computed once, shared by the three precisions)
# ---------------------------------------------------------------------------------------------------------------------------------

class Reference:
    def __init__(self, family, model, y_dim, B):
        self.family, self.model, self.B = family, model, B
        self.dims = dims_of(y_dim)
        ps, bs = SEEDS[family]
        self.params = gu.make_params(model, self.dims, ps)
        if family == "bench":
            self.x, self.y, self.e = gu.make_batch(self.dims, B, bs)
        else:
            self.x, self.y, self.e = make_speech_batch(self.dims, B, bs, 1.0 / 64 if family == "info" else 1.0)
        self.replaced, self.margin = 0, np.inf
        if model == "M2_info":
            self.replaced, self.margin = make_tie_free(self.params, self.x, self.y, self.e)
        self._build()

    @classmethod
    def at(cls, model, y_dim, params, x, y, e):
        """The reference of one step on GIVEN float32 parameters and frames (tests/later_steps.py) in the place of the family's."""
        self = cls.__new__(cls)
        self.family, self.model, self.B, self.dims = "given", model, int(x.shape[0]), dims_of(y_dim)
        self.params, self.x, self.y, self.e = params, x, y, e
        self.replaced, self.margin = 0, np.inf
        self._build()
        return self

    def _build(self):
        model = self.model
        a = (model, self.params, self.x, self.y, self.e)
        self.truth = oracle_grads(*a)
        self.restated = {"fp32": oracle_grads(*a, dtype=np.float32), "fp32 k-steps": oracle_grads(*a, dtype=np.float32, hook=KStepOrderF32())}
        for name, make in POLICIES.items():
            self.restated[name] = oracle_grads(*a, hook=make())
        self.draws = {p: {k: column_figures(g[k], self.truth[k]) for k in self.truth} for p, g in self.restated.items()}
        self.figures = {p: self.draws[p] for p in POLICIES}
        self.figures["fp32"] = {k: merge_figures(self.draws["fp32"][k], self.draws["fp32 k-steps"][k]) for k in self.truth}
        for arr in (self.x, self.y, self.e):
            if arr is not None:
                arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(family, model, y_dim, B):
    return Reference(family, model, y_dim, B)

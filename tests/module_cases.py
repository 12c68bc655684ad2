"""The whole-model module path (disentangled-vae_amd/module_path.py: dvae_module_forward / dvae_module_backward, the 8-wave rows kernel
in its forward-only and upstream-gradient modes) against float64: truth, restatements, statistics, bound and inputs (numpy only;
tests/test_module_oracle_cpu.py and tests/test_gpu_module_oracle.py use it).

Truth.  oracle/vae_oracle.py in float64 on the float32 inputs.  Forward: m1_forward / m2_forward / m2v3_forward (M2_DEC: encoder on x alone,
decoder on [z | y], the VAE body of a _v3 module) -> r, a = log r, mu, log_var, z.  Backward from the upstream gradients (g_r, g_z, g_mu,
g_lv), each possibly None = zero:  da = g_r * r;  dd = decoder_bwd(.., da);  dz = dd[:, :16] + g_z;  encoder_bwd(.., dz, g_mu, g_lv) --
the gradient of sum(r g_r) + sum(z g_z) + sum(mu g_mu) + sum(lv g_lv), pinned against torch.float64 autograd in the CPU test.

Restatements (what a correct implementation may deviate by; from the oracle, never from the library), built as tests/grad_columns.py
builds them and with its classes:
  float32   the same composition in float32, two draws and the larger figure of the two: numpy's order with numpy's tanh and exp, and
            grad_columns.KStepOrderF32 with the two functions as the 16-bit policies compute them (csrc/fused_tiles.hpp, PolBF16; PolX3
            inherits them), in float32: exp(v) = exp2(v * log2 e), tanh(v) = 1 - 2 / (exp2(v * 2 log2 e) + 1).  The rounding of exp2's
            argument moves exp(a) by |a| 2^-24 of itself, where numpy's float32 exp stays within 2^-24: a frame sum of da = g_r * r that
            nearly cancels (a row of the reconstruction bias gradient) feels it.  The second form of tanh leaves an ABSOLUTE error of
            about 2^-24 on an output near zero: at one frame a column of the reconstruction weight gradient is da x d2[k], its figure the
            relative error of that one tanh.
  bf16x3    two draws and the larger figure of the two: float64 under vae_oracle.gemm_hook(OperandPolicy(2, True)), and ThreeProductsF32
            below -- the same split operands multiplied as the kernels multiply them (csrc/fused_tiles.hpp, PolX3: hi*hi + lo*hi +
            hi*lo, no lo*lo) and accumulated in float32 in k-steps of 16 (PolBF16::KSTEP), with the policies' exp and tanh.  The first
            draw rounds operands and then sums exactly; the float32 restatement rounds sums and keeps operands exact; a kernel does
            both to the same numbers.  Where one element stands alone at its own scale the two separate draws are one sample each of
            a heavy-tailed ratio: the first device run had three such figures at 1.6 ... 2.5 of a bound made without the second draw
            -- two elements of the reconstruction bias gradient whose frame sums cancel to 1e-6 of their terms (M2 y 1 at 31 and
            8193 frames; their absolute errors were 0.3 and 2.4 times the median element's), and at ONE frame the column of the
            reconstruction weight gradient that belongs to a decoder unit whose output lies 250 times below the median unit's -- and
            this draw is of the device's size there (7e-4 on that column against the device's 2.4e-3 where the first draw has 1.7e-4;
            0.15 on the 31-frame element against 0.19 where the first has 3.5e-3).
  bf16      float64 under OperandPolicy(1, False).
  One term from the operand format, for the one statistic whose columns are single numbers (the reconstruction bias per row): element
  k is the frame sum of da[:, k], each term an MFMA operand of 16 significant bits under bf16x3 (hi + lo) and 8 under bf16, i.e. rounded
  by up to u = 2^-17 / 2^-9 of itself, so the sum moves by u sqrt(sum_b da[b, k]^2) whatever the order -- relative to a sum that cancels
  to 1e-6 of its terms that is percents, and any ONE draw of it (a restatement's, the device's) is one sample of a centred normal: the
  ratio of two such samples exceeds 4 one time in six.  The policy term of that statistic is therefore never taken below
  u sqrt(sum_b da[b, k]^2) / |G[k]| (worst and median over k, da and G from the float64 truth), as the float32 term is never taken
  below 2^-24.

Statistics.
  mu, log_var, z   max |got - truth| / max |truth| of the tensor.
  r                on log r: max |log got - a| / max(1, max |a|)  (r = exp(a) spans decades; a max-normalised figure on r sees the loudest
                   bins only).
  every gradient   grad_columns.column_figures: per input column at its own scale, worst and median column; a column whose truth is
                   identically zero must be exactly zero.
  decoder.reconstruction.weight / .bias   additionally per OUTPUT ROW, each of the 513 rows at its own scale (entries "<name> rows"): this
                   is what sees bin 512, which one wave computes on its own path.

Bound: grad_columns.bound -- statistic <= 4 x (max(float32 restatement, 2^-24) + policy restatement) of the very case under test, each
restatement the larger of its draws (and, for the per-row bias statistic, the operand-format term above).  Under
bf16 a tensor whose bound comes out above 0.3 takes the stated bf16 bar of test_fused_step_vs_oracle instead: within 0.3 of the maximum
and cosine >= 0.99 with the truth.

Inputs.  Parameters golden_util.make_params(model, dims, 11), batch golden_util.make_batch(dims, B, 12).  Upstream gradients from
default_rng(13): g_r = N(0, 1) * s_k / B with per-column scales s_k = exp(U(-6, 0)) (bin 512 and its neighbours each at a scale of their
own), g_z, g_mu, g_lv = N(0, 1) / B.
"""
import contextlib
import functools

import numpy as np

import golden_util as gu
import grad_columns as gc
from oracle import vae_oracle as vo

XD, ZD = gc.XD, 16
PARAM_SEED, BATCH_SEED, UPSTREAM_SEED = 11, 12, 13
MODELS = [("M1", 0), ("M2", 1), ("M2", 513), ("M2_DEC", 1)]
# which upstream gradients are given (the others are None: a null pointer at the kernel)
UPSTREAMS = {"all": ("r", "z", "mu", "lv"), "r": ("r",), "z": ("z",), "mu": ("mu",), "lv": ("lv",), "mu+lv": ("mu", "lv")}
FULL_CROSS_AT = (33, 8193)                 # batch sizes whose references carry every entry of UPSTREAMS; elsewhere "all" alone
OUTPUTS = ("r", "mu", "lv", "z")
REC_W, REC_B = "decoder.reconstruction.weight", "decoder.reconstruction.bias"
BF16_BAR, BF16_COS = 0.3, 0.99
OPERAND_UNIT = {"bf16x3": 2.0 ** -17, "bf16": 2.0 ** -9}      # half the spacing of a 16-bit (hi + lo) / 8-bit significand
_INFO_PREFIX = "enc_dec_clf."


def params_of(model, y_dim):
    """The 14 tensors by their names in the module path's order.  M2_DEC: the encoder + decoder of an M2_info draw, prefix removed."""
    dims = gc.dims_of(y_dim)
    if model != "M2_DEC":
        return gu.make_params(model, dims, PARAM_SEED)
    full = gu.make_params("M2_info", dims, PARAM_SEED)
    return {k[len(_INFO_PREFIX):]: v for k, v in full.items() if k.startswith((_INFO_PREFIX + "encoder.", _INFO_PREFIX + "decoder."))}


def make_upstream(B, seed=UPSTREAM_SEED):
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(-6.0, 0.0, XD))
    up = {"r": rng.standard_normal((B, XD)) * s / B}
    for k in ("z", "mu", "lv"):
        up[k] = rng.standard_normal((B, ZD)) / B
    return {k: v.astype(np.float32) for k, v in up.items()}


def select(up, key):
    """(g_r, g_z, g_mu, g_lv) of an UPSTREAMS entry, None where not given"""
    return tuple(up[k] if k in UPSTREAMS[key] else None for k in ("r", "z", "mu", "lv"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the composition
# ---------------------------------------------------------------------------------------------------------------------------------

def forward(model, p, x, y, e):
    if model == "M1":
        return vo.m1_forward(p, x, e)
    if model == "M2":
        return vo.m2_forward(p, x, y, e)
    if model == "M2_DEC":
        return vo.m2v3_forward(p, x, y, e, prefix="")
    raise ValueError(model)


def backward(p, enc, dec, g_r, g_z, g_mu, g_lv):
    """Every parameter's gradient from the upstream gradients of (r, z, mu, log_var); None = zero."""
    zero = lambda like: np.zeros_like(like)
    grads = {}
    da = zero(dec["r"]) if g_r is None else g_r * dec["r"]
    dd = vo.decoder_bwd(p, grads, "decoder.", dec, da)
    dz = dd[:, :ZD] if g_z is None else dd[:, :ZD] + g_z
    vo.encoder_bwd(p, grads, "encoder.", enc, dz, zero(enc["mu"]) if g_mu is None else g_mu, zero(enc["lv"]) if g_lv is None else g_lv)
    return grads


class PolicyElementwiseF32:
    """vae_oracle.elementwise_hook for the float32 restatement: exp and tanh as struct PolBF16 of csrc/fused_tiles.hpp writes them,
    every operation rounded to float32 (numpy's float32 exp2 for the hardware's)."""
    LOG2E, TWO_LOG2E = np.float32(1.44269504088896341), np.float32(2.88539008177792681)

    @classmethod
    def exp(cls, v):
        assert v.dtype == np.float32
        return np.exp2(v * cls.LOG2E)

    @classmethod
    def tanh(cls, v):
        assert v.dtype == np.float32
        with np.errstate(over="ignore"):                    # exp2 -> inf: 2 / inf = 0, tanh = 1, as on the device
            return np.float32(1) - np.float32(2) / (np.exp2(v * cls.TWO_LOG2E) + np.float32(1))


class ThreeProductsF32(gc.OperandPolicy):
    """The second draw of the bf16x3 restatement (module docstring): split-bf16 operands as OperandPolicy(2, True) has them, every product
    as hi*hi + lo*hi + hi*lo in float32 through one accumulator in k-steps of 16.  The x block of encoder layer 1 stays the fp16 block of
    OperandPolicy.  Planes are made once per array; forget(keep) drops every array but those given."""
    STEP = 16

    def __init__(self):
        super().__init__(2, True)
        self.done = {}

    def planes(self, v):
        hit = self.done.get(id(v))
        if hit is None or hit[0] is not v:
            v32 = gc.f32(v)
            hi = gc.bf16(v32)
            hit = self.done[id(v)] = (v, hi, gc.bf16(v32 - hi))
        return hit[1], hit[2]

    def forget(self, keep):
        keep = {id(a) for a in keep}
        for k in [k for k in self.done if k not in keep]:
            del self.done[k]

    def _chain(self, a, b, ta=False, tb=False):
        """a @ b from the planes of a and b (ta / tb: of a.T / b.T), float64 out"""
        (ah, al), (bh, bl) = a, b
        if ta:
            ah, al = np.ascontiguousarray(ah.T), np.ascontiguousarray(al.T)
        if tb:
            bh, bl = np.ascontiguousarray(bh.T), np.ascontiguousarray(bl.T)
        af = ah + al                                                    # 16 significant bits: exact in float32
        acc = np.zeros((ah.shape[0], bh.shape[1]), np.float32)
        for k in range(0, ah.shape[1], self.STEP):
            acc = acc + (af[:, k:k + self.STEP] @ bh[k:k + self.STEP] + ah[:, k:k + self.STEP] @ bl[k:k + self.STEP])
        return acc.astype(np.float64)

    def fwd(self, name, x, W):
        if name in gc.L1X:
            return super().fwd(name, x, W)
        return self._chain(self.planes(x), self.planes(W), tb=True)

    def wgrad(self, name, dpre, inp):
        return self._chain(self.planes(dpre), self.planes(inp), ta=True)

    def bias(self, name, dpre):
        one = np.ones((dpre.shape[0], 1), np.float32)
        return self._chain(self.planes(dpre), (one, 0 * one), ta=True)[:, 0]

    def bwd(self, name, dpre, W):
        return self._chain(self.planes(dpre), self.planes(W))


class _ElementwiseAsF32:
    """PolicyElementwiseF32 inside a float64 run: the argument rounded to float32, the result carried on in float64"""
    exp = staticmethod(lambda v: PolicyElementwiseF32.exp(v.astype(np.float32)).astype(np.float64))
    tanh = staticmethod(lambda v: PolicyElementwiseF32.tanh(v.astype(np.float32)).astype(np.float64))


class Remembered:
    """An OperandPolicy of grad_columns whose operand rounding is done once per array: the same bits, but x, the activations and a layer's
    dpre (an operand of its weight gradient, its bias sum and its data gradient) are not split again for every product and every upstream
    combination.  forget(keep) drops every array but those given."""

    def __init__(self, policy):
        self.policy, self.done, rounding = policy, {}, policy.op

        def op(v):
            hit = self.done.get(id(v))
            if hit is None or hit[0] is not v:
                hit = self.done[id(v)] = (v, rounding(v))        # the array itself is held, so its id stays its own
            return hit[1]
        policy.op = op
        self.fwd, self.wgrad, self.bias, self.bwd = policy.fwd, policy.wgrad, policy.bias, policy.bwd

    def forget(self, keep):
        keep = {id(a) for a in keep}
        for k in [k for k in self.done if k not in keep]:
            del self.done[k]


def run(model, params, x, y, e, upstreams, dtype=np.float64, hook=None, elementwise=None):
    """-> (outputs, {key: gradients}): one forward in `dtype` under `hook`, one backward per entry of `upstreams` ({key: (g_r, g_z, g_mu,
    g_lv)}).  Everything comes back as float64 arrays; gradients in the parameters' shapes."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    p = {k: c(v) for k, v in params.items()}
    if isinstance(hook, gc.OperandPolicy) and not hasattr(hook, "forget"):
        hook = Remembered(hook)
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()), \
         (vo.elementwise_hook(elementwise) if elementwise is not None else contextlib.nullcontext()):
        enc, dec = forward(model, p, c(x), c(y), c(e))
        out = {k: np.asarray(v, np.float64) for k, v in (("r", dec["r"]), ("a", dec["a"]), ("mu", enc["mu"]), ("lv", enc["lv"]), ("z", enc["z"]))}
        grads = {}
        for key, ups in upstreams.items():
            g = backward(p, enc, dec, *(c(u) for u in ups))
            grads[key] = {k: np.asarray(g[k], np.float64).reshape(params[k].shape) for k in params}
            if hasattr(hook, "forget"):                    # the forward's arrays serve every upstream combination
                hook.forget([enc["inp"], *enc["hs"], dec["inp"], *dec["ds"], *p.values()])
    return out, grads


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics and bound
# ---------------------------------------------------------------------------------------------------------------------------------

def output_figures(got, truth):
    """{name: dict(worst, median)} of the outputs r (on log r), mu, lv, z; got: {name: array}, truth: the float64 outputs with "a"."""
    figs = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], np.float64)
        if k == "r":
            v = float(np.abs(np.log(g) - truth["a"]).max() / max(1.0, np.abs(truth["a"]).max()))
        else:
            v = float(np.abs(g - truth[k]).max() / np.abs(truth[k]).max())
        figs[k] = dict(worst=v, median=v)
    return figs


def grad_figures(grads, truth):
    """{name: grad_columns.column_figures} per input column, plus "<name> rows" for the reconstruction layer per output row."""
    figs = {k: gc.column_figures(grads[k], G) for k, G in truth.items()}
    figs[REC_W + " rows"] = gc.column_figures(np.asarray(grads[REC_W], np.float64).reshape(truth[REC_W].shape).T, truth[REC_W].T)
    figs[REC_B + " rows"] = gc.column_figures(np.asarray(grads[REC_B], np.float64).reshape(1, -1), truth[REC_B].reshape(1, -1))
    return figs


def merge(a, b):
    return {k: gc.merge_figures(a[k], b[k]) if "zero_ok" in a[k] else dict(worst=max(a[k]["worst"], b[k]["worst"]), median=max(a[k]["median"], b[k]["median"]))
            for k in a}


def _flat_pair(name, got, truth):
    """(got, truth) as flat float64 arrays for the tensor-level bf16 bar; r on log r"""
    if name == "r":
        return np.log(np.asarray(got, np.float64)).ravel(), truth["a"].ravel()
    base = name[:-len(" rows")] if name.endswith(" rows") else name
    t = truth[base]
    return np.asarray(got, np.float64).reshape(t.shape).ravel(), t.ravel()


def check(figs, got, truth, fig32, figpol, label="", bf16_bar=False):
    """Figures `figs` of the tensors `got` against the rule.  Prints one line per statistic; returns (failures, worst ratio to the bound,
    {name: ratio}).  figpol None: no policy term.  bf16_bar: a tensor whose bound exceeds 0.3 stands under the stated bf16 bar instead."""
    fails, ratios = [], {}
    for k, f in figs.items():
        bw, bm = gc.bound(fig32[k], figpol[k] if figpol is not None else None)
        if not f.get("zero_ok", True):
            fails.append((k, "a column whose float64 gradient is identically zero is not exactly zero"))
        if bf16_bar and bw > BF16_BAR:                                   # the stated bf16 bar in place of a bound that says nothing
            base = k[:-len(" rows")] if k.endswith(" rows") else k
            g, t = _flat_pair(k, got[base], truth)
            top = np.abs(t).max()
            rel = float(np.abs(g - t).max() / (top + 1e-300))
            cos = float(g @ t / (np.linalg.norm(g) * np.linalg.norm(t) + 1e-300)) if top > 0 else 1.0
            ratios[k] = rel / BF16_BAR
            print(f"{label} {k:46s} bf16 bar: {rel:.2e} of the maximum ({ratios[k]:5.2f} of 0.3), cosine {cos:.5f}   (rule's bound {bw:.2e})")
            if not (rel <= BF16_BAR and cos >= BF16_COS):
                fails.append((k, f"bf16 bar: {rel:.3e} of the maximum, cosine {cos:.5f}"))
            continue
        rw, rm = f["worst"] / (bw + 1e-300), f["median"] / (bm + 1e-300)
        ratios[k] = max(rw, rm)
        where = f"at column {f['arg']:4d}   median {f['median']:.2e} ({rm:5.2f})   zero columns {100 * f['zero_share']:.1f} %" if "arg" in f else ""
        print(f"{label} {k:46s} {f['worst']:.2e} ({rw:5.2f} of bound {bw:.2e}) {where}")
        if not f["worst"] <= bw:
            fails.append((k, f"worst: {f['worst']:.3e} > {bw:.3e}"))
        if not f["median"] <= bm:
            fails.append((k, f"median: {f['median']:.3e} > {bm:.3e}"))
    return fails, max(ratios.values(), default=0.0), ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# a case: inputs, truth, restatements (the policies' on first use)
# ---------------------------------------------------------------------------------------------------------------------------------

class Reference:
    def __init__(self, model, y_dim, B):
        self.model, self.y_dim, self.B = model, y_dim, B
        self.dims = gc.dims_of(y_dim)
        self.params = params_of(model, y_dim)
        self.x, self.y, self.e = gu.make_batch(self.dims, B, BATCH_SEED)
        self.up = make_upstream(B)
        self.keys = tuple(UPSTREAMS) if B in FULL_CROSS_AT else ("all",)
        self._build()

    @classmethod
    def at(cls, model, y_dim, params, x, y, e, up, keys=("all",)):
        """The reference on GIVEN float32 parameters, frames and upstream gradients (tests/later_steps.py) in the place of the case's."""
        self = cls.__new__(cls)
        self.model, self.y_dim, self.B, self.dims = model, y_dim, int(x.shape[0]), gc.dims_of(y_dim)
        self.params, self.x, self.y, self.e, self.up, self.keys = params, x, y, e, up, tuple(keys)
        self._build()
        return self

    def _build(self):
        for arr in (self.x, self.y, self.e, *self.up.values()):
            if arr is not None:
                arr.setflags(write=False)
        self.out, self.truth = self.run()
        # per key and bin: sqrt(sum_b da[b, k]^2) / |G[k]| of the reconstruction bias (the operand-format term of its per-row statistic)
        self.bias_condition = {}
        for key in self.keys:
            G, g_r = self.truth[key][REC_B], select(self.up, key)[0]
            live = G != 0
            da = 0.0 if g_r is None else g_r.astype(np.float64)[:, live] * self.out["r"][:, live]
            self.bias_condition[key] = np.sqrt(np.sum(da * da, axis=0)) / np.abs(G[live])
        a = self._figures(*self.run(dtype=np.float32))
        b = self._figures(*self.run(dtype=np.float32, hook=gc.KStepOrderF32(), elementwise=PolicyElementwiseF32))
        self.draws = {"fp32": a, "fp32 k-steps, the policies' exp and tanh": b}
        self.out_fig = {"fp32": merge(a[0], b[0])}
        self.grad_fig = {"fp32": {key: merge(a[1][key], b[1][key]) for key in self.keys}}

    def upstreams(self, keys=None):
        return {key: select(self.up, key) for key in (self.keys if keys is None else keys)}

    def run(self, dtype=np.float64, hook=None, keys=None, elementwise=None):
        return run(self.model, self.params, self.x, self.y, self.e, self.upstreams(keys), dtype, hook, elementwise)

    def _figures(self, out, grads):
        return output_figures(out, self.out), {key: grad_figures(g, self.truth[key]) for key, g in grads.items()}

    def policy(self, precision):
        """(output figures, {key: gradient figures}) of the restatement of an operand policy"""
        if precision not in self.out_fig:
            o, g = self._figures(*self.run(hook=gc.POLICIES[precision]()))
            self.draws[precision] = (o, g)
            if precision == "bf16x3":
                o2, g2 = self.draws["bf16x3, three products in float32"] = self._figures(*self.run(hook=ThreeProductsF32(), elementwise=_ElementwiseAsF32))
                o, g = merge(o, o2), {key: merge(g[key], g2[key]) for key in self.keys}
            for key in self.keys:                            # the operand-format term (module docstring)
                c = self.bias_condition[key]
                if c.size:
                    f = g[key][REC_B + " rows"]
                    g[key][REC_B + " rows"] = dict(f, worst=max(f["worst"], OPERAND_UNIT[precision] * float(c.max())),
                                                   median=max(f["median"], OPERAND_UNIT[precision] * float(np.median(c))))
            self.out_fig[precision], self.grad_fig[precision] = o, g
        return self.out_fig[precision], self.grad_fig[precision]

    def check_outputs(self, got, precision, label=""):
        po, _ = self.policy(precision)
        return check(output_figures(got, self.out), got, self.out, self.out_fig["fp32"], po, label, precision == "bf16")

    def check_grads(self, grads, key, precision, label=""):
        _, pg = self.policy(precision)
        return check(grad_figures(grads, self.truth[key]), grads, self.truth[key], self.grad_fig["fp32"][key], pg[key], label, precision == "bf16")


@functools.lru_cache(maxsize=None)
def reference(model, y_dim, B):
    return Reference(model, y_dim, B)

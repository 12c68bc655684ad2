"""Weight and bias gradients of the any-size fused train steps PER INPUT COLUMN and PER OUTPUT ROW against float64: tests/grad_columns.py
generalised to the M1 / M2 step (csrc/train_generic.hip), the classifier step (csrc/train_classifier.hip), the M2_info step in its modes
(csrc/train_info.hip) and gradient accumulation on top of them (train_generic_reduce_kernel, accumulate.py).  numpy only;
tests/test_grad_columns_generic_cpu.py and tests/test_gpu_train_columns.py use it.  grad_columns.py supplies the statistic
(column_figures), the bound (bound, MARGIN = 4, the floor F32_UNIT), merge_figures and make_speech_batch, unchanged.

All three steps take every weight and bias gradient from ONE kernel, train_generic_wgrad_kernel, and every other gradient check of that
code measures a tensor against its own largest element (grad_err of the three cases modules, 1e-4).  The columns of a layer fed by x
differ by orders of magnitude, label columns sit behind them at their own scale: a ragged block that is 1 % off, or never written,
moves that figure by 1e-5 (tests/test_grad_columns_generic_cpu.py seeds such faults).

A case is (kind, case, mode, B, ksplit[, family][, micro]):
    kind     "generic" (train_generic_cases), "clf" (train_classifier_cases), "info" (train_info_cases; a non-default mode:
             train_info_modes_cases.run_on)
    family   "bench": the inputs of the cases module, with its frame selection for the ReLU nets; "speech" (generic only, tanh nets, no
             selection needed): grad_columns.make_speech_batch, bins falling 60 dB; "real" (generic only): the bench inputs with y drawn
             uniform in [0, 1)
    micro    None: one step on B frames; (48, 48, 20): AccumulatedStep over those micro-batches, B their sum

Truth: the cases module's own oracle run in float64 on all B frames (M2_info: g1 + g2 on the auxiliary net, as `truth` returns it).

The float32 restatement, from the oracle and never from the library, in two summation orders; its figure is the larger of the two:
  numpy      run(case, B, np.float32) of the cases module: blocked GEMMs, pairwise sums.
  k-steps    the kernels' order through vae_oracle.gemm_hook (StepOrderF32), read from csrc/train_tables.hpp (tg_gemm) and
             csrc/train_tables.hip (train_generic_wgrad_kernel, slab_sum_at's order, train_generic_reduce_kernel):
             * a forward or backward-data product is ONE float32 accumulator over k ascending, one mfma_f32_16x16x4f32 per four k
               (frag_pos: MFMA i of k block b holds k = 16 b + 4 i .. + 3).  [x | y] and [z | y] are two packed blocks, each padded with
               zeros to a multiple of 16, summed into the same accumulator x (z) first: the groups of four start again at the first
               label column.  d h2e = [d mu | d log_var] [Wmu; Wlv] is one accumulator over both heads, mu first.
             * a weight gradient is one accumulator per frame slice, one MFMA per four frames f .. f + 3 (frames past the slice end are
               zeros); the bias is the same product with a column of ones.  slice_frames follows choose_slices.  The slices' slabs are
               added in slab order.
             * accumulated: flat = G_0, then flat + fl(w_k G_k) with w_k = fl32(B_k / B_0) (two roundings, contraction off), and
               grads_numpy() multiplies by fl32(B_0 / sum B_k); G_k is micro-batch k's own mean gradient (invB = 1 / B_k).
             * inside one MFMA the four terms enter the accumulator one after the other, each by ONE fused multiply-add: the product
               is not rounded, the sum is (v_mfma_f32_16x16x4_f32 is exact float32 arithmetic, a chain of fmaf).  Restated as
               float32(float64(acc) + float64(a) float64(b)): the product of two 24-bit significands is exact in float64, and rounding
               the sum to 53 bits before 24 differs from fmaf only on a tie of the second rounding, about one sum in 2^29.
               Added because the device needed it.  With numpy's float32 dot of four terms in its place the first device run left the
               bound at three cases of 32: (3, 17, (129, 127)) at one frame (encoder layer 2's weight, column 92: 7.0e-5 against
               4 x 9.0e-6), (1, 5, (48, 200)) at one frame (the mu bias: 1.26e-6 against 4 x 2.1e-7) and the classifier's accumulated
               step (layer 2's weight, column 27: 4.7e-6 against 4 x 1.0e-6).  A chain of n fused terms carries the rounding of every
               partial sum, an error that grows with n and with the largest partial sum on the way; numpy's blocked GEMM and
               pairwise sums keep neither.  At ONE frame a column of a weight gradient is dpre x in[k], so its figure IS the relative
               float32 error of one activation: of one sum of 516 (129) terms.  The fused chain on the CPU returns 7.00e-5, 1.26e-6
               and 4.69e-6 for those three figures, the device's own to three digits, so nothing else is missing there.
Everything that is not a product (tanh, exp, the sigmoid, the loss derivatives) is float32 numpy in both orders.

Statistic.  grad_columns.column_figures per tensor (worst column, median column, columns whose truth is identically zero; a bias is one
column), and the same figure per OUTPUT ROW of every weight matrix.  A column (row) whose float64 gradient is identically zero must be
+0.0 in every element: the accumulators start at +0.0 and only ever add signed zeros to it, so -0.0 or 1e-30 there is something else
written.

Bound (grad_columns.bound, fp32 policy): worst column <= 4 x max(float32 restatement, 2^-24); median column and median row by the same
rule.  The worst row is printed and not held: it is the tail of a tanh unit whose gradient nearly cancels, float32 numpy itself reaches
2.5e-4 and 6e-4 on one row of encoder layer 1 at (3, 17, (129, 127)) and (513, 128, (512, 512)).  No device figure enters a bound.
"""
import contextlib
import functools

import numpy as np

import grad_columns as gcol
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic
import train_info_modes_cases as mc
from grad_columns import F32_UNIT, MARGIN, bound, column_figures, make_speech_batch, merge_figures     # noqa: F401 (re-exported)
from oracle import vae_oracle as vo

XD = 513
MODS = {"generic": gc, "clf": cc, "info": ic}
DEFAULT_MODE = ("truth", "bce")
SPEECH_SEED = gcol.SEEDS["speech"][1]
REAL_LABEL_SEED = 33
MAX_SLICES = 16                          # G_MAX_SLICES
ORDERS = ("numpy", "k-steps")            # the two summation orders of the float32 restatement


# The cases: (kind, case, mode, B, ksplit, family, micro), the smallest existing ones that reach each ragged path of the weight-gradient
# kernel -- column 512 alone in the ninth block, label blocks of 1, 3, 17 and 513 columns behind in_w, the bias block in each of a
# workgroup's four waves, row tiles and rows past the matrix, one frame, a ragged last four frames, 513-float rows.
_G = [(3, 17, (129, 127)), (513, 128, (512, 512)), (1, 5, (48, 200)), (513, 64, (16, 16)), (0, 1, (1, 1)), (0, 32, (256, 64))]
_I = (3, 17, (129, 127))
GENERIC_CASES = ([("generic", c, None, B, 1, "bench", None) for c in _G for B in (1, 50)]
                 + [("generic", c, None, 50, 4, "bench", None) for c in _G[:2]]
                 + [("generic", c, None, 50, 1, "speech", None) for c in (_G[0], _G[5])]
                 + [("generic", _G[0], None, 50, 1, "real", None)])
CLF_CASES = ([("clf", c, None, 50, 1, "bench", None) for c in (((129, 127), 17), ((512, 512), 513), ((48, 200), 2), ((1, 1), 1))]
             + [("clf", ((129, 127), 17), None, 1, 1, "bench", None), ("clf", ((129, 127), 17), None, 50, 4, "bench", None)])
INFO_CASES = ([("info", c, DEFAULT_MODE, 50, 1, "bench", None) for c in (_I, (513, 128, (512, 512)), (1, 1, (1, 1)))]
              + [("info", _I, ("classifier", "entropy"), 50, 1, "bench", None), ("info", _I, ("classifier", "entropy"), 50, 4, "bench", None),
                 ("info", _I, ("truth", "uniform"), 50, 1, "bench", None)])
MICRO = (48, 48, 20)
ACCUMULATED_CASES = [("generic", (513, 128, (512, 512)), None, 116, 0, "bench", MICRO), ("clf", ((48, 200), 2), None, 116, 0, "bench", MICRO),
                     ("info", _I, DEFAULT_MODE, 116, 0, "bench", MICRO)]            # the F64_CASES of tests/test_gpu_train_accumulate.py
ALL_CASES = GENERIC_CASES + CLF_CASES + INFO_CASES + ACCUMULATED_CASES


def case_label(kind, case, mode, B, ksplit, family="bench", micro=None):
    s = f"{kind} {MODS[kind].case_id(case)}"
    if kind == "info" and mode not in (None, DEFAULT_MODE):
        s += " " + mc.mode_id(mode)
    if family != "bench":
        s += " " + family
    return s + f" B{B}" + (f" ksplit{ksplit}" if ksplit != 1 else "") + (" micro " + "+".join(map(str, micro)) if micro else "")


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan's frame slices (csrc/train_tables.hpp: choose_slices)
# ---------------------------------------------------------------------------------------------------------------------------------

def slice_plan(B, ksplit):
    """(slice_frames, nslices) of a plan asked for `ksplit` slices; 0 (choose) only below 128 frames, where the choice is one slice
    whatever the geometry (ks <= B / 64)."""
    ks = int(ksplit)
    if ks <= 0:
        assert B < 128, "choose_slices picks by the item count from 128 frames on: ask for a ksplit"
        ks = 1
    ks = max(1, min(ks, MAX_SLICES))
    sf = (-(-B // ks) + 15) // 16 * 16
    return sf, -(-B // sf)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' summation order
# ---------------------------------------------------------------------------------------------------------------------------------

class StepOrderF32:
    """grad_columns.KStepOrderF32 with its constants as parameters (a hook for the oracle run in float32; in float64 it only reorders):
    kstep terms of a forward / backward-data reduction per step through one accumulator, fstep frames per step of a weight-gradient
    reduction, one accumulator per slice of slice_frames frames, the slices added in order.  z_dim: where decoder layer 1's input
    splits into its two packed blocks (encoder layer 1's splits behind x).  fused: a step's terms enter by one fused multiply-add
    each, as the f32 MFMA adds them; False: a step is numpy's dot of its terms, as in KStepOrderF32."""

    def __init__(self, slice_frames, z_dim=None, kstep=4, fstep=4, fused=True):
        self.slice_frames, self.z_dim, self.kstep, self.fstep, self.fused = int(slice_frames), z_dim, int(kstep), int(fstep), bool(fused)
        self._mu = None

    def _chain(self, a, b, step, acc=None):
        """acc + a @ b, the reduction axis in steps of `step` through one accumulator of the operands' dtype.  fused (float32 only):
        the terms of a step enter one by one, each by a fused multiply-add (see the module docstring); a step's width then changes
        nothing, and the zeros that pad a block or a slice leave the accumulator as it is."""
        if acc is None:
            acc = np.zeros((a.shape[0], b.shape[1]), a.dtype)
        if self.fused and a.dtype == np.float32:
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            for k in range(a.shape[1]):
                acc = (acc.astype(np.float64) + a64[:, k:k + 1] * b64[k]).astype(np.float32)
            return acc
        for k in range(0, a.shape[1], step):
            acc = acc + a[:, k:k + step] @ b[k:k + step]
        return acc

    def _split(self, name, width):
        if name.endswith("encoder.hidden.0") and width > XD:
            return XD
        if name.endswith("decoder.hidden.0") and self.z_dim is not None and width > self.z_dim:
            return self.z_dim
        return width

    def fwd(self, name, x, W):
        s = self._split(name, x.shape[1])
        Wt = np.ascontiguousarray(W.T)
        acc = self._chain(x[:, :s], Wt[:s], self.kstep)
        return acc if s == x.shape[1] else self._chain(x[:, s:], Wt[s:], self.kstep, acc)

    def _sliced(self, dpre, inp):
        total = None
        for f0 in range(0, dpre.shape[0], self.slice_frames):
            part = self._chain(np.ascontiguousarray(dpre[f0:f0 + self.slice_frames].T), inp[f0:f0 + self.slice_frames], self.fstep)
            total = part if total is None else total + part
        return total

    def wgrad(self, name, dpre, inp):
        return self._sliced(dpre, inp)

    def bias(self, name, dpre):
        return self._sliced(dpre, np.ones((dpre.shape[0], 1), dpre.dtype))[:, 0]

    def bwd(self, name, dpre, W):
        if name.endswith("sample.mu"):                  # vo.encoder_bwd adds the two heads' products: 0 + (both in one accumulator)
            self._mu = (dpre, W)
            return np.zeros((dpre.shape[0], W.shape[1]), dpre.dtype)
        if name.endswith("sample.log_var") and self._mu is not None:
            (dmu, Wmu), self._mu = self._mu, None
            return self._chain(dpre, W, self.kstep, self._chain(dmu, Wmu, self.kstep))
        return self._chain(dpre, W, self.kstep)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle of a kind on given frames, in a dtype, under a hook
# ---------------------------------------------------------------------------------------------------------------------------------

def oracle_grads(kind, case, mode, params, x, y, e, dtype, hook=None):
    """One step's gradients (float64 arrays, the tensors the GPU tests compare) by the cases module's own run."""
    ctx = vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()
    with ctx:
        if kind == "generic":
            c = lambda a: None if a is None else a.astype(dtype)
            p = {k: c(v) for k, v in params.items()}
            _, g = vo.train_step_vae(gc.model_of(case), p, vo.AdamState(list(p)), c(x), c(y), c(e), lr=1e-4)       # what gc.run does
            return {k: np.asarray(v, np.float64).reshape(params[k].shape) for k, v in g.items()}
        if kind == "clf":
            return cc.run_on(params, x, y, dtype)[1][0]
        if mode in (None, DEFAULT_MODE):
            return ic.run_on(params, x, y, e, dtype)[1][0]
        return mc.run_on(params, x, y, e, dtype, mode)[1][0]


def case_inputs(kind, case, B, family="bench"):
    """(params, x, y, eps) of a case; eps None for the classifier."""
    if kind == "clf":
        assert family == "bench"
        return cc.inputs(case, B) + (None,)
    if family == "bench":
        return MODS[kind].inputs(case, B)
    assert kind == "generic", "the other families are for the tanh nets: no frame selection exists for them"
    params, x, y, e = gc.inputs(case, B)
    if family == "speech":
        x, y, e = make_speech_batch(gc.dims_of(case), B, SPEECH_SEED)
    elif family == "real":
        y = np.random.default_rng(REAL_LABEL_SEED).random(y.shape).astype(np.float32)
    else:
        raise ValueError(family)
    for a in (x, y, e):
        if a is not None:
            a.setflags(write=False)
    return params, x, y, e


def accumulate_f32(parts, sizes):
    """train_generic_reduce_kernel over micro-batch gradients `parts` (float32 arrays of micro-batches of `sizes` frames) and the
    scale of AccumulatedStep.grads_numpy(): every product and sum rounded to float32."""
    flat = parts[0].astype(np.float32)
    for g, b in zip(parts[1:], sizes[1:]):
        flat = flat + np.float32(b / sizes[0]) * g.astype(np.float32)
    return flat * np.float32(float(sizes[0]) / float(sum(sizes)))


# ---------------------------------------------------------------------------------------------------------------------------------
# figures
# ---------------------------------------------------------------------------------------------------------------------------------

def is_matrix(G):
    return np.ndim(G) == 2


def row_figures(g, G):
    """column_figures over the output rows of a weight matrix"""
    G = np.asarray(G, np.float64)
    return column_figures(np.asarray(g, np.float64).reshape(G.shape).T, G.T)


def zeros_are_plus_zero(g, G):
    """every element of g in a column or row whose truth is identically zero is +0.0"""
    G = np.asarray(G, np.float64)
    g = np.asarray(g).reshape(G.shape)
    if G.ndim == 1:
        dead = np.broadcast_to(not np.any(G), G.shape)
    else:
        dead = ~np.any(G, axis=0)[None, :] | ~np.any(G, axis=1)[:, None]
    v = g[dead]
    return bool(np.all(v == 0) and not np.any(np.signbit(v)))


class Reference:
    def __init__(self, kind, case, mode, B, ksplit, family="bench", micro=None):
        self.key = (kind, case, mode, B, ksplit, family, micro)
        self.label = case_label(*self.key)
        self.params, self.x, self.y, self.e = case_inputs(kind, case, B, family)
        if family == "bench" and mode in (None, DEFAULT_MODE):
            self._build(MODS[kind].truth(case, B)[1][0])
        elif family == "bench":
            self._build(mc.truth(case, B, tuple(mode))[1][0])
        else:
            self._build()

    @classmethod
    def at(cls, kind, case, mode, params, x, y, e, ksplit, micro=None, label=None):
        """The reference of one step on GIVEN float32 parameters and frames (tests/later_steps.py: step k of a trainer, whose
        parameters are what the device reports before it) in the place of case_inputs(...); everything else as __init__ builds it."""
        self = cls.__new__(cls)
        self.key = (kind, case, None if mode is None else tuple(mode), int(x.shape[0]), ksplit, "given", micro)
        self.label = case_label(*self.key) if label is None else label
        self.params, self.x, self.y, self.e = params, x, y, e
        self._build()
        return self

    def _build(self, truth=None):
        """truth None: the float64 oracle on the frames as they stand (what the cases modules' cached truths hold, bit for bit)."""
        kind, case, mode, B, ksplit, family, micro = self.key
        self.z_dim = None if kind == "clf" else case[1]
        self.truth = self.run(np.arange(B), np.float64) if truth is None else truth
        self.sizes = (B,) if micro is None else tuple(micro)
        assert sum(self.sizes) == B
        self.plans = [slice_plan(b, ksplit) for b in self.sizes]
        self.slice_frames, self.nslices = self.plans[0]
        self.restated = {name: self.restate(name) for name in ORDERS}
        self.draws = {n: {k: column_figures(g[k], self.truth[k]) for k in self.truth} for n, g in self.restated.items()}
        self.row_draws = {n: {k: row_figures(g[k], G) for k, G in self.truth.items() if is_matrix(G)} for n, g in self.restated.items()}
        self.figures = {k: merge_figures(self.draws["numpy"][k], self.draws["k-steps"][k]) for k in self.truth}
        self.row_figures = {k: merge_figures(self.row_draws["numpy"][k], self.row_draws["k-steps"][k]) for k in self.row_draws["numpy"]}

    def run(self, frames, dtype, hook=None):
        """the oracle on the given frames of the case (an index array)"""
        kind, case, mode = self.key[:3]
        sub = lambda a: None if a is None else a[frames]
        return oracle_grads(kind, case, mode, self.params, sub(self.x), sub(self.y), sub(self.e), dtype, hook)

    def hook(self, i=0, slice_frames=None):
        return StepOrderF32(self.plans[i][0] if slice_frames is None else slice_frames, self.z_dim)

    def restate(self, order, perm=None):
        """The float32 restatement in `order` ("numpy" or "k-steps") on the frames in the order `perm` (default: as they stand): one
        step, or the micro-batches combined as the reduce kernel combines them."""
        perm = np.arange(self.key[3]) if perm is None else np.asarray(perm)
        parts, lo = [], 0
        for i, b in enumerate(self.sizes):
            parts.append(self.run(perm[lo:lo + b], np.float32, self.hook(i) if order == "k-steps" else None))
            lo += b
        if len(parts) == 1:
            return parts[0]
        return {k: accumulate_f32([p[k] for p in parts], self.sizes).astype(np.float64) for k in self.truth}

    def truth_copy(self):
        return {k: np.array(v, np.float64) for k, v in self.truth.items()}


@functools.lru_cache(maxsize=None)
def reference(kind, case, mode, B, ksplit, family="bench", micro=None):
    return Reference(kind, case, None if mode is None else tuple(mode), B, ksplit, family, micro)


# ---------------------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------------------

def check(grads, ref, label=None, signed_zeros=True, quiet=False):
    """Every tensor of `grads` against ref (a Reference).  Prints one line per tensor, returns the list of failures (empty: pass) and
    the worst ratio of a held figure to its bound.  signed_zeros False: a zero column may hold -0.0 (numpy's pairwise sum of a column
    of -0.0 is -0.0; the kernels' accumulators start at +0.0)."""
    label = ref.label if label is None else label
    fails, top = [], 0.0
    say = (lambda *a: None) if quiet else print
    for k, G in ref.truth.items():
        f = column_figures(grads[k], G)
        bw, bm = bound(ref.figures[k])
        rw, rm = f["worst"] / bw, f["median"] / bm
        top = max(top, rw, rm)
        line = (f"[{label}] {k:46s} worst column {f['worst']:.2e} ({rw:5.2f} of bound) at {f['arg']:4d}   median {f['median']:.2e} ({rm:5.2f})")
        if is_matrix(G):
            r = row_figures(grads[k], G)
            _, brm = bound(ref.row_figures[k])
            rrm = r["median"] / brm
            top = max(top, rrm)
            line += f"   worst row {r['worst']:.2e} at {r['arg']:3d} (not held)   median row {r['median']:.2e} ({rrm:5.2f})"
            if not r["zero_ok"]:
                fails.append((k, "a row whose float64 gradient is identically zero is not exactly zero"))
            if not r["median"] <= brm:
                fails.append((k, f"median row: {r['median']:.3e} > {brm:.3e}"))
        say(line + f"   zero columns {100 * f['zero_share']:.1f} %   tensor-level {f['tensor']:.1e}")
        if not f["zero_ok"] or (signed_zeros and not zeros_are_plus_zero(grads[k], G)):
            fails.append((k, "a column whose float64 gradient is identically zero is not exactly +0.0"))
        if not f["worst"] <= bw:
            fails.append((k, f"worst column {f['arg']}: {f['worst']:.3e} > {bw:.3e}"))
        if not f["median"] <= bm:
            fails.append((k, f"median column: {f['median']:.3e} > {bm:.3e}"))
    say(f"[{label}] worst ratio to the bound: {top:.3f}")
    return fails, top

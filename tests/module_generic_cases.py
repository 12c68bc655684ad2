"""The whole-model module path at any covered size (disentangled-vae_amd/module_path.py: GenericModuleEngine; dvae_module_generic_forward /
dvae_module_generic_backward, the generic rows kernel in its two module modes) against float64: truth, restatements, statistics, bound,
inputs and cases (numpy only; tests/test_module_generic_cpu.py and tests/test_gpu_module_generic.py use it).

Truth.  The composition of tests/module_cases.py for any z_dim: oracle/vae_oracle.py in float64 on the float32 inputs, m1_forward /
m2_forward -> r, a = log r, mu, log_var, z; backward from the upstream gradients (g_r, g_z, g_mu, g_lv), each possibly None = zero:
da = g_r * r;  dd = decoder_bwd(.., da);  dz = dd[:, :z] + g_z;  encoder_bwd(.., dz, g_mu, g_lv).  Pinned against torch.float64 autograd of
the drop-in modules in the CPU test.

Float32 restatement (from the oracle, never from the library): the same composition in float32 in two summation orders, the larger
figure of the two -- numpy's, and the kernels' k-step order with fused multiply-adds, grad_columns_generic.StepOrderF32 on the plan's
frame slices (slice_plan below restates choose_slices of csrc/train_tables.hpp; the CPU test holds it against the library's plans).
tanh and exp are float32 numpy in both.  The path is exact fp32: there is no policy term.

Statistics.  module_cases.output_figures / grad_figures: log r; mu, log_var, z over the tensor maximum; every gradient per input column,
the reconstruction layer also per output row.  Bound: grad_columns.bound, statistic <= 4 x max(float32 restatement, 2^-24).  No device
figure enters a bound.

Cases.  Geometries (y, z, (h1, h2)): grad_columns_generic._G, plus (1, 16, (128, 128)) -- the reference geometry, which reaches the generic
engine under DVAE_MODULE_GENERIC=force only.  Frames (tiles are 16 frames): 1, 15, 16, 17 at the first geometry, whose sizes are all off
every multiple of 16; one batch of train_generic_cases.loops_batch at its LOOPS_CASE (more tiles than workgroups: the tile loop runs more
than once; two frame slices, the last shorter); 50 (three tiles and a ragged fourth) everywhere.  Upstream sets: all of
module_cases.UPSTREAMS at 17 frames, "all" elsewhere.  Inputs: train_generic_cases.inputs (parameters seed 11, batch seed 12); upstream
gradients as module_cases.make_upstream draws them, with [B, z] latent gradients: g_r = N(0, 1) s_k / B with per-bin scales s_k =
exp(U(-6, 0)) over six decades, g_z, g_mu, g_lv = N(0, 1) / B.
"""
import contextlib
import functools

import numpy as np

import grad_columns_generic as gg
import module_cases as mc
import train_generic_cases as gc
from oracle import vae_oracle as vo

XD = 513
UPSTREAM_SEED = mc.UPSTREAM_SEED
UPSTREAMS = mc.UPSTREAMS
REFERENCE_GEOMETRY = (1, 16, (128, 128))
GEOMETRIES = list(gg._G) + [REFERENCE_GEOMETRY]
EDGE_CASE, EDGE_FRAMES, FULL_CROSS_AT, COMMON_FRAMES = gg._G[0], (1, 15, 16, 17), 17, 50
LOOPS_CASE = gc.LOOPS_CASE
MAX_SLICES, ROWS_GRID = gg.MAX_SLICES, 256


def forced(case):
    """the geometry reaches the generic engine under `force` only"""
    return case == REFERENCE_GEOMETRY


def forward_cases(loops_B):
    """[(case, B)]; loops_B: the batch of train_generic_cases.loops_batch (the caller asks the library's plans for it)"""
    return ([(EDGE_CASE, B) for B in EDGE_FRAMES] + [(c, COMMON_FRAMES) for c in GEOMETRIES] + [(LOOPS_CASE, loops_B)])


def backward_cases(loops_B):
    """[(case, B, upstream key)]"""
    return [(c, B, key) for c, B in forward_cases(loops_B) for key in (UPSTREAMS if B == FULL_CROSS_AT else ("all",))]


def case_id(case, B, key=None):
    return f"{gc.case_id(case)}-B{B}" + (f"-{key}" if key else "")


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan's frame slices (csrc/train_tables.hpp: choose_slices, gemm_items; csrc/train_generic.hip: make_gemms)
# ---------------------------------------------------------------------------------------------------------------------------------

def slice_plan(case, B, ksplit=0):
    """(slice_frames, nslices) of dvae_train_generic_plan(case, B, ksplit)"""
    y, z, (h1, h2) = case
    t16 = lambda v: -(-v // 16)
    b64 = lambda v: -(-v // 64)
    gemms = [(t16(h1), XD, y), (t16(h2), h1, 0), (t16(z), h2, 0), (t16(z), h2, 0), (t16(h2), z, y), (t16(h1), h2, 0), (33, h1, 0)]
    row_tiles = sum(-(-nrt // 4) * -(-(b64(w) + b64(yw) + 1) // 4) for nrt, w, yw in gemms)
    ks = int(ksplit)
    if ks <= 0:
        ks = min(-(-768 // row_tiles), B // 64)
    ks = max(1, min(ks, MAX_SLICES))
    sf = (-(-B // ks) + 15) // 16 * 16
    return sf, -(-B // sf)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the composition
# ---------------------------------------------------------------------------------------------------------------------------------

def make_upstream(B, z, seed=UPSTREAM_SEED):
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(-6.0, 0.0, XD))
    up = {"r": rng.standard_normal((B, XD)) * s / B}
    for k in ("z", "mu", "lv"):
        up[k] = rng.standard_normal((B, z)) / B
    return {k: v.astype(np.float32) for k, v in up.items()}


select = mc.select


def backward(p, enc, dec, z, g_r, g_z, g_mu, g_lv):
    """module_cases.backward with the latent width as a parameter"""
    zero = lambda like: np.zeros_like(like)
    grads = {}
    da = zero(dec["r"]) if g_r is None else g_r * dec["r"]
    dd = vo.decoder_bwd(p, grads, "decoder.", dec, da)
    dz = dd[:, :z] if g_z is None else dd[:, :z] + g_z
    vo.encoder_bwd(p, grads, "encoder.", enc, dz, zero(enc["mu"]) if g_mu is None else g_mu, zero(enc["lv"]) if g_lv is None else g_lv)
    return grads


def run(case, params, x, y, e, upstreams, dtype=np.float64, hook=None, back=backward):
    """-> (outputs, {key: gradients}): one forward in `dtype` under `hook`, one backward per entry of `upstreams` ({key: (g_r, g_z, g_mu,
    g_lv)}); float64 arrays out.  back: the backward composition (the CPU test seeds faults through it)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    p = {k: c(v) for k, v in params.items()}
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
        enc, dec = mc.forward(gc.model_of(case), p, c(x), c(y), c(e))
        out = {k: np.asarray(v, np.float64) for k, v in (("r", dec["r"]), ("a", dec["a"]), ("mu", enc["mu"]), ("lv", enc["lv"]), ("z", enc["z"]))}
        grads = {}
        for key, ups in upstreams.items():
            g = back(p, enc, dec, case[1], *(c(u) for u in ups))
            grads[key] = {k: np.asarray(g[k], np.float64).reshape(params[k].shape) for k in params}
    return out, grads


# ---------------------------------------------------------------------------------------------------------------------------------
# a case: inputs, truth, the float32 restatement in its two orders
# ---------------------------------------------------------------------------------------------------------------------------------

class Reference:
    def __init__(self, case, B):
        self.case, self.B = tuple(case), B
        self.params, self.x, self.y, self.e = gc.inputs(case, B)
        self.up = make_upstream(B, case[1])
        self.keys = tuple(UPSTREAMS) if B == FULL_CROSS_AT else ("all",)
        self._build()

    @classmethod
    def at(cls, case, params, x, y, e, up, keys=("all",)):
        """The reference on GIVEN float32 parameters, frames and upstream gradients (tests/later_steps.py) in the place of the case's."""
        self = cls.__new__(cls)
        self.case, self.B = tuple(case), int(x.shape[0])
        self.params, self.x, self.y, self.e, self.up, self.keys = params, x, y, e, up, tuple(keys)
        self._build()
        return self

    def _build(self):
        case, B = self.case, self.B
        for a in self.up.values():
            a.setflags(write=False)
        self.slice_frames, self.nslices = slice_plan(case, B)
        self.out, self.truth = self.run()
        a = self._figures(*self.run(np.float32))
        b = self._figures(*self.run(np.float32, gg.StepOrderF32(self.slice_frames, case[1])))
        self.draws = {"numpy": a, "k-steps": b}
        self.out_fig = mc.merge(a[0], b[0])
        self.grad_fig = {key: mc.merge(a[1][key], b[1][key]) for key in self.keys}

    def upstreams(self):
        return {key: select(self.up, key) for key in self.keys}

    def run(self, dtype=np.float64, hook=None, back=backward):
        return run(self.case, self.params, self.x, self.y, self.e, self.upstreams(), dtype, hook, back)

    def _figures(self, out, grads):
        return mc.output_figures(out, self.out), {key: mc.grad_figures(g, self.truth[key]) for key, g in grads.items()}

    def check_outputs(self, got, label=""):
        """-> (failures, worst ratio to the bound, {name: ratio})"""
        return mc.check(mc.output_figures(got, self.out), got, self.out, self.out_fig, None, label)

    def check_grads(self, grads, key, label=""):
        return mc.check(mc.grad_figures(grads, self.truth[key]), grads, self.truth[key], self.grad_fig[key], None, label)


@functools.lru_cache(maxsize=None)
def reference(case, B):
    return Reference(case, B)

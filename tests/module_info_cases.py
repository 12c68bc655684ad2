"""The M2_info body ("M2_DEC": encoder on x alone, decoder on [z | y]) of any covered size on the generic module engine
(disentangled-vae_amd/module_path.py: GenericModuleEngine on a plan of dvae_module_generic_plan; the DEC variant of the generic rows
kernel's two module modes, dvae_module_generic_backward_y) against float64: truth, restatements, statistics, bound, inputs and cases
(numpy only; tests/test_module_info_cpu.py and tests/test_gpu_module_info.py use it).  Built on tests/module_generic_cases.py, whose
composition, upstream gradients, statistics and bound it imports.

Truth.  oracle/vae_oracle.py in float64 on the float32 inputs: m2v3_forward(p, x, y, e, prefix="") -> r, a = log r, mu, log_var, z;
module_generic_cases.backward from the upstream gradients (g_r, g_z, g_mu, g_lv), each possibly None = zero, for the 14 parameter
gradients; and the label gradient g_y = dd[:, z:] of dd = decoder_bwd(.., da), da = g_r * r -- the decoder's share and the only one, the
encoder does not see y.  Pinned against torch.float64 autograd of DeepGenerativeModel_v3 with y.requires_grad_() in the CPU test.

Float32 restatement (from the oracle, never from the library): the same composition in float32 in numpy's order and in the kernels'
k-step order (grad_columns_generic.StepOrderF32 on the plan's frame slices), the larger figure of the two.  slice_plan below restates
choose_slices for an M2_DEC plan -- matrix 0 has no label columns (yw = 0) --; the CPU test holds it against the library's plans.

Statistics.  module_cases.output_figures / grad_figures for the outputs and the 14 gradients.  g_y: per label column at its own scale,
as grad_figures scores a gradient per input column ("g_y"), and max |got - truth| / max |truth| of the tensor ("g_y tensor").  A label
column whose float64 gradient is identically zero (no g_r upstream: nothing reaches the decoder) must be exactly zero.
Bound: grad_columns.bound, statistic <= 4 x max(float32 restatement, 2^-24).  No device figure enters a bound.

Cases (y, z, (h1, h2)): GEOMETRIES; (1, 16, (128, 128)) is the reference geometry, which reaches the generic engine under
DVAE_MODULE_INFO_BODY=force only.  Frames: 1, 15, 16, 17 at the first geometry; 50 everywhere; the train_generic_cases.loops_batch batch
at (1, 5, (48, 200)).  Upstream sets: every entry of UPSTREAMS at 17 frames, "all" elsewhere.  Inputs: the encoder and decoder of
golden_util.make_params("M2_info", dims, 11), batch golden_util.make_batch(dims, B, 12), upstream gradients of
module_generic_cases.make_upstream.
"""
import contextlib
import functools

import numpy as np

import golden_util as gu
import module_generic_cases as mg
import train_generic_cases as gc
from module_generic_cases import gg, mc, vo

XD = mg.XD
UPSTREAMS = mg.UPSTREAMS
REFERENCE_GEOMETRY = (1, 16, (128, 128))
GEOMETRIES = [(3, 17, (129, 127)), (513, 128, (512, 512)), (1, 5, (48, 200)), (513, 64, (16, 16)), (1, 1, (1, 1)), (513, 16, (128, 128)),
              REFERENCE_GEOMETRY]
EDGE_CASE, EDGE_FRAMES, FULL_CROSS_AT, COMMON_FRAMES = GEOMETRIES[0], (1, 15, 16, 17), 17, 50
LOOPS_CASE = gc.LOOPS_CASE
GY, GY_TENSOR = "g_y", "g_y tensor"
_PREFIX = "enc_dec_clf."


def forced(case):
    """the geometry reaches the generic engine under `force` only"""
    return case == REFERENCE_GEOMETRY


def forward_cases(loops_B):
    return [(EDGE_CASE, B) for B in EDGE_FRAMES] + [(c, COMMON_FRAMES) for c in GEOMETRIES] + [(LOOPS_CASE, loops_B)]


def backward_cases(loops_B):
    """[(case, B, upstream key, g_y requested)]"""
    out = []
    for c, B in forward_cases(loops_B):
        if B == FULL_CROSS_AT:
            out += [(c, B, key, gy) for key in UPSTREAMS for gy in (True, False)]
        else:
            out.append((c, B, "all", True))
    return out


def case_id(case, B, key=None, gy=None):
    return mg.case_id(case, B, key) + ("" if gy is None else "-gy" if gy else "-nogy")


def slice_plan(case, B, ksplit=0):
    """(slice_frames, nslices) of dvae_module_generic_plan(M2_DEC, case, B, ksplit): module_generic_cases.slice_plan with yw = 0 for matrix 0"""
    y, z, (h1, h2) = case
    t16 = lambda v: -(-v // 16)
    b64 = lambda v: -(-v // 64)
    gemms = [(t16(h1), XD, 0), (t16(h2), h1, 0), (t16(z), h2, 0), (t16(z), h2, 0), (t16(h2), z, y), (t16(h1), h2, 0), (33, h1, 0)]
    row_tiles = sum(-(-nrt // 4) * -(-(b64(w) + b64(yw) + 1) // 4) for nrt, w, yw in gemms)
    ks = int(ksplit)
    if ks <= 0:
        ks = min(-(-768 // row_tiles), B // 64)
    ks = max(1, min(ks, mg.MAX_SLICES))
    sf = (-(-B // ks) + 15) // 16 * 16
    return sf, -(-B // sf)


@functools.lru_cache(maxsize=None)
def inputs(case, B):
    """(params, x, y, eps) in float32; shared, never written.  params: the 14 tensors of the body by the module path's names"""
    dims = gc.dims_of(case)
    full = gu.make_params("M2_info", dims, gc.PARAM_SEED)
    params = {k[len(_PREFIX):]: v for k, v in full.items() if k.startswith((_PREFIX + "encoder.", _PREFIX + "decoder."))}
    x, y, e = gu.make_batch(dims, B, gc.BATCH_SEED)
    for a in list(params.values()) + [x, y, e]:
        a.setflags(write=False)
    return params, x, y, e


def forward(p, x, y, e):
    return vo.m2v3_forward(p, x, y, e, prefix="")


def backward(p, enc, dec, z, g_r, g_z, g_mu, g_lv):
    """module_generic_cases.backward, and "g_y": the label columns of the decoder's input gradient"""
    grads = mg.backward(p, enc, dec, z, g_r, g_z, g_mu, g_lv)
    da = np.zeros_like(dec["r"]) if g_r is None else g_r * dec["r"]
    grads[GY] = vo.decoder_bwd(p, {}, "decoder.", dec, da)[:, z:]
    return grads


def run(case, params, x, y, e, upstreams, dtype=np.float64, hook=None, back=backward, fwd=forward):
    """-> (outputs, {key: the 14 gradients and g_y}): one forward in `dtype` under `hook`, one backward per entry of `upstreams`; float64
    arrays out.  back / fwd: the compositions (the CPU test seeds faults through them)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    p = {k: c(v) for k, v in params.items()}
    with (vo.gemm_hook(hook) if hook is not None else contextlib.nullcontext()):
        enc, dec = fwd(p, c(x), c(y), c(e))
        out = {k: np.asarray(v, np.float64) for k, v in (("r", dec["r"]), ("a", dec["a"]), ("mu", enc["mu"]), ("lv", enc["lv"]), ("z", enc["z"]))}
        grads = {}
        for key, ups in upstreams.items():
            g = back(p, enc, dec, case[1], *(c(u) for u in ups))
            grads[key] = {k: np.asarray(g[k], np.float64).reshape(params[k].shape) for k in params}
            grads[key][GY] = np.asarray(g[GY], np.float64).reshape(x.shape[0], case[0])
    return out, grads


def grad_figures(grads, truth):
    """module_cases.grad_figures of the tensors in `grads` (g_y among them or not); with g_y also its tensor-level figure"""
    figs = mc.grad_figures(grads, {k: G for k, G in truth.items() if k in grads})
    if GY in grads:
        t = figs[GY]["tensor"]
        figs[GY_TENSOR] = dict(worst=t, median=t)
    return figs


class Reference:
    def __init__(self, case, B):
        self.case, self.B = tuple(case), B
        self.params, self.x, self.y, self.e = inputs(self.case, B)
        self.up = mg.make_upstream(B, case[1])
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
        return {key: mg.select(self.up, key) for key in self.keys}

    def run(self, dtype=np.float64, hook=None, back=backward, fwd=forward):
        return run(self.case, self.params, self.x, self.y, self.e, self.upstreams(), dtype, hook, back, fwd)

    def _figures(self, out, grads):
        return mc.output_figures(out, self.out), {key: grad_figures(g, self.truth[key]) for key, g in grads.items()}

    def check_outputs(self, got, label=""):
        """-> (failures, worst ratio to the bound, {name: ratio})"""
        return mc.check(mc.output_figures(got, self.out), got, self.out, self.out_fig, None, label)

    def check_grads(self, grads, key, label=""):
        """grads: the 14 gradients by name, with or without "g_y" """
        return mc.check(grad_figures(grads, self.truth[key]), grads, self.truth[key], self.grad_fig[key], None, label)


@functools.lru_cache(maxsize=None)
def reference(case, B):
    return Reference(case, B)

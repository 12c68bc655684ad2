"""The four train steps on row-strided and offset x / y (tests/strided_inputs.py: the layouts; tests/test_strided_inputs_cpu.py: what each
exposes) against float64 and against a packed twin.  Everything goes through the public trainers -- GenericTrainer, ClassifierTrainer,
InfoTrainer, trainer.Trainer, accumulate.AccumulatedStep --, every test builds fresh trainers and prints its worst figures before it
asserts.  Every view lies in a buffer that is NaN outside the view, so a read through the width instead of the stride, or from the wrong
base, is a NaN or another frame's value in the result.

Any-size steps (csrc/train_generic.hip, train_classifier.hip, train_info.hip): the cases of tests/grad_columns_generic.py at 1 and 50
frames and the accumulated 48 + 48 + 20.
  float64      grads_numpy() under grad_columns_generic.check (its bound, MARGIN 4, unchanged), the losses under the cases modules'
               LOSS_RTOL; std_norm under tests/std_norm_cases.py's bars.  The truth is the existing one: the values are the same.
  packed twin  same parameters, same noise, the packed arrays: losses, gradients, params, m, v and a following evaluate() are equal
               BIT FOR BIT.  Derived, not measured: these kernels have one load path (a guarded scalar or 16-byte load per element
               group), and a stride changes addresses only, never which values are loaded or the order of any sum.
Reference-geometry step (csrc/train_fused.hip and the rows / weight-gradient kernels behind it), fp32, bf16x3, bf16: the cases of
tests/grad_columns.py.
  float64      grad_columns.check unchanged; [ELBO, recon, KL] within the tolerance of test_fused_step_vs_oracle for the precision
               (LOSS_RTOL_FUSED, restated from there).
  packed twin  the largest gradient and loss differences are PRINTED, not asserted: a packed, aligned tile goes through the whole-tile
               loads and forms its log-sum from registers (rows_helper.inc), a strided one through load_rows_to_lds, which adds the
               same terms in another order -- loss bits may differ.  The gradients were not proven bit-identical from the code either
               (the 16-bit policies decide per tile whether a label lo plane is needed; the decision is made in the two paths'
               own code), so nothing is asserted about them here beyond the float64 bound.

MEASURED: see the end of this docstring.

Refused steps.  A batch whose rows overlap or repeat (expand(), an as_strided view with a row stride below the width) is refused by
_check_inputs of all four trainers with a ValueError BEFORE the step is counted; until this module the library refused it after
step_count and the shared version had moved, and every later Adam bias correction was off by one.  No test passes the library a
stride it would have to refuse: these are host checks.

MEASURED on the MI355X (94 tests, 7.3 s of wall time with the CPU references when the module runs alone, the slowest test 0.8 s; the
two column modules report 4.9 s and 13 s).  Worst ratio of a held figure to its column bound -- it does not depend on the layout:
every layout of a case returned the packed twin's bits, so the figures are those of tests/test_gpu_train_columns.py and
tests/test_gpu_fused_columns.py:
  M1 / M2      50 frames: 0.35 (3, 17, (129, 127))  0.30 (513, 128, (512, 512))  0.35 (1, 5, (48, 200))  0.28 (0, 32, (256, 64)), the same under
               ld+7, odd, shifted and column; one frame: 0.38  0.48  0.73  0.36; accumulated 0.27; losses <= 1.2e-7 of the truth
  classifier   50 frames: 0.26  0.26  0.26; one frame: 0.32  0.28  0.25; accumulated 0.38; losses <= 1.3e-5
  M2_info      50 frames: 0.32  0.37  0.61 at (1, 1, (1, 1)), (classifier, entropy) 0.40; one frame: 0.31  0.38  0.69; accumulated 0.30;
               losses <= 1.3e-5
  std_norm     losses 5.5e-8 / 4.2e-8, gradients 3.4e-6 / 2.0e-6 of a tensor's maximum at the two geometries, both layouts
  Trainer      fp32 / bf16x3 / bf16 -- M2 y 513 at 33 frames 0.36 / 0.56 / 0.28 (all three layout pairs), at one frame 0.88 / 0.50 / 0.34,
               M2 y 1 at 1000 0.30 / 0.52 / 0.37, speech-like M1 at 1000 0.32 / 0.41 / 0.30, M2_info at 1000 0.52 / 0.88 / 0.27; rows= at
               237 -> 200 frames: M2 fp32 0.27, bf16 0.31, M2_info fp32 0.50.  Losses against float64: fp32 <= 5.9e-8, bf16x3 <= 2.0e-6
               (the one-frame case; 2.6e-7 elsewhere), bf16 <= 1.8e-4
  Trainer against its packed twin (printed, not held): in all 33 runs NO gradient element and NO loss scalar differed by a bit.
No NaN reached a result anywhere: no kernel's result depends on memory outside the view.

Scratch breakages of csrc/train_generic.hip and train_tables.hip (one at a time in a scratch copy, each only SHRINKS a stride, so every read stays inside
the tensor's allocation; nothing of them committed; this module run once against each library):
  a  `513` in place of `g.ldx` in the raw-x re-read of the std_norm output layer (train_generic_rows_kernel)
       4 of 94 fail: the four std_norm tests, and nothing else -- as expected.
  b  `m.y_w` in place of `g.ldy` for the label block of train_generic_wgrad_kernel
       20 of 94 fail: every M1 / M2 and M2_info test with more than one frame, a y whose ld is not its width (ld+7, odd, column) and a
       label block -- 10 one-step cases, 4 rows= cases, 2 accumulated, 2 clipped, the 2 std_norm cases with an `odd` y.  What passes
       is what must: M1, the classifier (its weight gradients have no label block), M2_info fed by its classifier, every one-frame
       case, every `shifted` y (ld == w) -- as expected.
  No test from before this module passes a train step anything but a packed tensor, where ldx == 513 and ldy == y_dim: both faults
  leave every address they compute unchanged there, so no earlier test can fail on either library (reasoned from that; they were not
  run against the two libraries).
The raw-input path: 77 801 (bf16x3) / 44 011 (bf16) workspace bytes are non-zero with the stash and zero without, none the other way.
The parent commit's wrappers on `x[:1].expand(50, 513)`, run once: all four raise RuntimeError from the library ("leading dimension of
x 0", the reference-geometry step "bad argument") and report step_count == 1 afterwards -- the refusal test fails there.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import golden_util as gu
import grad_columns as gcol
import grad_columns_generic as gg
import std_norm_cases as sc
import strided_inputs as S
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic
import train_info_modes_cases as mc
from oracle import vae_oracle as vo

pytestmark = pytest.mark.gpu
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")
N = importlib.import_module("disentangled-vae_amd.native")

DEV = "cuda:0"
LR = 1e-4
MODS = {"generic": gc, "clf": cc, "info": ic}
PRETRAIN = ("classifier", "entropy")
LOSS_RTOL_FUSED = {"fp32": 1e-4, "bf16x3": 1e-5, "bf16": 2e-3}         # tests/test_gpu_fused.py: test_fused_step_vs_oracle (ltol)


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------

def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only)


def _view(a, name, kind="x"):
    """a (packed numpy [n, w]) on the device in layout `name`; None stays None."""
    if a is None:
        return None
    v = S.on_device(S.layout(a, name), DEV)
    shape, ld, off = S.geometry(name, *a.shape)
    assert v.stride() == (ld, 1) and v.storage_offset() == off and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _state(tr):
    """losses, gradients, params, m, v of a trainer, as numpy"""
    out = {"losses": tr.losses.cpu().numpy().copy(), "params": tr.params.cpu().numpy(), "m": tr.m.cpu().numpy(), "v": tr.v.cpu().numpy()}
    out.update({"grad " + k: v for k, v in tr.grads_numpy().items()})
    return out


def _assert_same_bits(a, b, what):
    assert set(a) == set(b)
    diff = {k: int(np.count_nonzero(_bits(a[k]) != _bits(b[k]))) for k in a}
    diff = {k: n for k, n in diff.items() if n}
    assert not diff, (what, "elements that differ", diff)


def _any_trainer(kind, case, mode, B, ksplit=1, params=None, **kw):
    if kind == "generic":
        return G.GenericTrainer(gc.model_of(case), gc.dims_of(case), params if params is not None else gc.inputs(case, 1)[0], batch=B,
                                device=DEV, lr=LR, ksplit=ksplit, **kw)
    if kind == "clf":
        return C.ClassifierTrainer(cc.dims_of(case), params=params if params is not None else cc.params_of(case), batch=B, device=DEV, lr=LR,
                                   ksplit=ksplit, **kw)
    a, b, g = ic.WEIGHTS
    mode = mode or gg.DEFAULT_MODE
    return I.InfoTrainer(ic.dims_of(case), params=params if params is not None else ic.params_of(case), batch=B, device=DEV, lr=LR, alpha=a,
                         beta=b, gamma=g, ksplit=ksplit, dec_label=mode[0], aux_enc=mode[1], **kw)


def _args(kind, x, y, e):
    return (x, y) if kind == "clf" else (x, y, e)


def _loss_error(kind, case, mode, B, losses):
    """(worst relative loss error against the float64 truth, its bar)"""
    if kind == "info" and mode not in (None, gg.DEFAULT_MODE):
        return mc.loss_err(losses, mc.truth(case, B, tuple(mode))[0][0], mc.by_terms(case, mode, B)), ic.LOSS_RTOL
    m = MODS[kind]
    return m.loss_err(losses if kind != "clf" else losses[0], m.truth(case, B)[0][0]), m.LOSS_RTOL


def _hold_columns(grads, ref, label):
    assert set(grads) == set(ref.truth)
    fails, top = gg.check(grads, ref, label=label)
    assert np.isfinite(top)
    assert not fails, fails
    return top


def _lay(xl, yl):
    return f"x:{xl}-y:{yl}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the any-size steps: one step, float64 and the packed twin
# ---------------------------------------------------------------------------------------------------------------------------------

_G3, _G513, _G1, _G0 = (3, 17, (129, 127)), (513, 128, (512, 512)), (1, 5, (48, 200)), (0, 32, (256, 64))
_C17, _C513, _C2 = ((129, 127), 17), ((512, 512), 513), ((48, 200), 2)
_I3, _I513, _I1 = (3, 17, (129, 127)), (513, 128, (512, 512)), (1, 1, (1, 1))
# (kind, case, mode, B, x layout, y layout): at 50 frames every x layout and every y layout (`column` where y_dim is 1, 3 or 17) with
# every kind, x and y both strided wherever there is a y; at one frame no stride is used, only the base: one pairing per case
ONE_STEP = [
    ("generic", _G3, None, 50, "odd", "shifted"), ("generic", _G3, None, 50, "ld+7", "column"),
    ("generic", _G513, None, 50, "ld+7", "ld+7"), ("generic", _G513, None, 50, "shifted", "odd"),
    ("generic", _G1, None, 50, "shifted", "column"), ("generic", _G1, None, 50, "odd", "ld+7"),
    ("generic", _G0, None, 50, "odd", None), ("generic", _G0, None, 50, "ld+7", None),
    ("generic", _G3, None, 1, "ld+7", "column"), ("generic", _G513, None, 1, "shifted", "odd"),
    ("generic", _G1, None, 1, "odd", "shifted"), ("generic", _G0, None, 1, "shifted", None),
    ("clf", _C17, None, 50, "ld+7", "column"), ("clf", _C17, None, 50, "odd", "shifted"),
    ("clf", _C513, None, 50, "shifted", "ld+7"), ("clf", _C513, None, 50, "ld+7", "odd"),
    ("clf", _C2, None, 50, "odd", "odd"), ("clf", _C2, None, 50, "shifted", "shifted"),
    ("clf", _C17, None, 1, "shifted", "odd"), ("clf", _C513, None, 1, "odd", "shifted"), ("clf", _C2, None, 1, "ld+7", "ld+7"),
    ("info", _I3, gg.DEFAULT_MODE, 50, "odd", "column"), ("info", _I3, gg.DEFAULT_MODE, 50, "ld+7", "shifted"),
    ("info", _I513, gg.DEFAULT_MODE, 50, "shifted", "ld+7"), ("info", _I513, gg.DEFAULT_MODE, 50, "odd", "odd"),
    ("info", _I1, gg.DEFAULT_MODE, 50, "ld+7", "column"), ("info", _I1, gg.DEFAULT_MODE, 50, "shifted", "odd"),
    ("info", _I3, PRETRAIN, 50, "odd", "ld+7"),
    ("info", _I3, gg.DEFAULT_MODE, 1, "shifted", "column"), ("info", _I513, gg.DEFAULT_MODE, 1, "ld+7", "shifted"),
    ("info", _I1, gg.DEFAULT_MODE, 1, "odd", "odd"),
]


def _one_step_id(c):
    kind, case, mode, B, xl, yl = c
    return gg.case_label(kind, case, mode, B, 1).replace(" ", "-") + "-" + _lay(xl, yl)


def test_the_one_step_cases_cover_every_layout_with_every_kind():
    for kind in MODS:
        at50 = [c for c in ONE_STEP if c[0] == kind and c[3] == 50]
        assert {c[4] for c in at50} == set(S.X_LAYOUTS), kind
        assert {c[5] for c in at50} - {None} == set(S.X_LAYOUTS) | {"column"}, kind
        assert any(c[4] != "packed" and c[5] not in (None, "packed") for c in at50)


@pytest.mark.parametrize("c", ONE_STEP, ids=_one_step_id)
def test_one_step_on_strided_inputs(c):
    kind, case, mode, B, xl, yl = c
    ref = gg.reference(kind, case, mode, B, 1)
    label = f"{ref.label} {_lay(xl, yl)}"
    x, y = _view(ref.x, xl), _view(ref.y, yl, "y")
    e = _dev(ref.e)
    tr = _any_trainer(kind, case, mode, B, params=ref.params)
    losses = tr.step(*_args(kind, x, y, e)).cpu().numpy().copy()
    got = _state(tr)
    top = _hold_columns(tr.grads_numpy(), ref, label)
    le, bar = _loss_error(kind, case, mode, B, losses)
    print(f"[{label}] worst ratio to the column bound {top:.3f}, losses {le:.2e} of the truth (bar {bar:.0e})")
    assert np.all(np.isfinite(losses)) and le <= bar
    twin = _any_trainer(kind, case, mode, B, params=ref.params)
    twin.step(*_args(kind, _dev(ref.x), _dev(ref.y), e))
    _assert_same_bits(got, _state(twin), label)
    ev = tr.evaluate(*_args(kind, x, y, e)).cpu().numpy()
    ev_twin = twin.evaluate(*_args(kind, _dev(ref.x), _dev(ref.y), e)).cpu().numpy()
    assert np.all(np.isfinite(ev)) and np.array_equal(_bits(ev), _bits(ev_twin)), (label, ev, ev_twin)
    assert tr.bad_row_count() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the any-size steps: rows= on strided stores
# ---------------------------------------------------------------------------------------------------------------------------------

GATHER = [("generic", _G3, "ld+7", "odd"), ("generic", _G1, "odd", "column"), ("clf", _C17, "odd", "ld+7"), ("clf", _C17, "ld+7", "column"),
          ("info", _I3, "ld+7", "odd"), ("info", _I1, "odd", "column")]


@pytest.mark.parametrize("kind,case,xl,yl", GATHER, ids=[f"{k}-{MODS[k].case_id(c)}-{_lay(a, b)}" for k, c, a, b in GATHER])
def test_gather_from_strided_stores(kind, case, xl, yl):
    """rows= on strided x and y stores of B + 37 frames: the bits of the packed twin stepped on X[rows].contiguous() (as test_gather of
    the three steps does for packed stores); then one index equal to n: the frame is trained on row 0 and counted once."""
    B = 50
    n = B + S.EXTRA_ROWS
    pool = MODS[kind].inputs(case, n)
    px, py = pool[1], pool[2]
    e = None if kind == "clf" else _dev(pool[3][:B])
    rows = S.gather_rows(n, B)
    sx, sy = _view(px[:n], xl), _view(py[:n], yl, "y")
    assert sx.shape[0] == n and sx.stride(0) != 513 and sy.stride(0) != py.shape[1]
    perm = torch.from_numpy(rows).to(DEV)
    a, b = _any_trainer(kind, case, None, B), _any_trainer(kind, case, None, B)
    a.step(*_args(kind, sx, sy, e), rows=perm)
    b.step(*_args(kind, _dev(px[rows]), _dev(py[rows]), e))
    assert a.bad_row_count() == 0
    _assert_same_bits(_state(a), _state(b), "gather")
    bad, fixed = rows.copy(), rows.copy()
    bad[7], fixed[7] = n, 0
    a, b = _any_trainer(kind, case, None, B), _any_trainer(kind, case, None, B)
    a.step(*_args(kind, sx, sy, e), rows=torch.from_numpy(bad).to(DEV))
    b.step(*_args(kind, _dev(px[fixed]), _dev(py[fixed]), e))
    assert a.bad_row_count() == 1 and a.bad_row_count() == 0 and b.bad_row_count() == 0
    _assert_same_bits(_state(a), _state(b), "gather, one index past the store")


# ---------------------------------------------------------------------------------------------------------------------------------
# the any-size steps: accumulation, clipping, std_norm, a Fortran-ordered x
# ---------------------------------------------------------------------------------------------------------------------------------

MICRO_LAYOUTS = [("ld+7", "odd"), ("odd", "shifted"), ("shifted", "ld+7")]


@pytest.mark.parametrize("case", gg.ACCUMULATED_CASES, ids=lambda c: gg.case_label(*c).replace(" ", "-"))
def test_accumulated_step_on_strided_micro_batches(case):
    """48 + 48 + 20 frames, the last micro-batch on a fork, each micro-batch a strided view in another layout: acc.grads_numpy()
    under the column bound of all 116 frames."""
    ref = gg.reference(*case)
    kind, cs, mode = case[:3]
    tr = _any_trainer(kind, cs, mode, 48, 0, params=ref.params)
    tail = tr.fork(20)
    assert [(t.plan.slice_frames, t.plan.ksplit) for t in (tr, tr, tail)] == ref.plans
    acc = A.AccumulatedStep(tr, micro_batches=list(gg.MICRO))
    for (lo, hi), (xl, yl), t in zip(((0, 48), (48, 96), (96, 116)), MICRO_LAYOUTS, (None, None, tail)):
        x, y = _view(ref.x[lo:hi], xl), _view(ref.y[lo:hi], yl, "y")
        e = None if ref.e is None else _dev(ref.e[lo:hi])
        acc.micro(*_args(kind, x, y, e), trainer=t)
    losses = acc.apply().cpu().numpy()
    assert np.all(np.isfinite(losses)) and tr.step_count == tail.step_count == 1
    top = _hold_columns(acc.grads_numpy(), ref, ref.label + " strided micro-batches")
    print(f"[{ref.label} strided micro-batches] worst ratio to the column bound {top:.3f}")


KIND_CASES = [("generic", _G3), ("clf", _C17), ("info", _I3)]


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=[k for k, _ in KIND_CASES])
def test_clipped_step_on_odd_inputs(kind, case):
    """max_norm = a tenth of the packed twin's total norm: the clipped step on `odd` x and y equals the packed twin's bit for bit,
    grad_norm included."""
    B = 50
    ref = gg.reference(kind, case, gg.DEFAULT_MODE if kind == "info" else None, B, 1)
    e = _dev(ref.e)
    packed = _args(kind, _dev(ref.x), _dev(ref.y), e)
    probe = _any_trainer(kind, case, None, B, params=ref.params)
    probe.step(*packed, max_norm=1.0)
    total = float(probe.grad_norm.cpu().numpy()[0])
    assert np.isfinite(total) and total > 0
    max_norm = 0.1 * total
    twin = _any_trainer(kind, case, None, B, params=ref.params)
    twin.step(*packed, max_norm=max_norm)
    tr = _any_trainer(kind, case, None, B, params=ref.params)
    tr.step(*_args(kind, _view(ref.x, "odd"), _view(ref.y, "odd", "y"), e), max_norm=max_norm)
    gn, gn_twin = tr.grad_norm.cpu().numpy(), twin.grad_norm.cpu().numpy()
    print(f"[clipped {kind}] total norm {gn[0]:.6e}, coefficient {gn[1]:.6e}")
    assert np.array_equal(_bits(gn), _bits(gn_twin)) and gn[0] == np.float32(total) and 0 < gn[1] < 0.11
    a, b = _state(tr), _state(twin)
    a["flat"], b["flat"] = tr._shared["clip"]["flat"].cpu().numpy(), twin._shared["clip"]["flat"].cpu().numpy()
    _assert_same_bits(a, b, "clipped")
    assert tr.skipped_step_count() == 0 and tr.step_count == 1


@pytest.mark.parametrize("xl,yl", [("ld+7", "shifted"), ("odd", "odd")], ids=lambda v: v)
@pytest.mark.parametrize("case", [_G3, _G513], ids=gc.case_id)
def test_std_norm_rereads_the_raw_x_through_the_stride(case, xl, yl):
    """GenericTrainer(std_norm=...): the output layer scores against the raw x, read a second time from the caller's tensor (the only
    route to that read site).  Held as tests/test_gpu_train_std_norm.py holds its one-step float64 case, and to the packed twin's bits."""
    B = 50
    params, x, y, eps = gc.inputs(case, B)
    make = lambda: T.make_trainer(gc.model_of(case), gc.dims_of(case), generic=True, params=params, batch=B, device=DEV, std_norm=sc.stats(case),
                                  norm_eps=sc.NORM_EPS, lr=LR)
    tr = make()
    assert isinstance(tr, G.GenericTrainer) and tr.plan.std_norm == 1
    xs, ys, e = _view(x, xl), _view(y, yl, "y"), _dev(eps)
    losses = tr.step(xs, ys, e).cpu().numpy().copy()
    l64, g64, _ = sc.truth(case, B)
    le, (ge, name) = gc.loss_err(losses, l64[0]), gc.grad_err(tr.grads_numpy(), g64[0])
    print(f"[std_norm {gc.case_id(case)} {_lay(xl, yl)}] losses {le:.2e}, gradients {ge:.2e} ({name})")
    assert le <= sc.LOSS_RTOL and ge <= sc.GRAD_TOL, (le, ge, name)
    twin = make()
    twin.step(_dev(x), _dev(y), e)
    _assert_same_bits(_state(tr), _state(twin), "std_norm")
    assert np.array_equal(_bits(tr.evaluate(xs, ys, e).cpu().numpy()), _bits(twin.evaluate(_dev(x), _dev(y), e).cpu().numpy()))


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=[k for k, _ in KIND_CASES])
def test_fortran_ordered_x_is_copied_and_steps_like_the_packed_one(kind, case):
    B = 50
    ref = gg.reference(kind, case, gg.DEFAULT_MODE if kind == "info" else None, B, 1)
    e = _dev(ref.e)
    xf = _dev(ref.x).t().contiguous().t()
    assert tuple(xf.shape) == (B, 513) and xf.stride() == (1, B)
    tr, twin = _any_trainer(kind, case, None, B, params=ref.params), _any_trainer(kind, case, None, B, params=ref.params)
    tr.step(*_args(kind, xf, _dev(ref.y), e))
    twin.step(*_args(kind, _dev(ref.x), _dev(ref.y), e))
    _assert_same_bits(_state(tr), _state(twin), "Fortran-ordered x")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference-geometry Trainer
# ---------------------------------------------------------------------------------------------------------------------------------

PRECISIONS = ["fp32", "bf16x3", "bf16"]
FUSED = [(("bench", "M2", 513, 33), "ld+7", "shifted"), (("bench", "M2", 513, 33), "odd", "ld+7"), (("bench", "M2", 513, 33), "shifted", "odd"),
         (("bench", "M2", 513, 1), "shifted", "ld+7"),
         (("bench", "M2", 1, 1000), "ld+7", "column"), (("bench", "M2", 1, 1000), "odd", "odd"),
         (("speech", "M1", 0, 1000), "odd", None), (("speech", "M1", 0, 1000), "shifted", None), (("speech", "M1", 0, 1000), "ld+7", None),
         (("info", "M2_info", 1, 1000), "shifted", "column"), (("info", "M2_info", 1, 1000), "ld+7", "odd")]


def _fused_trainer(r, precision, **kw):
    info = dict(zip(("alpha", "beta", "gamma"), gcol.INFO_WEIGHTS)) if r.model == "M2_info" else {}
    return T.Trainer(r.model, r.dims, r.params, batch=r.B, precision=precision, **info, **kw)


def _losses64(model, params, x, y, e):
    """[ELBO, recon, KL] of the float64 oracle (M2_info: its first three loss scalars are these)."""
    c = lambda a: None if a is None else np.asarray(a, np.float64)
    p = {k: c(v) for k, v in params.items()}
    if model == "M2_info":
        a, b, g = gcol.INFO_WEIGHTS
        out = vo.m2info_losses_and_grads(p, c(x), c(y), c(e), a, b, g)[0]
        return np.array([out["ELBO"], out["recon"], out["kl"]])
    out = vo.vae_loss_and_grads(model, p, c(x), c(y), c(e))[0]
    return np.array([out["loss"], out["recon"], out["kl"]])


@functools.lru_cache(maxsize=None)
def _fused_losses64(family, model, y_dim, B):
    r = gcol.reference(family, model, y_dim, B)
    return _losses64(model, r.params, r.x, r.y, r.e)


def _hold_fused(tr, losses, r, precision, want_losses, label):
    g = tr.grads_numpy()
    assert set(g) == set(r.truth)
    fails, top = gcol.check(g, r, precision, label=f"[{label}]")
    le = float(np.max(np.abs(losses[:3].astype(np.float64) - want_losses) / np.abs(want_losses)))
    print(f"[{label}] worst ratio to the column bound {top:.3f}, losses {le:.2e} of the truth (bar {LOSS_RTOL_FUSED[precision]:.0e})")
    assert np.all(np.isfinite(losses))
    np.testing.assert_allclose(losses[:3], want_losses, rtol=LOSS_RTOL_FUSED[precision])
    assert not fails, fails
    return top


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", FUSED, ids=["{}-{}-y{}-B{}-".format(*c[0]) + _lay(c[1], c[2]) for c in FUSED])
def test_fused_step_on_strided_inputs(c, precision):
    """Strided x never meets the whole-tile condition (ld == 513 and a 16-byte aligned base), so every tile goes through
    load_rows_to_lds, xt_issue, xstash_reload and the single reads of bin 512: `shifted` is dense but misaligned, `ld+7` aligned but
    padded, `odd` neither."""
    key, xl, yl = c
    r = gcol.reference(*key)
    label = "{} {} y{} B{} ".format(*key) + f"{precision} {_lay(xl, yl)}"
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)
    x, y, e = _view(r.x, xl), _view(r.y, yl, "y"), t(r.e)
    tr = _fused_trainer(r, precision)
    losses = tr.step(x, y, e).cpu().numpy().copy()
    _hold_fused(tr, losses, r, precision, _fused_losses64(*key), label)
    twin = _fused_trainer(r, precision)
    tl = twin.step(t(r.x), t(r.y), e).cpu().numpy()
    g, gt = tr.grads_numpy(), twin.grads_numpy()
    gd = max(float(np.max(np.abs(g[k].astype(np.float64) - gt[k])) / (np.max(np.abs(gt[k])) + 1e-300)) for k in g)
    nd = sum(int(np.count_nonzero(_bits(g[k]) != _bits(gt[k]))) for k in g)
    ld = float(np.max(np.abs(losses.astype(np.float64) - tl) / (np.abs(tl.astype(np.float64)) + 1e-300)))
    print(f"[{label}] against the packed twin (printed, not held): gradients {gd:.2e} of a tensor's maximum ({nd} elements differ), losses {ld:.2e}")
    assert tr.bad_row_count() == 0


def _zeroed_workspace(tr):
    """The trainer's workspace replaced by one that starts from zeros and set up again (as test_kernels_stay_inside_their_buffers
    swaps in its guarded one)."""
    import ctypes
    tr.ws = torch.zeros(tr.plan.workspace_bytes, dtype=torch.uint8, device=DEV)
    go = tr.plan.grad_offset_bytes
    tr.flat_grad = tr.ws[go:go + 4 * tr.plan.n_params].view(torch.float32)
    N.check(tr.lib.dvae_train_init(ctypes.byref(tr.plan), N.ptr(tr.params), N.ptr(tr.ws), N.stream()), "dvae_train_init")


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_raw_input_weight_gradients_on_strided_x_and_labels(precision, monkeypatch):
    """The weight-gradient kernel's raw-input B tiles (train_wgrad.hip: rld) on strided x and strided 513-column labels, selected as
    test_weight_gradients_from_raw_inputs_equal_the_stash_path selects them.  That the path ran is asserted from the plan (the 8-wave
    rows kernel, no gather) and from the workspace: with raw inputs the rows kernel writes no x / label stash, so of two workspaces
    that started from zeros the raw one is still zero where the other holds the stash of x (every x of the bench family is positive:
    at least one non-zero byte per element and live frame) -- and the weight-gradient kernel, which then has nothing but the
    caller's tensors to read, meets the float64 bound and returns the stash path's bits."""
    key = ("bench", "M2", 513, 33)
    r = gcol.reference(*key)
    assert np.all(r.x > 0)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    x, y, e = _view(r.x, "odd"), _view(r.y, "shifted", "y"), t(r.e)
    monkeypatch.setenv("DVAE_WGRAD", "wg4")
    out, ws = {}, {}
    for raw in (False, True):
        if raw:
            monkeypatch.setenv("DVAE_RAW_INPUTS", "1")
        else:
            monkeypatch.delenv("DVAE_RAW_INPUTS", raising=False)
        tr = _fused_trainer(r, precision)
        assert tr.plan.rows_kernel == 2 and tr.plan.row_index == 0
        _zeroed_workspace(tr)
        losses = tr.step(x, y, e).cpu().numpy().copy()
        ws[raw] = tr.ws.clone()
        _hold_fused(tr, losses, r, precision, _fused_losses64(*key), "{} {} y{} B{} ".format(*key) + f"{precision} raw inputs {raw}")
        out[raw] = (losses, tr.grads_numpy())
    only_stash = int(((ws[False] != 0) & (ws[True] == 0)).sum().item())
    only_raw = int(((ws[True] != 0) & (ws[False] == 0)).sum().item())
    print(f"[raw inputs {precision}] workspace bytes non-zero with the stash and zero without: {only_stash}; the other way round: {only_raw}")
    assert only_stash >= 513 * r.B
    assert np.array_equal(_bits(out[False][0]), _bits(out[True][0]))
    for k in out[False][1]:
        assert np.array_equal(_bits(out[False][1][k]), _bits(out[True][1][k])), k


def _reference_on(model, dims, params, x, y, e):
    """grad_columns.Reference built by its own functions on given frames (the gathered batch of a rows= case)."""
    r = object.__new__(gcol.Reference)
    r.model, r.dims, r.params, r.x, r.y, r.e, r.B = model, dims, params, x, y, e, x.shape[0]
    a = (model, params, x, y, e)
    r.truth = gcol.oracle_grads(*a)
    r.restated = {"fp32": gcol.oracle_grads(*a, dtype=np.float32), "fp32 k-steps": gcol.oracle_grads(*a, dtype=np.float32, hook=gcol.KStepOrderF32())}
    for name, make in gcol.POLICIES.items():
        r.restated[name] = gcol.oracle_grads(*a, hook=make())
    r.draws = {p: {k: gcol.column_figures(g[k], r.truth[k]) for k in r.truth} for p, g in r.restated.items()}
    r.figures = {p: r.draws[p] for p in gcol.POLICIES}
    r.figures["fp32"] = {k: gcol.merge_figures(r.draws["fp32"][k], r.draws["fp32 k-steps"][k]) for k in r.truth}
    return r


@functools.lru_cache(maxsize=None)
def _gathered(model, y_dim, B):
    """(reference of the gathered batch, x store, y store, rows): n = B + 37 frames, the families of grad_columns.py (M2_info: the
    speech-like family / 64 with the gathered batch made tie-free, the replaced frames written back into the stores)."""
    n = B + S.EXTRA_ROWS
    family = "info" if model == "M2_info" else "bench"
    dims = gcol.dims_of(y_dim)
    ps, bs = gcol.SEEDS[family]
    params = gu.make_params(model, dims, ps)
    if family == "bench":
        x, y, e = gu.make_batch(dims, n, bs)
    else:
        x, y, e = gcol.make_speech_batch(dims, n, bs, 1.0 / 64)
    rows = S.gather_rows(n, B)
    xb, yb, eb = x[rows].copy(), y[rows].copy(), e[:B].copy()
    if model == "M2_info":
        replaced, margin = gcol.make_tie_free(params, xb, yb, eb)
        assert margin >= gcol.TIE_DELTA and replaced < B // 4
        x, y = x.copy(), y.copy()
        x[rows], y[rows] = xb, yb
    return _reference_on(model, dims, params, xb, yb, eb), x, y, rows


@pytest.mark.parametrize("model,y_dim,precision,xl,yl", [("M2", 513, "fp32", "ld+7", "odd"), ("M2", 513, "bf16", "odd", "shifted"),
                                                         ("M2_info", 1, "fp32", "shifted", "column")])
def test_fused_gather_from_strided_stores(model, y_dim, precision, xl, yl):
    B = 200
    r, x, y, rows = _gathered(model, y_dim, B)
    assert x.shape[0] == 237
    sx, sy, e = _view(x, xl), _view(y, yl, "y"), torch.from_numpy(np.array(r.e)).to(DEV)
    tr = _fused_trainer(r, precision)
    losses = tr.step(sx, sy, e, rows=torch.from_numpy(rows).to(DEV)).cpu().numpy().copy()
    _hold_fused(tr, losses, r, precision, _losses64(model, r.params, r.x, r.y, r.e), f"gather {model} y{y_dim} {precision} {_lay(xl, yl)}")
    assert tr.bad_row_count() == 0


def test_fused_evaluate_on_strided_inputs_matches_the_step_losses():
    """test_evaluate_is_forward_only_and_matches_step_losses on strided views: evaluate() leaves the parameters alone and returns the
    loss bits of the step that follows on the same views."""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 41)
    x, y, e = gu.make_batch(dims, 1000, 42)
    xs, ys, es = _view(x, "odd"), _view(y, "ld+7", "y"), torch.from_numpy(e).to(DEV)
    tr = T.Trainer("M2", dims, params, batch=1000, precision="fp32")
    before = tr.state_dict_numpy()
    ev = tr.evaluate(xs, ys, es).cpu().numpy()
    after = tr.state_dict_numpy()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    st = tr.step(xs, ys, es).cpu().numpy()
    assert np.all(np.isfinite(ev)) and np.array_equal(_bits(ev), _bits(st)), (ev, st)
    np.testing.assert_allclose(ev, _losses64("M2", params, x, y, e), rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------------
# refused steps (host checks: the library never sees these strides)
# ---------------------------------------------------------------------------------------------------------------------------------

def _refusal_setup(kind):
    """(make a trainer, packed x, packed y, noise or None, y_dim) at 50 frames"""
    B = 50
    if kind == "fused":
        dims = gcol.dims_of(513)
        params = gu.make_params("M2", dims, 11)
        x, y, e = gu.make_batch(dims, B, 12)
        return (lambda b=B: T.Trainer("M2", dims, params, batch=b, precision="fp32")), x, y, e, 513
    case = dict(KIND_CASES)[kind]
    p = MODS[kind].inputs(case, B)
    return (lambda b=B: _any_trainer(kind, case, None, b)), p[1], p[2], (None if kind == "clf" else p[3]), p[2].shape[1]


def _step(kind, tr, x, y, e):
    return tr.step(x, y) if kind == "clf" else tr.step(x, y, e)


@pytest.mark.parametrize("kind", ["generic", "clf", "info", "fused"])
def test_a_batch_of_overlapping_rows_is_refused_before_the_step_is_counted(kind):
    make, x, y, e, yd = _refusal_setup(kind)
    B = x.shape[0]
    X, Y, E = _dev(x), _dev(y), _dev(e)
    tr = make()
    snap = lambda: [t.clone() for t in (tr.params, tr.m, tr.v)]
    before = snap()
    flat = torch.cat([X.reshape(-1), X.reshape(-1)[:513]])
    bad_inputs = [(X[:1].expand(B, 513), Y, "x"),                                          # one frame, B times: stride 0
                  (flat.as_strided((B, 513), (512, 1)), Y, "x"),                           # rows that overlap by one element
                  (X, Y[:1].expand(B, yd), "y")]                                           # one label row, B times
    for bx, by, who in bad_inputs:
        assert (bx if who == "x" else by).stride(0) < (513 if who == "x" else yd)
        with pytest.raises(ValueError, match=r"row stride .*contiguous\(\)"):
            _step(kind, tr, bx, by, E)
        with pytest.raises(ValueError, match="row stride"):
            tr.evaluate(bx, by) if kind == "clf" else tr.evaluate(bx, by, E)
        assert tr.step_count == 0 and tr.bad_row_count() == 0
        assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    # the next good step is the first step of a fresh trainer: its bias correction is at t = 1
    _step(kind, tr, X, Y, E)
    fresh = make()
    _step(kind, fresh, X, Y, E)
    assert tr.step_count == fresh.step_count == 1
    _assert_same_bits(_state(tr), _state(fresh), "the step after a refusal")
    # one row has no stride: an expanded or strided [1, 513] x steps like its packed copy
    one, one_twin = make(1), make(1)
    x1 = X[:1].expand(1, 513).as_strided((1, 513), (0, 1))
    y1 = Y[:1].as_strided((1, yd), (3, 1))
    assert x1.stride(0) == 0 and y1.stride(0) == 3
    _step(kind, one, x1, y1, None if E is None else E[:1])
    _step(kind, one_twin, X[:1].clone(), Y[:1].clone(), None if E is None else E[:1])
    _assert_same_bits(_state(one), _state(one_twin), "one row")

"""tests/grad_columns_generic.py on the CPU: the float32 restatements against float64 on every case of tests/test_gpu_train_columns.py,
seeded faults of train_generic_wgrad_kernel's ragged paths (applied to a copy of the float64 truth) against the tensor-level bar of
the cases modules and against the per-column bound, the zero-column rule, and the kernels' summation order run in float64.

What the seeded faults show (figures: grad_err of the cases module, i.e. max |g - G| / max |G| over the tensor, bar 1e-4; every fault
below breaks the per-column bound by a factor of 500 or more):
    fault                                           generic (3, 17, (129, 127))   generic (513, 128, (512, 512))   M2_info
    1 label columns of encoder layer 1 x 1.01        4.9e-6  hides                 3.5e-6  hides                    --
    2 column 512 of an x-fed layer left zero         1.2e-5  hides                 2.1e-6  hides                    7.0e-5  hides  (1, 16, (128, 128))
    3 frame 7 missing from one 64-column block       5.2e-6  hides (block 0)       9.4e-7  hides (block 0)          7.2e-6  hides  (3, 17, (129, 127)), the ninth block
    4 the columns from in_w on shifted by one        4.7e-4  SEEN                  3.5e-4  SEEN                     2.3e-1  SEEN   (decoder layer 1)
Fault 4 does not hide anywhere: the first label column is never written and its neighbours hold another label's gradient, an error of
a whole label column, which is 3e-4 ... 3e-3 of the tensor's maximum on every generic case with labels (bench, speech-like and
real-valued labels alike).  It hides only 1 % of itself (fault 1).  test_faults_the_tensor_level_bar_sees asserts that, so that the
table stays true.  M2_info's encoder sees x alone; its label columns are those of decoder layer 1, the loudest of that tensor
(x 1.01: 3.0e-3, seen), and on its selected frames an unwritten column 512 of the encoder's layer 1 shows at tensor level at six of
the eight cases of train_info_cases.py (1.7e-4 ... 5.2e-3), (3, 17, (129, 127)) among them.
The classifier is the exception the other way round: on its selected inputs column 512 is loud enough that leaving it unwritten
already shows at tensor level (2.1e-3 at ((129, 127), 17), 2.8e-3 at ((512, 512), 513)), and so does its quietest column left unwritten
(1.6e-4).  The fault that hides there is the quietest live column of layer 1, chosen from the truth, x 1.01."""
import numpy as np
import pytest

import grad_columns_generic as gg
from oracle import vae_oracle as vo

GA, GB = (3, 17, (129, 127)), (513, 128, (512, 512))
W1 = "encoder.hidden.0.weight"
IW1, ID1, IC1 = "enc_dec_clf.encoder.hidden.0.weight", "enc_dec_clf.decoder.hidden.0.weight", "enc_dec_clf.classifier.hidden.0.weight"
GEN = lambda c: ("generic", c, None, 50, 1, "bench", None)
INF = lambda c: ("info", c, gg.DEFAULT_MODE, 50, 1, "bench", None)
FRAME = 7


def _id(v):
    return gg.case_label(*v).replace(" ", "-") if isinstance(v, tuple) and len(v) == 7 else None


# ---- restatements ----
@pytest.mark.parametrize("case", gg.ALL_CASES, ids=_id)
def test_restatements_stay_inside_their_own_bound(case):
    """Both orders of the float32 restatement hold the bound made from them; so does a second draw of each -- the same step on the
    frames in another order, i.e. other sums of the same terms (and other micro-batches of an accumulated step); and no column or row
    that is zero in float64 is anything but +0.0 in a restatement."""
    r = gg.reference(*case)
    for order in gg.ORDERS:
        fails, top = gg.check(r.restated[order], r, label=f"{r.label} {order}", quiet=True)
        assert not fails and top <= 1 / gg.MARGIN + 1e-12, (order, fails, top)
    perm = np.random.default_rng(5).permutation(case[3])
    for order in gg.ORDERS:
        fails, top = gg.check(r.restate(order, perm), r, quiet=True)
        print(f"{r.label} {order}, frames permuted: worst ratio to the bound {top:.3f}")
        assert not fails, (order, fails)


def test_the_kernels_order_is_live_and_follows_the_plan():
    """slice_plan restates choose_slices; the k-steps order differs from numpy's in float32, and four slices differ from one."""
    assert gg.slice_plan(50, 4) == (16, 4) and gg.slice_plan(50, 1) == (64, 1) and gg.slice_plan(1, 1) == (16, 1)
    assert gg.slice_plan(48, 0) == (48, 1) and gg.slice_plan(20, 0) == (32, 1) and gg.slice_plan(116, 16) == (16, 8)
    one, four = gg.reference(*GEN(GA)), gg.reference("generic", GA, None, 50, 4, "bench", None)
    assert [min(16, 50 - f) for f in range(0, 50, four.slice_frames)] == [16, 16, 16, 2]
    assert np.any(one.restated["numpy"][W1] != one.restated["k-steps"][W1])
    assert np.any(one.restated["k-steps"][W1] != four.restated["k-steps"][W1])
    for k in one.truth:                                 # the slices change the weight-gradient sums alone: same float64 truth
        assert np.array_equal(one.truth[k], four.truth[k])


@pytest.mark.parametrize("case", [GEN(GA), ("generic", GB, None, 50, 4, "bench", None), ("clf", ((129, 127), 17), None, 50, 4, "bench", None),
                                  INF(GA), ("info", GA, ("classifier", "entropy"), 50, 4, "bench", None)], ids=_id)
def test_the_hook_in_float64_changes_the_truth_by_float64_rounding(case):
    """gemm_hook(StepOrderF32) under float64 only reorders sums (there is no wider format to fuse in: steps of four terms).  The same
    hook under float32 is the same algorithm in the same order with a rounding unit 2^29 times larger, and to first order every
    rounding error scales with the unit: what that float32 run deviates by per column, times 2^-29 (and the margin of two draws),
    bounds the float64 run."""
    r = gg.reference(*case)
    frames = np.arange(case[3])
    unfused = lambda: gg.StepOrderF32(r.slice_frames, r.z_dim, fused=False)
    g, g32 = r.run(frames, np.float64, unfused()), r.run(frames, np.float32, unfused())
    worst = 0.0
    for k, G in r.truth.items():
        f = gg.column_figures(g[k], G)
        bw, _ = gg.bound(gg.column_figures(g32[k], G))
        worst = max(worst, f["worst"] / (bw * 2.0 ** -29))
        assert f["zero_ok"] and f["worst"] <= bw * 2.0 ** -29, (k, f["worst"], bw * 2.0 ** -29)
    print(f"{r.label}: the kernels' order in float64, worst column over (float32 bound x 2^-29): {worst:.3f}")
    assert vo._GEMM_HOOK is None


# ---- seeded faults ----
def _frame_part(r, f):
    """frame f's contribution to every gradient: a frame's term depends on that frame alone, so it is the mean over the B frames minus
    (B - 1) / B of the mean over the others (float64)"""
    B = r.key[3]
    rest = r.run(np.flatnonzero(np.arange(B) != f), np.float64)
    return {k: r.truth[k] - (B - 1) / B * rest[k] for k in r.truth}


def _seed(r, fault, k, in_w):
    g, G = r.truth_copy(), r.truth[k]
    if fault == "labels x 1.01":
        g[k][:, in_w:] *= 1.01
    elif fault == "column 512 zero":
        assert in_w == 513
        g[k][:, 512] = 0.0
    elif fault == "ocol + 1":
        g[k][:, in_w + 1:] = G[:, in_w:-1]
        g[k][:, in_w] = 0.0
    elif fault.startswith("frame missing from block "):
        b0 = 64 * int(fault.rsplit(" ", 1)[1])
        g[k][:, b0:b0 + 64] -= _frame_part(r, FRAME)[k][:, b0:b0 + 64]
    elif fault == "quietest column x 1.01":
        top = np.abs(G).max(axis=0)
        g[k][:, int(np.argmin(np.where(top > 0, top, np.inf)))] *= 1.01
    else:
        raise ValueError(fault)
    return g


def _verdicts(case, fault, k, in_w):
    r = gg.reference(*case)
    assert r.truth[k].shape[1] > (in_w if fault in ("labels x 1.01", "ocol + 1") else 512)
    g = _seed(r, fault, k, in_w)
    m = gg.MODS[case[0]]
    ge, name = m.grad_err(g, r.truth)
    fails, top = gg.check(g, r, quiet=True)
    print(f"{r.label}, {k}, {fault}: tensor-level {ge:.1e} ({name}; bar {m.GRAD_TOL:.0e}), {top:.0f} x the column bound, {len(fails)} failures: {fails[:2]}")
    return ge, m.GRAD_TOL, fails


HIDDEN = [(GEN(GA), "labels x 1.01", W1, 513), (GEN(GB), "labels x 1.01", W1, 513),
          (GEN(GA), "column 512 zero", W1, 513), (GEN(GB), "column 512 zero", W1, 513), (INF((1, 16, (128, 128))), "column 512 zero", IW1, 513),
          (GEN(GA), "frame missing from block 0", W1, 513), (GEN(GB), "frame missing from block 0", W1, 513),
          (INF(GA), "frame missing from block 8", IW1, 513), (INF(GA), "frame missing from block 8", IC1, 513),
          (("clf", ((129, 127), 17), None, 50, 1, "bench", None), "quietest column x 1.01", "hidden.0.weight", 513),
          (("clf", ((512, 512), 513), None, 50, 1, "bench", None), "quietest column x 1.01", "hidden.0.weight", 513)]
SEEN = [(GEN(GA), "ocol + 1", W1, 513), (GEN(GB), "ocol + 1", W1, 513), (("generic", GA, None, 50, 1, "real", None), "ocol + 1", W1, 513),
        (INF(GA), "ocol + 1", ID1, 17), (INF(GA), "labels x 1.01", ID1, 17), (INF(GA), "column 512 zero", IW1, 513),
        (("clf", ((129, 127), 17), None, 50, 1, "bench", None), "column 512 zero", "hidden.0.weight", 513),
        (("clf", ((512, 512), 513), None, 50, 1, "bench", None), "column 512 zero", "hidden.0.weight", 513)]
_fid = lambda v: _id(v) if isinstance(v, tuple) else (v.replace(" ", "-") if isinstance(v, str) else None)


@pytest.mark.parametrize("case,fault,k,in_w", HIDDEN, ids=_fid)
def test_faults_the_tensor_level_bar_cannot_see(case, fault, k, in_w):
    """Each passes grad_err <= GRAD_TOL of its cases module and fails the column bound."""
    ge, tol, fails = _verdicts(case, fault, k, in_w)
    assert ge <= tol, ge
    assert fails and all(name == k for name, _ in fails), fails


@pytest.mark.parametrize("case,fault,k,in_w", SEEN, ids=_fid)
def test_faults_the_tensor_level_bar_sees(case, fault, k, in_w):
    """The other half of the module docstring's table: these fail the column bound too, and grad_err already exceeds GRAD_TOL -- the
    ocol shift everywhere, decoder layer 1's label columns and an unwritten column 512 on M2_info's and the classifier's selected
    frames."""
    ge, tol, fails = _verdicts(case, fault, k, in_w)
    assert ge > tol, ge
    assert fails and all(name == k for name, _ in fails), fails


# ---- zero columns ----
ZERO_CASES = [(("generic", GA, None, 1, 1, "bench", None), W1, "a label that is 0 in the one frame"),
              (("generic", GB, None, 1, 1, "bench", None), W1, "y 513 at one frame"),
              (("generic", GB, None, 1, 1, "bench", None), "decoder.hidden.0.weight", "y 513 at one frame"),
              (("info", (1, 1, (1, 1)), gg.DEFAULT_MODE, 50, 1, "bench", None), None, "the dead unit")]


@pytest.mark.parametrize("case,k,what", ZERO_CASES, ids=_fid)
def test_a_zero_column_must_be_exactly_zero(case, k, what):
    r = gg.reference(*case)
    if k is None:                                       # the dead unit: some tensor of the auxiliary net is all zero
        dead = [n for n, G in r.truth.items() if not np.any(G)]
        assert dead and all(n.startswith("auxiliary.") for n in dead), dead
        k = [n for n in dead if gg.is_matrix(r.truth[n])][0]
        col = 0
    else:
        zero = np.flatnonzero(~np.any(r.truth[k], axis=0))
        live = np.flatnonzero(np.any(r.truth[k], axis=0))
        assert zero.size and live.size and zero.max() >= 513, (zero.size, live.size)          # label columns among them
        col = int(zero[-1])
    f = gg.column_figures(r.truth[k], r.truth[k])
    print(f"{r.label} {k} ({what}): {100 * f['zero_share']:.1f} % of the columns are identically zero")
    assert f["zero_share"] > 0
    assert gg.check(r.truth_copy(), r, quiet=True)[0] == []
    for v in (-0.0, 1e-30, -1e-30):
        g = r.truth_copy()
        g[k][0, col] = v
        fails, _ = gg.check(g, r, quiet=True)
        assert fails and all(name == k and "zero" in why for name, why in fails), (v, fails)
    g = r.truth_copy()
    g[k] = g[k].astype(np.float32)                      # what a trainer returns
    g[k][-1, col] = np.float32(-0.0)
    assert gg.check(g, r, quiet=True)[0]

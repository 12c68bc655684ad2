"""tests/later_steps.py on the CPU: the harness is sound, its premises hold on the cases of tests/test_gpu_train_later_steps.py, and what
the suite held before it is blind to a step that runs on the previous step's state.
1. reference_at on a case's own parameters and inputs IS grad_columns_generic.reference(...): truth, both restatements and every figure
   equal bit for bit (M2 in four slices, the classifier, its accumulated step, M2_info in two modes); the same for the alternate
   constructors of grad_columns.Reference, module_generic_cases.Reference; frames_at at a case's parameters is the case's own selection.
2. Three float32 oracle steps at lr 1e-3, another batch each (BATCH_SEED + k), m and v carried, on every case of the device test.  The
   ReLU nets find their B frames in the pool at every step's parameters (asserted inside frames_at), the float32 oracle stays at 0.20 ...
   0.25 of the column bound of reference_at of its own step, its losses within 0.41 of LOSS_RTOL, a step moves the median weight by
   1.0 ... 3.5 % (0 at the classifier's one-frame step 1, where most units are dead), and the float64 gradient at the PREVIOUS step's
   parameters lies, in column bounds (stale_ratio, steps 2 / 3):
     M2 (3, 17, (129, 127)) 9.6e3 / 3.8e3 (one and four slices)   (513, 128, (512, 512)) 3.0e4 / 1.8e4   (1, 5, (48, 200)) 1.1e4 / 1.6e3
     M1 (0, 32, (256, 64)) 1.5e4 / 6.9e3     M2 at one frame 387 / 1.4e4     std_norm 1.4e4 / 9.1e3, one frame 2.3e3 / 6.1e3
     classifier ((129, 127), 17) 4.7e4 / 2.8e4   ((512, 512), 513) 2.2e5 / 1.3e5   one frame 3.2e3 / 6.9e3
     M2_info (3, 17, (129, 127)) 2.5e4 / 3.0e4   (classifier, entropy) 2.4e4 / 2.6e4   one frame 7.5e3 / 1.9e4
   The smallest, 387, is held against STALE_MIN = 100.
3. Seeded faults, each the step-k float32 gradient or update with ONE thing left over from step k - 1, at steps 2 and 3 of M2 (3, 17,
   (129, 127)), the classifier ((129, 127), 17) and M2_info (3, 17, (129, 127)) at 50 frames.  Smallest excess over the bound:
     a  one weight tensor stale in the gradient computation (each in turn)      2.3e3   5.5e4   9.1e3   column bounds
     b  Adam with the bias corrections of step k - 1                            1.4e5   1.4e5   1.4e5   Adam bounds
     c  Adam with m not carried                                                 7.6e6   7.6e6   7.6e6
     d  Adam with v not carried                                                 3.7e11  1.2e12  1.6e12
4. What the suite held after step one before: the losses of a three-step trajectory on one batch under LOSS_RTOL, and the parameters
   within steps x lr on all but a share of the elements.  The same faults as float64 trajectories against the sound one:
     at lr 1e-6 (train_info_cases.LR_TRAJ, the rate of the M2_info trajectory tests) the stale layer-1 weight moves the losses of steps
     2 - 3 by 2.0e-5 / 4.8e-5 / 1.5e-5 (M2 / classifier / M2_info; the bar is 1e-4) and the parameters by at most 1.17 / 0.15 / 0.35 of
     steps x lr, 0.001 % of them by more than 1: unseen.  The Adam faults move the losses by 7.9e-6 ... 6.5e-5 on M2 and the classifier:
     unseen; on M2_info by 1.2e-4 ... 1.7e-4: its trajectory test does see them, by a fifth to two thirds of a bar, through the small
     loss differences among its seven scalars (printed, not asserted).
     at lr 1e-2 (LR_TRAJ of the M1 / M2 and classifier trajectory tests) every one of these faults moves the losses by 4e-2 or more:
     those two trajectory tests do see state that is not carried, on three loss scalars and without saying which state -- printed,
     not asserted.  What no trajectory can hold is the size of the deviation: Adam is sign-like, so a sound float32 run leaves the float64
     trajectory as well, and the bar has to stay loose (1e-4 of a loss against the 2^-24-scale bounds of 2 and 3).
"""
import functools

import numpy as np
import pytest

import adam_bounds as ab
import grad_columns as gcol
import grad_columns_generic as gg
import later_steps as ls
import module_generic_cases as mg
import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic
from oracle import vae_oracle as vo

F32 = np.float32
ADAM = (0.9, 0.999, 1e-8)
_M2, _CLF, _INFO = (3, 17, (129, 127)), ((129, 127), 17), (3, 17, (129, 127))
# (kind, case, mode, B, ksplit): the cases of tests/test_gpu_train_later_steps.py
CASES = ([("generic", _M2, None, 50, 1), ("generic", _M2, None, 50, 4), ("generic", (513, 128, (512, 512)), None, 50, 1),
          ("generic", (1, 5, (48, 200)), None, 50, 1), ("generic", (0, 32, (256, 64)), None, 50, 1), ("generic", _M2, None, 1, 1),
          ("clf", _CLF, None, 50, 1), ("clf", ((512, 512), 513), None, 50, 1), ("clf", _CLF, None, 1, 1),
          ("info", _INFO, gg.DEFAULT_MODE, 50, 1), ("info", _INFO, ("classifier", "entropy"), 50, 1), ("info", _INFO, gg.DEFAULT_MODE, 1, 1),
          ("norm", _M2, None, 50, 1), ("norm", _M2, None, 1, 1)])
FAULT_CASES = [CASES[0], CASES[6], CASES[9]]              # one per kind, 50 frames


def _id(c):
    return ls.case_label(*c).replace(" ", "-")


def initial_params(kind, case):
    if kind == "clf":
        return cc.params_of(case)
    return ic.params_of(case) if kind == "info" else gc.inputs(case, 1)[0]


def unflat(vec, like):
    out, lo = {}, 0
    for k, v in like.items():
        out[k] = np.ascontiguousarray(vec[lo:lo + v.size].reshape(v.shape))
        lo += v.size
    return out


@functools.lru_cache(maxsize=None)
def f32_steps(kind, case, mode, B, ksplit, lr=ls.LR):
    """ls.STEPS float32 oracle steps at `lr`, another batch each step (BATCH_SEED + k; the ReLU nets' frames selected again at the
    parameters in force), m and v carried, the update by adam_bounds.emulate (the documented float32 order).  One dict per step."""
    params = initial_params(kind, case)
    n = sum(v.size for v in params.values())
    m, v, out = np.zeros(n, F32), np.zeros(n, F32), []
    for k in range(1, ls.STEPS + 1):
        x, y, e = ls.frames_at(kind, case, params, B, gc.BATCH_SEED + k)
        losses, g, _ = ls.oracle_step(kind, case, mode, params, x, y, e, F32)
        g = {t: a.astype(F32) for t, a in g.items()}
        p0 = ls.flat(params)
        p1, m1, v1 = ab.emulate(p0, m, v, ls.flat(g, params)[None, :], (k, lr) + ADAM)
        out.append(dict(k=k, params=params, batch=(x, y, e), losses=losses, grads=g, before=(p0, m, v), after=(p1, m1, v1)))
        params, m, v = unflat(p1, params), m1, v1
    return out


@functools.lru_cache(maxsize=None)
def ref_of_step(kind, case, mode, B, ksplit, k):
    s = f32_steps(kind, case, mode, B, ksplit)[k - 1]
    return ls.reference_at(kind, case, mode, s["params"], *s["batch"], ksplit)


# ---- 1. reference_at is the cases' own reference ----
def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, (path, a, b)


PIN_CASES = [("generic", _M2, None, 50, 4, "bench", None), ("clf", _CLF, None, 50, 1, "bench", None),
             ("clf", ((48, 200), 2), None, 116, 0, "bench", gg.MICRO), ("info", _INFO, gg.DEFAULT_MODE, 50, 1, "bench", None),
             ("info", _INFO, ("classifier", "entropy"), 50, 1, "bench", None)]


@pytest.mark.parametrize("case", PIN_CASES, ids=lambda c: gg.case_label(*c).replace(" ", "-"))
def test_reference_at_reproduces_the_reference_of_the_case_bit_for_bit(case):
    kind, c, mode, B, ksplit, _, micro = case
    want = gg.reference(*case)
    got = ls.reference_at(kind, c, mode, want.params, want.x, want.y, want.e, ksplit, micro)
    assert got.plans == want.plans and got.sizes == want.sizes and (got.slice_frames, got.nslices) == (want.slice_frames, want.nslices)
    for name in ("truth", "restated", "draws", "row_draws", "figures", "row_figures"):
        _same_tree(getattr(got, name), getattr(want, name), name)


def test_the_reference_size_and_module_references_take_given_inputs_bit_for_bit():
    want = gcol.reference("bench", "M2", 513, 33)
    got = gcol.Reference.at("M2", 513, want.params, want.x, want.y, want.e)
    for name in ("truth", "restated", "draws", "figures"):
        _same_tree(getattr(got, name), getattr(want, name), name)
    want = mg.reference((0, 32, (256, 64)), 50)
    got = mg.Reference.at(want.case, want.params, want.x, want.y, want.e, want.up, want.keys)
    assert (got.slice_frames, got.nslices) == (want.slice_frames, want.nslices)
    for name in ("out", "truth", "out_fig", "grad_fig"):
        _same_tree(getattr(got, name), getattr(want, name), name)


def test_frames_at_the_case_parameters_is_the_case_selection():
    for kind, case in (("clf", _CLF), ("info", _INFO)):
        mod = ls.CASES_MOD[kind]
        want = mod.inputs(case, 50)
        got = ls.frames_at(kind, case, want[0], 50, mod.BATCH_SEED)
        for a, b in zip(got, want[1:] + ((None,) if kind == "clf" else ())):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
    x, _ = cc.pool(_CLF, 50)
    assert np.array_equal(cc.frame_ok(_CLF, x), cc.frames_ok(cc.params_of(_CLF), x))


# ---- 2. three float32 steps: the premises of the device test, and the reference inside its own rule ----
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_three_float32_steps_stay_inside_the_rule_of_their_own_step(case):
    """frames_at asserts that B pool frames pass at every step's parameters (the ReLU nets); each step's float32 gradients pass check
    against reference_at of that step; from step 2 on the float64 gradient at the previous step's parameters lies at least
    STALE_MIN bounds away (the premise of the device test, from the oracle alone)."""
    kind, c, mode, B, ksplit = case
    steps = f32_steps(*case)
    for s in steps:
        k = s["k"]
        ref = ref_of_step(*case, k)
        fails, top = ls.check(s["grads"], ref, quiet=True)
        moved = np.abs(s["after"][0].astype(np.float64) - s["before"][0])
        lerr = ls.loss_err(kind, mode, s["losses"], ls.oracle_step(kind, c, mode, s["params"], *s["batch"])[0]) / ls.loss_rtol(kind)
        line = (f"[{_id(case)}] step {k}: float32 oracle at {top:.3f} of the bound, its losses at {lerr:.3f} of LOSS_RTOL; "
                f"median |dp| / |p| {np.median(moved / (np.abs(s['before'][0]) + 1e-30)):.3f}")
        stale = None
        if k >= 2:
            before = ls.oracle_step(kind, c, mode, steps[k - 2]["params"], *s["batch"])[1]
            stale = ls.stale_ratio(ref, before)
            line += f"; stale_ratio {stale:.3g}"
        print(line)
        assert not fails, fails
        assert lerr <= 1.0, lerr
        assert stale is None or stale >= ls.STALE_MIN, stale


# ---- 3. seeded faults: one thing left over from step k - 1 ----
def _weights(params):
    return [k for k in params if k.endswith("weight")]


@pytest.mark.parametrize("case", FAULT_CASES, ids=_id)
def test_a_stale_weight_tensor_exceeds_the_column_bound(case):
    """(a) the float32 gradient of step k with ONE weight tensor still that of step k - 1."""
    kind, c, mode, B, ksplit = case
    steps = f32_steps(*case)
    smallest = np.inf
    for k in (2, 3):
        s, ref = steps[k - 1], ref_of_step(*case, k)
        for name in _weights(s["params"]):
            p = dict(s["params"], **{name: steps[k - 2]["params"][name]})
            g = ls.oracle_step(kind, c, mode, p, *s["batch"], F32)[1]
            fails, top = ls.check(g, ref, quiet=True)
            smallest = min(smallest, top)
            assert fails and top > 1.0, (k, name, top)
    print(f"[{_id(case)}] a stale weight tensor: the smallest worst ratio to the bound over tensors and steps 2-3 is {smallest:.3g}")


EXEMPT = 0.06                          # the share of a tensor's elements golden_check's parameter rule leaves out, at its smallest
ADAM_FAULTS = ("bias corrections of step k - 1", "m not carried", "v not carried")


@pytest.mark.parametrize("case", FAULT_CASES, ids=_id)
def test_an_update_on_stale_adam_state_exceeds_the_adam_bounds(case):
    """(b) - (d) the float32 update of step k with the step number, m or v of a trainer that did not carry it."""
    steps = f32_steps(*case)
    for fault in ADAM_FAULTS:
        smallest = np.inf
        for k in (2, 3):
            s = steps[k - 1]
            p0, m0, v0 = s["before"]
            g = ls.flat(s["grads"], s["params"])
            hyper = (k, ls.LR) + ADAM
            ok = ls.adam_figures(p0, m0, v0, g, *s["after"], hyper)
            assert max(ok.values()) <= 1.0, ok                     # the sound update is inside
            t, m, v = k, m0, v0
            if fault == ADAM_FAULTS[0]:
                t = k - 1
            elif fault == ADAM_FAULTS[1]:
                m = np.zeros_like(m0)
            else:
                v = np.zeros_like(v0)
            got = ab.emulate(p0, m, v, g[None, :], (t, ls.LR) + ADAM)
            fig = ls.adam_figures(p0, m0, v0, g, *got, hyper)
            smallest = min(smallest, max(fig.values()))
            assert max(fig.values()) > 1.0 and fig["p"] > 1.0, (fault, k, fig)
        print(f"[{_id(case)}] {fault}: the smallest worst ratio to the Adam bounds over steps 2-3 is {smallest:.3g}")


# ---- 4. what the suite held before: the trajectory's losses and the parameters within steps x lr ----
def _f64_trajectory(kind, case, mode, params, batch, lr, fault=None, tensor=None):
    """STEPS float64 steps on ONE batch at `lr` (the trajectory tests' shape), Adam state carried; from step 2 on with `fault`."""
    p = {k: v.astype(np.float64) for k, v in params.items()}
    n = sum(v.size for v in p.values())
    m, v, losses, prev = np.zeros(n), np.zeros(n), [], None
    for k in range(1, ls.STEPS + 1):
        q = dict(p, **{tensor: prev[tensor]}) if (fault == "stale" and k >= 2) else p
        l, g, _ = ls.oracle_step(kind, case, mode, q, *batch)
        t, mm, vv = k, m, v
        if k >= 2 and fault == ADAM_FAULTS[0]:
            t = k - 1
        if k >= 2 and fault == ADAM_FAULTS[1]:
            mm = np.zeros(n)
        if k >= 2 and fault == ADAM_FAULTS[2]:
            vv = np.zeros(n)
        p1, m, v = vo.adam_step(ls.flat(p), ls.flat(g, p), mm, vv, t, lr, *ADAM)
        losses.append(l)
        prev, p = p, unflat(p1, p)
    return losses, ls.flat(p)


@pytest.mark.parametrize("case", FAULT_CASES, ids=_id)
def test_the_trajectory_and_parameter_checks_do_not_see_the_faults_at_1e_6(case):
    """Every fault above, run as a float64 trajectory of three steps on one batch at lr = 1e-6 (train_info_cases.LR_TRAJ, the rate of the
    M2_info trajectory tests): the losses of steps 2 - 3 stay within LOSS_RTOL of the sound trajectory's and the parameters within
    steps x lr of its on all but EXEMPT of the elements (Adam is sign-like: an element whose gradient is rounding noise moves by
    +-lr in either run) -- the two things held after step one before this module.  (The M1 / M2 and classifier trajectory tests run at
    1e-2; the figure at that rate is printed beside it and not asserted: there a trajectory does see most of these faults, on the
    loss scalars alone.)"""
    kind, c, mode, B, ksplit = case
    params = initial_params(kind, c)
    batch = ls.frames_at(kind, c, params, B, gc.BATCH_SEED)
    first = _weights(params)[0]
    for lr, held in ((ic.LR_TRAJ, True), (gc.LR_TRAJ, False)):
        sound_l, sound_p = _f64_trajectory(kind, c, mode, params, batch, lr)
        for fault, tensor in [("stale", first)] + [(f, None) for f in ADAM_FAULTS]:
            with np.errstate(all="ignore"):            # v not carried at 1e-2 throws the parameters far enough for exp to overflow
                l, p = _f64_trajectory(kind, c, mode, params, batch, lr, fault, tensor)
            err = max(ls.loss_err(kind, mode, l[k], sound_l[k]) for k in (1, 2))
            off = np.abs(p - sound_p) / (ls.STEPS * lr)
            dp, beyond = float(off.max()), float(np.mean(off > 1.0))
            name = f"{first} stale" if fault == "stale" else fault
            print(f"[{_id(case)}] lr {lr:g}, {name}: losses of steps 2-3 off by {err:.2e} (LOSS_RTOL {ls.loss_rtol(kind):g}), "
                  f"parameters off by at most {dp:.3f} of steps x lr, {100 * beyond:.3f} % of them by more than 1")
            if held and not (kind == "info" and fault in ADAM_FAULTS):
                assert err <= ls.loss_rtol(kind) and beyond <= EXEMPT, (fault, err, dp, beyond)

"""CPU (no GPU): the host side of the two options of the generic M2_info fused train step -- dvae_train_info_plan_mode
(include/dvae_train.h), trainer_info.mode_bits / make_plan / info_trainer_kind / make_info_trainer -- the numpy truth of
tests/train_info_modes_ref.py, and the premises of tests/test_gpu_train_info_modes.py: float32 arithmetic itself needs less than half of
the bars that test asserts, and the float64 trajectories keep enough cases whole at the learning rate chosen.  Every test prints its
worst figures before it asserts."""
import ctypes
import importlib

import numpy as np
import pytest

import golden_modes_cases as gmc
import golden_util as gu
import train_info_cases as ic
import train_info_modes_cases as mc
import train_info_modes_ref as mr
from oracle import vae_oracle as vo

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
I = importlib.import_module("disentangled-vae_amd.trainer_info")

E_BADARG = 1001
LDS_MAX = 160 * 1024
DEC_CLASSIFIER, AUX_UNIFORM, AUX_ENTROPY = 1, 2, 4      # include/dvae_train.h: DVAE_INFO_*
ALL_MODES = [0, AUX_UNIFORM, AUX_ENTROPY, DEC_CLASSIFIER, DEC_CLASSIFIER | AUX_UNIFORM, DEC_CLASSIFIER | AUX_ENTROPY]
REF = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))


def _plan_mode(case, B, mode, ksplit=0):
    y, z, (h1, h2) = case
    p = I.InfoPlan()
    rc = native.load().dvae_train_info_plan_mode(y, z, h1, h2, B, ksplit, mode, ctypes.byref(p))
    return rc, p


def _err():
    return native.load().dvae_last_error().decode()


def test_mode_0_is_the_plain_plan_field_for_field():
    for case in mc.CASES:
        for B, ks in [(1, 0), (50, 0), (8192, 0), (8192, 3)]:
            y, z, (h1, h2) = case
            a = I.InfoPlan()
            assert native.load().dvae_train_info_plan(y, z, h1, h2, B, ks, ctypes.byref(a)) == 0
            rc, b = _plan_mode(case, B, 0, ks)
            assert rc == 0 and bytes(a) == bytes(b) and b.info_mode == 0
            assert bytes(I.make_plan(ic.dims_of(case), B, ks)) == bytes(a)
            assert bytes(I.make_plan(ic.dims_of(case), B, ks, "truth", "bce")) == bytes(a)


def test_plans_of_every_mode():
    """Three launches and the LDS limit at every case, mode and batch; the tensors do not move with the mode, the workspace may."""
    worst = 0
    for case in mc.CASES + [(513, 128, (512, 512))]:
        for B in (1, 50, 8192):
            base = _plan_mode(case, B, 0)[1]
            for mode in ALL_MODES:
                rc, p = _plan_mode(case, B, mode)
                assert rc == 0, _err()
                worst = max(worst, p.lds_bytes)
                assert p.info_mode == mode and p.launches_per_step == 3 and p.n_tensors == 26 and p.lds_bytes <= LDS_MAX
                assert p.n_params == base.n_params and list(p.tensor_offset) == list(base.tensor_offset) and p.rows_grid == base.rows_grid
                assert p.workspace_bytes >= base.workspace_bytes and (not mode & DEC_CLASSIFIER or p.workspace_bytes > base.workspace_bytes)
                assert (p.info_alpha, p.info_beta, p.info_gamma) == (0.0, 10.0, 1.0)
    print(f"largest LDS request over the cases and modes: {worst} B of {LDS_MAX}")
    assert _plan_mode((513, 128, (512, 512)), 8192, DEC_CLASSIFIER | AUX_ENTROPY)[1].lds_bytes == _plan_mode((513, 128, (512, 512)), 8192, 0)[1].lds_bytes


def test_bad_mode_bits_are_refused_with_the_choices_named():
    for mode in (AUX_UNIFORM | AUX_ENTROPY, DEC_CLASSIFIER | AUX_UNIFORM | AUX_ENTROPY, 8, 16 | DEC_CLASSIFIER, -1):
        rc, _ = _plan_mode((1, 16, (128, 128)), 8, mode)
        msg = _err()
        print(f"mode {mode}: {rc} {msg}")
        assert rc == E_BADARG and all(w in msg for w in ("DVAE_INFO_DEC_CLASSIFIER", "DVAE_INFO_AUX_UNIFORM", "DVAE_INFO_AUX_ENTROPY"))
    # a plan whose mode was changed after planning is no plan: host check, nothing is launched
    rc, p = _plan_mode((3, 17, (129, 127)), 50, DEC_CLASSIFIER)
    assert rc == 0
    p.info_mode = AUX_UNIFORM | AUX_ENTROPY
    assert native.load().dvae_train_info_repack(ctypes.byref(p), None, None, None) == E_BADARG


def test_option_strings():
    assert I.mode_bits() == 0 and I.mode_bits("classifier", "entropy") == DEC_CLASSIFIER | AUX_ENTROPY
    assert I.mode_bits("truth", "uniform") == AUX_UNIFORM and I.mode_bits("classifier", "bce") == DEC_CLASSIFIER
    for kw in (dict(dec_label="soft"), dict(aux_enc="v3"), dict(dec_label=None), dict(aux_enc="")):
        for call in (lambda: I.mode_bits(**kw), lambda: I.make_plan(REF, 8, **kw), lambda: I.info_trainer_kind(REF, **kw),
                     lambda: I.make_info_trainer(REF, batch=8, **kw), lambda: I.InfoTrainer(REF, batch=8, **kw)):
            with pytest.raises(ValueError) as e:
                call()
            names = ("truth", "classifier") if "dec_label" in kw else ("bce", "uniform", "entropy")
            assert all(n in str(e.value) for n in names), str(e.value)


def test_routing():
    assert I.info_trainer_kind(REF) == "resident" and I.info_trainer_kind(REF, "truth", "bce") == "resident"
    for mode in mc.MODES:
        assert I.info_trainer_kind(REF, *mode) == "generic"
        assert I.info_trainer_kind(ic.dims_of((7, 16, (128, 128))), *mode) == "generic"
        assert I.info_trainer_kind(dict(REF, z_dim=129), *mode) is None
        for kw in (dict(precision="bf16x3"), dict(precision="bf16"), dict(world=2), dict(process_group=object())):
            with pytest.raises(NotImplementedError) as e:
                I.make_info_trainer(REF, dec_label=mode[0], aux_enc=mode[1], batch=8, **kw)
            assert "z_dim 1..128" in str(e.value) and "fp32" in str(e.value), str(e.value)
        with pytest.raises(NotImplementedError):
            I.make_info_trainer(dict(REF, z_dim=129), dec_label=mode[0], aux_enc=mode[1], batch=8)


def test_default_mode_truth_equals_the_oracle_bit_for_bit():
    for case in [(3, 17, (129, 127)), (1, 1, (1, 1)), (513, 64, (16, 16))]:
        for dtype in (np.float32, np.float64):
            a = ic.run(case, 50, dtype, steps=2)
            b = mc.run_on(*ic.inputs(case, 50), dtype, ("truth", "bce"), steps=2)
            for s in range(2):
                assert np.array_equal(a[0][s], b[0][s])
                assert set(a[1][s]) == set(b[1][s]) and all(np.array_equal(a[1][s][k], b[1][s][k]) for k in a[1][s])
            assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    p, x, y, eps = ic.inputs((3, 17, (129, 127)), 50)
    want = vo.m2info_losses_and_grads(p, x, y, eps, 0.5, 10.0, 1.0, ic.ELBO_EPS)
    got = mr.losses_and_grads(p, x, y, eps, 0.5, 10.0, 1.0, ic.ELBO_EPS)
    assert all(np.array_equal(want[0][k], got[0][k]) for k in want[0])
    for w, g in zip(want[1:], got[1:]):
        assert set(w) == set(g) and all(np.array_equal(w[k], g[k]) for k in w)
    with pytest.raises(ValueError):
        mr.losses_and_grads(p, x, y, eps, 0.5, 10.0, 1.0, ic.ELBO_EPS, aux_enc="v3")


def test_mode_truth_against_finite_differences():
    """The composed backward pass is the gradient of the composed losses: central differences in float64 along one random direction
    per tensor group, for enc_loss into the enc_dec_clf tensors and for aux_loss - (beta V) into the auxiliary ones."""
    case, B = (3, 17, (129, 127)), 5
    p, x, y, eps = (ic.inputs(case, 50)[0],) + tuple(a[:B] for a in ic.inputs(case, 50)[1:])
    p = {k: v.astype(np.float64) for k, v in p.items()}
    x, y, eps = x.astype(np.float64), y.astype(np.float64), eps.astype(np.float64)
    w = (0.5, 10.0, 3.0)
    rng = np.random.default_rng(0)
    worst = 0.0
    for mode in mc.MODES:
        out, g1, g2 = mr.losses_and_grads(p, x, y, eps, *w, ic.ELBO_EPS, *mode)
        for group, loss_of, grad_of in (
                ([k for k in p if not k.startswith(ic.AUX)], lambda o: o["enc_loss"], lambda k: g1[k]),
                ([k for k in p if k.startswith(ic.AUX)], lambda o: o["aux_loss"] - o["aux_enc_loss"], lambda k: g1[k] + g2[k])):
            d = {k: rng.standard_normal(p[k].shape) for k in group}
            h = 1e-6
            lp = loss_of(mr.losses_and_grads({k: v + h * d.get(k, 0) for k, v in p.items()}, x, y, eps, *w, ic.ELBO_EPS, *mode)[0])
            lm = loss_of(mr.losses_and_grads({k: v - h * d.get(k, 0) for k, v in p.items()}, x, y, eps, *w, ic.ELBO_EPS, *mode)[0])
            fd = (lp - lm) / (2 * h)
            an = sum(float(np.sum(np.reshape(grad_of(k), p[k].shape) * d[k])) for k in group)
            err = abs(fd - an) / max(abs(an), 1e-30)
            print(f"{mc.mode_id(mode)} {'aux' if group[0].startswith(ic.AUX) else 'enc_dec_clf'}: analytic {an:.6e}, differences {fd:.6e}, {err:.1e}")
            worst = max(worst, err)
    assert worst <= 1e-5


def test_float32_premise():
    """float32 numpy on the same inputs stays within half of each bar at every case, mode and batch -- for enc_loss relative to itself
    except at the (case, mode, B) of ENC_LOSS_BY_TERMS, and those are exactly the ones that need it."""
    worst_l = worst_g = worst_b = 0.0
    need = set()
    for case in mc.CASES:
        for mode in mc.MODES:
            for B in mc.BATCHES:
                l64, g64, _, _ = mc.truth(case, B, mode)
                l32, g32, _, _ = mc.run_on(*ic.inputs(case, B), np.float32, mode)
                plain = mc.loss_errs(l32[0], l64[0])
                if plain[3] > 0.5 * ic.LOSS_RTOL:
                    need.add((case, mode, B))
                le = mc.loss_err(l32[0], l64[0], mc.by_terms(case, mode, B))
                ge, name = ic.grad_err(g32[0], g64[0])
                be, bname = ic.grad_err(mc.block_grads(g32[0], case[1]), mc.block_grads(g64[0], case[1]))
                worst_l, worst_g, worst_b = max(worst_l, le), max(worst_g, ge), max(worst_b, be)
                assert le <= 0.5 * ic.LOSS_RTOL and ge <= 0.5 * ic.GRAD_TOL and be <= 0.5 * ic.GRAD_TOL, (case, mode, B, le, ge, name, be, bname)
    print(f"float32 numpy: losses {worst_l:.1e}, gradients {worst_g:.1e}, blocks {worst_b:.1e}; enc_loss compared by its terms at {sorted(need)}")
    assert need == set(mc.ENC_LOSS_BY_TERMS)


def test_trajectory_premises():
    """LR_TRAJ is the largest candidate at which at most a quarter of the (case, mode) pairs drop, and every pair keeps a frame."""
    pairs = [(c, m) for c in mc.CASES for m in mc.MODES]
    chosen = None
    for lr in mc.LR_CANDIDATES:
        kept = {(c, m): mc.traj_kept(c, m, lr) for c, m in pairs}
        dropped = sum(mc.traj_dropped(c, m, lr) for c, m in pairs)
        for m in mc.MODES:
            print(f"lr {lr:g} {mc.mode_id(m)}: kept {[kept[(c, m)] for c in mc.CASES]}")
        if chosen is None and dropped <= ic.TRAJ_DROPPED_MAX * len(pairs):
            chosen = lr
            break
    assert chosen == mc.LR_TRAJ
    assert all(mc.traj_frames(c, m).size >= 1 for c, m in pairs)


def _numpy_step(params, state, x, y, e, mode, weights):
    p = {k: v.astype(np.float32) for k, v in params.items()}
    if state is None:
        state = (vo.AdamState([k for k in p if not k.startswith(ic.AUX)]), vo.AdamState([k for k in p if k.startswith(ic.AUX)]))
    a, b, g = weights
    out, g1, _, aux_total = mr.train_step(p, state[0], state[1], x, y, e, alpha=a, beta=b, gamma=g, eps=1e-8, lr=1e-4, dec_label=mode[0],
                                          aux_enc=mode[1])
    g1 = {k: (np.zeros_like(p[k]) if isinstance(v, (int, float)) else v) for k, v in g1.items()}
    return ic.losses_of(out), g1, aux_total, p, state


@pytest.mark.parametrize("case", gmc.CASES, ids=[c[0] for c in gmc.CASES])
def test_float32_truth_matches_the_reference_vectors(case):
    """tests/golden/make_golden_modes.py ran the reference's own models, losses and torch.optim.Adam; the float32 numpy truth is held
    to what it stored with the default tolerances of golden_check.check_case for M2_info."""
    gmc.check_case(_numpy_step, gu.load_golden(gmc.STEM), case)

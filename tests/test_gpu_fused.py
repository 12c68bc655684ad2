"""GPU parity of the fused train step (disentangled-vae_amd/trainer.py -> dvae_train_* C ABI):
golden vectors from the reference (fp32 operand mode, the parity mode), the numpy oracle at
BASELINE.json's batch size, ragged batches, determinism, and the bf16 operand mode with its
measured deviation stated."""
import importlib
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from golden_check import check_case
from oracle import vae_oracle as vo

pytestmark = pytest.mark.gpu
trainer = importlib.import_module("disentangled-vae_amd.trainer")
N = importlib.import_module("disentangled-vae_amd.native")


def _has_diag():
    try:
        return bool(N.load().dvae_build_has_diag())
    except Exception:
        return False


# tests of the measured-slower alternates: they exist in the diagnostic library only (python disentangled-vae_amd/build.py --diag, then
# DVAE_LIB=disentangled-vae_amd/libdvae_hip_diag.so python -m pytest ...); the default library holds product kernels only
needs_diag = pytest.mark.skipif(not _has_diag(), reason="alternate kernels: diagnostic build only (build.py --diag, DVAE_LIB=...)")

X3_TOL = 5e-5      # bf16x3: every gradient tensor within this fraction of its maximum (measured worst 1.8e-5, profiles/r04_parity.json)

FULL = [c for c in gu.CASES if c[0] in ("M1_full", "M2_full_y1", "M2_full_y513", "M2_full_y513_hot")]


class FusedImpl:
    def __init__(self, precision="fp32", ksplit=0):
        self.precision, self.ksplit = precision, ksplit

    def load(self, model, dims, params):
        self.model, self.dims, self.p0 = model, dims, params
        self.tr = None

    def step(self, x, y, e):
        if self.tr is None:
            self.tr = trainer.Trainer(self.model, self.dims, self.p0, batch=x.shape[0], precision=self.precision, ksplit=self.ksplit)
        t = lambda a: None if a is None else torch.from_numpy(a).cuda()
        losses = self.tr.step(t(x), t(y), t(e)).cpu().numpy().astype(np.float64)
        return dict(losses=tuple(losses), grads=self.tr.grads_numpy())

    def params(self):
        return self.tr.state_dict_numpy()


@pytest.mark.parametrize("case", FULL, ids=[c[0] for c in FULL])
def test_fused_fp32_matches_reference_vectors(vae_golden, case):
    check_case(FusedImpl("fp32"), vae_golden, case)


ALL_FULL = FULL + [c for c in gu.CASES if c[0] in ("M2info_full", "M2info_full_b1")]


@pytest.mark.parametrize("case", ALL_FULL, ids=[c[0] for c in ALL_FULL])
def test_fused_bf16x3_matches_reference_vectors(vae_golden, case):
    """The BENCHMARKED operand policy (bf16x3: split-bf16 operands, three MFMAs per product) against the vectors captured from the
    reference itself (fp32 torch on CPU), all six reference-geometry cases, three Adam steps each.  Stated bounds: loss scalars 1e-5
    relative; every gradient element within 1e-4 relative + 2e-4 of its tensor's maximum (measured worst: profiles/r03_parity.json);
    parameters after 1 and 3 Adam steps within steps x lr everywhere and within the fp32 bound for all but 6 % of the elements
    (Adam's first steps are sign-like: an element whose gradient is rounding noise moves by +-lr in any two correct implementations)."""
    impl = FusedInfoImpl("bf16x3") if case[1] == "M2_info" else FusedImpl("bf16x3")
    check_case(impl, vae_golden, case, rtol_loss=1e-5, rtol_grad=1e-4, atol_rel_grad=2e-4, bad_frac=0.06)


@pytest.mark.parametrize("case", gu.BIG_CASES, ids=[c[0] for c in gu.BIG_CASES])
def test_fused_bf16x3_matches_reference_vectors_at_the_benchmarked_batch(vae_golden_big, case):
    """BASELINE.json configs 1-3 at their own batch: 8192 frames per step, bench.py's operand policy, against vectors captured from the
    REFERENCE ITSELF on CPU (tests/golden/make_golden.py --big: scripts/training_M2.py:132-147, training_M1.py:125-139,
    training_M2_info_vad.py:153-198; three Adam steps).  Bounds: loss scalars 1e-5 relative; every sampled gradient element within
    X3_TOL (5e-5) of its tensor's maximum -- no elementwise-relative allowance on top; the moments of every gradient tensor; parameters
    after 1 and 3 Adam steps as in the B <= 32 cases.  M2_info's ReLU nets (classifier, auxiliary net and, through -beta BCE, everything
    upstream of z) take the raw-batch bound of test_fused_m2info_vs_oracle_full_batch (1e-3: mask flips of units within rounding of zero,
    DESIGN 3)."""
    info = case[1] == "M2_info"
    impl = FusedInfoImpl("bf16x3") if info else FusedImpl("bf16x3")
    check_case(impl, vae_golden_big, case, rtol_loss=1e-5, rtol_grad=0.0, atol_rel_grad=1e-3 if info else X3_TOL, bad_frac=0.06)


def _oracle_step(model, dims, params, x, y, e):
    p = {k: v.copy() for k, v in params.items()}
    opt = vo.AdamState(list(p))
    out, grads = vo.train_step_vae(model, p, opt, x, y, e)
    return out, grads, p


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / (np.max(np.abs(b)) + 1e-30))


# bf16x3 gradient bound (fraction of the tensor's maximum), see test_fused_step_vs_oracle
def x3_grad_bound(name):
    return X3_TOL


# 20 000 frames = 625 tiles: more tiles than workgroups (256 fp32 / 512 bf16), i.e. the persistent tile loop
@pytest.mark.parametrize("model,y_dim,B", [("M2", 513, 8192), ("M1", 0, 8192), ("M2", 1, 1000), ("M2", 513, 33), ("M1", 0, 1), ("M2", 1, 20000),
                                           ("M2", 513, 20000), ("M2", 513, 65536)])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_fused_step_vs_oracle(model, y_dim, B, precision):
    """fp32 operand mode: <= 1e-4 relative (north_star bar) on losses and gradients.
    bf16x3 (split bf16, three MFMAs per product: the benchmarked mode): losses <= 1e-5 relative (measured <= 3e-7); every gradient tensor
    within 5e-5 of its maximum and 5e-5 in rms at EVERY batch size and label type measured (B = 1000 / 8192 / 20 000 / 65 536, binary
    and full-mantissa labels: worst 1.8e-5, profiles/r04_parity.json).  Round 3 measured 7.5e-5 ... 3.3e-4 on the weight of encoder
    layer 1, by the batch's content; tools/r04/sim_l1x.py traced all of it to the 16-bit operands of the L1 x GEMM on heavy-tailed power
    spectra (a unit on the knee of tanh whose terms are ~100), and since round 4 that one GEMM multiplies split-FP16 planes (11 + 11
    bits, fixed power-of-two scales, csrc/fused_tiles.hpp: struct X16) while its weight-gradient operand keeps split-bf16 planes of the
    fp32 values (relative precision per element: Adam normalises each element by its own history).
    bf16 (one bf16 per operand, opt-in fast mode): the synthetic power spectra span 1e-12 .. 1e4, so bf16
    rounding of x and W1 moves encoder pre-activations by O(1) on the loudest frames; measured deviation bound
    stated here: losses 2e-3 relative, every gradient tensor cosine >= 0.99 with the fp64 oracle and within 0.3 of its max.
    Every figure here is relative to a tensor's LARGEST element; per input column, each at its own scale: tests/test_gpu_fused_columns.py."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 11)
    x, y, e = gu.make_batch(dims, B, 12)
    out, grads, p_after = _oracle_step(model, dims, params, x.astype(np.float64), None if y is None else y.astype(np.float64),
                                       e.astype(np.float64))
    tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    ref = np.array([out["loss"], out["recon"], out["kl"]])
    ltol, gtol = {"fp32": (1e-4, 1e-4), "bf16x3": (1e-5, None), "bf16": (2e-3, 0.3)}[precision]
    np.testing.assert_allclose(losses, ref, rtol=ltol)
    g = tr.grads_numpy()
    worst = max(_relmax(g[k], np.asarray(grads[k], np.float64).reshape(g[k].shape)) for k in grads)
    print(f"fused[{model},y{y_dim},B{B},{precision}]: loss rel err {np.max(np.abs(losses - ref) / np.abs(ref)):.2e}, worst grad relmax {worst:.2e}")
    for k in grads:
        gr = np.asarray(grads[k], np.float64).reshape(g[k].shape)
        assert _relmax(g[k], gr) < (gtol if gtol is not None else x3_grad_bound(k)), k
        if precision == "bf16x3":
            rms = float(np.sqrt(np.mean((g[k].astype(np.float64) - gr) ** 2)) / (np.sqrt(np.mean(gr ** 2)) + 1e-30))
            assert rms < 5e-5, (k, rms)
        if precision == "bf16" and B > 1:
            cos = float(np.sum(g[k] * gr) / (np.linalg.norm(g[k]) * np.linalg.norm(gr) + 1e-300))
            assert cos > (0.99 if B < 20000 else 0.97), (k, cos)     # the 20 000-frame draw holds louder outliers (0.982 on W1)
    pn = tr.state_dict_numpy()
    for k in params:
        assert np.max(np.abs(pn[k] - params[k])) <= 1.05e-4          # one Adam step at lr 1e-4
        assert np.all(np.isfinite(pn[k]))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("model,y_dim,B", [("M2", 513, 8192), ("M2_info", 1, 2000), ("M1", 0, 300), ("M2", 1, 20000)])
def test_class_sliced_weight_gradient_schedule_equals_the_uniform_one(model, y_dim, B, precision, monkeypatch):
    """The weight-gradient launch reads a host-built item table (csrc/train_fused.hip: w4_build_items).  Class-sliced (default under the fp32
    policy, DVAE_W4_CLASSES=1 elsewhere): every block of 32 x 32 tiles is cut into as many frame slices as its cost per k-step asks for and
    writes only its own first slabs -- the others keep the zeros of dvae_train_init.  Against the uniform table (DVAE_W4_UNIFORM=1): the same
    losses bit for bit (the rows kernel is untouched), gradients equal up to the order of the slab sums, over three steps on one workspace
    (a slab that held anything but zeros would show from the second step on), and the class-sliced run is deterministic."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 5)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    batches = [gu.make_batch(dims, B, 60 + i) for i in range(3)]
    res = {}
    for mode in ("uniform", "classes", "classes2"):
        monkeypatch.delenv("DVAE_W4_UNIFORM", raising=False); monkeypatch.delenv("DVAE_W4_CLASSES", raising=False)
        monkeypatch.setenv("DVAE_W4_UNIFORM" if mode == "uniform" else "DVAE_W4_CLASSES", "1")
        tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
        assert (tr.plan.reserved0 > 0) == (mode != "uniform")
        out = []
        for x, y, e in batches:
            losses = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
            out.append((losses, tr.grads_numpy()))
        res[mode] = (out, tr.state_dict_numpy())
    for i, ((lu, gu_), (lc, gc), (lc2, gc2)) in enumerate(zip(res["uniform"][0], res["classes"][0], res["classes2"][0])):
        assert np.array_equal(lc, lc2) and all(np.array_equal(gc[k], gc2[k]) for k in gc)
        if i == 0:
            assert np.array_equal(lc[:3], lu[:3])
        np.testing.assert_allclose(lc[:3], lu[:3], rtol=1e-5)      # steps 2, 3 start from parameters that differ where Adam's first steps are sign-like
        for k in gu_:
            assert _relmax(gc[k], gu_[k].astype(np.float64)) < (2e-6 if i == 0 else 2e-3), (i, k)
    for k in res["uniform"][1]:
        assert np.max(np.abs(res["uniform"][1][k] - res["classes"][1][k])) <= 2.1e-4     # three Adam steps at lr 1e-4, sign-like where |g| ~ eps
        assert np.array_equal(res["classes"][1][k], res["classes2"][1][k])


@pytest.mark.parametrize("model,y_dim,B,precision", [("M2", 513, 8192, "bf16x3"), ("M1", 0, 1000, "bf16x3"), ("M2_info", 1, 3000, "fp32")])
def test_a_plan_made_for_two_weight_gradient_launches_steps_like_the_one_launch_plan(model, y_dim, B, precision, monkeypatch):
    """A plan made under DVAE_EXCHANGE_GROUPS=2 holds two item tables (decoder-side blocks, encoder blocks), each cut to fill the CUs by
    itself; the single-process step on it (dvae_train_step -> both launches, back to back) gives the uniform plan's losses bit for bit and
    its gradients up to the order of the slab sums, over three steps on one workspace."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 6)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    batches = [gu.make_batch(dims, B, 70 + i) for i in range(3)]
    res = {}
    for mode in ("uniform", "groups"):
        for k in ("DVAE_W4_UNIFORM", "DVAE_W4_CLASSES", "DVAE_EXCHANGE_GROUPS"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("DVAE_W4_UNIFORM" if mode == "uniform" else "DVAE_EXCHANGE_GROUPS", "1" if mode == "uniform" else "2")
        tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
        assert tr._groups == (2 if mode == "groups" else 1)
        out = []
        for x, y, e in batches:
            losses = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
            out.append((losses, tr.grads_numpy()))
        res[mode] = out
    for i, ((lu, gu_), (lg, gg)) in enumerate(zip(res["uniform"], res["groups"])):
        if i == 0:
            assert np.array_equal(lu[:3], lg[:3])
        np.testing.assert_allclose(lg[:3], lu[:3], rtol=1e-5)
        for k in gu_:
            assert _relmax(gg[k], gu_[k].astype(np.float64)) < (2e-6 if i == 0 else 2e-3), (i, k)


def test_fused_is_deterministic_and_ksplit_invariant():
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 3)
    x, y, e = gu.make_batch(dims, 4096, 4)
    t = lambda a: torch.from_numpy(a).cuda()
    res = []
    for ks in (0, 0, 1, 3):
        tr = trainer.Trainer("M2", dims, params, batch=4096, precision="fp32", ksplit=ks)
        for _ in range(2):
            losses = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
        res.append((losses, tr.state_dict_numpy()))
    assert np.array_equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k           # bitwise reproducible run to run
        for other in res[2:]:
            assert np.max(np.abs(res[0][1][k] - other[1][k])) <= 2.1e-4   # slab count only reorders fp32 sums


@pytest.mark.parametrize("path,ltol,gtol", [("layers", 2e-5, 5e-5), ("fused", 2e-5, 1e-3)])
def test_fused_matches_module_paths_at_full_batch(path, ltol, gtol, monkeypatch):
    """The fp32 fused trainer against the drop-in modules + autograd + torch Adam at B = 8192: the per-layer fp32 Functions
    (DVAE_MODULE_PATH=layers) and the whole-model path (one Function per forward, split-bf16 operands: measured 1.5e-4)."""
    from impl_modules import ModuleImpl
    monkeypatch.setenv("DVAE_MODULE_PATH", path)
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 5)
    x, y, e = gu.make_batch(dims, 8192, 6)
    mi = ModuleImpl("cuda")
    mi.load("M2", dims, {k: v.copy() for k, v in params.items()})
    out = mi.step(x, y, e)
    assert (mi.m.__dict__.get("_dvae_engine") is not None) == (path == "fused")
    tr = trainer.Trainer("M2", dims, params, batch=8192, precision="fp32")
    t = lambda a: torch.from_numpy(a).cuda()
    losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    np.testing.assert_allclose(losses, out["losses"], rtol=ltol)
    g = tr.grads_numpy()
    for k in params:
        assert _relmax(g[k], out["grads"][k].astype(np.float64)) < gtol, k


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_workgroup_blocked_wgrad_kernel_equals_the_default(precision, monkeypatch):
    """The three forms of the weight-gradient pass -- the workgroup k-split 4 x 4 kernel (default), DVAE_WGRAD=ring (2 x 2 tiles per
    wave, register ring) and DVAE_WGRAD=lds (4 x 4 blocks, operands staged once in LDS) -- compute the same gradients from the same
    stash: identical operand values, only the order of the frame sums differs (fp32 rounding: 2e-6 of a tensor's maximum)."""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 8)
    x, y, e = gu.make_batch(dims, 3000, 9)                       # 94 tiles: ragged last tile, partial last k-slice
    t = lambda a: torch.from_numpy(a).cuda()
    got = {}
    kinds = ("wg4", "ring", "lds") if _has_diag() else ("wg4", "ring")       # the LDS-staged form: diagnostic builds only
    for kind in kinds:
        monkeypatch.setenv("DVAE_WGRAD", kind)
        tr = trainer.Trainer("M2", dims, params, batch=3000, precision=precision)
        tr.step(t(x), t(y), t(e))
        got[kind] = tr.grads_numpy()
    for k in got["wg4"]:
        for kind in kinds[1:]:
            assert _relmax(got[kind][k], got["wg4"][k].astype(np.float64)) < 2e-6, (kind, k)


def test_state_dict_round_trip_and_repack():
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    tr = trainer.Trainer("M2", dims, None, batch=64, precision="bf16", seed=0)
    sd = tr.state_dict()
    from packages.models.models import DeepGenerativeModel
    torch.manual_seed(0)
    m = DeepGenerativeModel([513, 1, 16, [128, 128]], None)
    for k, v in m.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k                        # same seeded init as the drop-in module
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    x, y, e = gu.make_batch(dims, 64, 1)
    t = lambda a: torch.from_numpy(a).cuda()
    l1 = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
    tr2 = trainer.Trainer("M2", dims, gu.make_params("M2", dims, 99), batch=64, precision="bf16")
    tr2.load_state_dict({k: v for k, v in sd.items()})
    l2 = tr2.step(t(x), t(y), t(e)).cpu().numpy()
    np.testing.assert_array_equal(l1, l2)
    with pytest.raises(NotImplementedError):
        trainer.Trainer("M2", dict(x_dim=513, y_dim=7, z_dim=16, h_dim=(128, 128)), None, batch=8)


def _dp_worker(rank, world, port, q, model="M2", y_dim=513, precision="fp32", exchange="rccl", groups=1):
    import os, sys
    os.environ["DVAE_ALLREDUCE"] = exchange
    if groups == 2:
        os.environ["DVAE_EXCHANGE_GROUPS"] = "2"
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    import importlib, numpy as np, torch, torch.distributed as dist
    import golden_util as gu
    tr_mod = importlib.import_module("disentangled-vae_amd.trainer")
    dp = importlib.import_module("disentangled-vae_amd.dp")
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    Bg = 512
    lo, hi = dp.shard_rows(Bg, rank, world)
    if exchange == "direct":
        # the staged constructor bench.py uses: a stage that fails on ONE rank (here: rank 1 asks for an impossible size) is reported on
        # every rank and nobody is left waiting in a collective
        dx, why = dp.DirectExchange.try_create(1000 if rank == 0 else -5, dist.group.WORLD)
        assert dx is None and "rank 1" in why, (dx, why)
    tr = tr_mod.Trainer(model, dims, gu.make_params(model, dims, 21), batch=hi - lo, precision=precision,
                        process_group=dist.group.WORLD, world=world)
    for step in range(2):
        x, y, e = gu.make_batch(dims, Bg, 30 + step)
        t = lambda a: torch.from_numpy(a[lo:hi].copy()).cuda()
        losses = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
    failed = tr.direct.failed() if tr.direct is not None else False
    assert tr._groups == groups
    q.put((rank, tr.state_dict_numpy(), losses, failed, tr.direct is not None))
    if tr.direct is not None:
        dist.barrier()
        tr.direct.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("model,y_dim,precision", [("M2", 513, "fp32"), ("M2", 513, "bf16x3"), ("M2_info", 1, "fp32")])
def test_two_rank_data_parallel_equals_single_process(model, y_dim, precision):
    """2 ranks (sharing the one GPU, gloo in place of RCCL) == 1 rank on the concatenated batch; M2_info: both Adam
    groups travel in the one flat buffer."""
    import torch.multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() + 7 * len(model) + y_dim + len(precision)) % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, model, y_dim, precision)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    tr = trainer.Trainer(model, dims, gu.make_params(model, dims, 21), batch=512, precision=precision)
    for step in range(2):
        x, y, e = gu.make_batch(dims, 512, 30 + step)
        t = lambda a: torch.from_numpy(a).cuda()
        losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    ref = tr.state_dict_numpy()
    # the two halves sum their gradients in a different order than one 512-frame pass; Adam's first steps are sign-like, so a
    # gradient that is rounding noise moves its parameter by up to 2 lr either way: bound the bulk tightly, every element by 2 steps
    for k in ref:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k                      # replicas identical
        d = np.abs(res[0][1][k] - ref[k])
        assert d.max() <= (2e-6 if (model, precision) == ("M2", "fp32") else 4.1e-4), (k, d.max())
        assert np.mean(d > 2e-6) < (0.0 if (model, precision) == ("M2", "fp32") else 0.02) + 1e-12, (k, float(np.mean(d > 2e-6)))
    np.testing.assert_allclose(0.5 * (res[0][2] + res[1][2]), losses, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("model,y_dim,precision", [("M2", 513, "bf16x3"), ("M2", 513, "fp32"), ("M2_info", 1, "bf16x3")])
def test_two_launch_weight_gradients_with_the_exchange_between_them(model, y_dim, precision):
    """DVAE_EXCHANGE_GROUPS=2 (opt-in; csrc/train_fused.hip: dvae_train_grads_group): the gradient pass of a data-parallel step as rows +
    weight gradients of the decoder-side tensors, their part of the flat gradient handed to the exchange, the encoder's weight gradients,
    their part, then the optimizer launch.  Two ranks sharing the one GPU (gloo in place of RCCL): replicas identical, and equal to the
    one-launch / one-exchange step up to the order of the slab sums (the same bounds the two-rank step holds against the one-rank step:
    Adam's first steps are sign-like where a gradient is rounding noise).  M2_info: the side nets' tensors travel with the decoder's."""
    import torch.multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    got = {}
    for groups in (2, 1):
        q = ctx.Queue()
        port = 33000 + (os.getpid() + 11 * len(model) + y_dim + 5 * groups + len(precision)) % 2000
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, model, y_dim, precision, "rccl", groups)) for r in range(2)]
        for pr in procs:
            pr.start()
        res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
        got[groups] = res
    for k in got[1][0][1]:
        assert np.array_equal(got[2][0][1][k], got[2][1][1][k]), k                # replicas identical
        d = np.abs(got[2][0][1][k] - got[1][0][1][k])
        assert d.max() <= 4.1e-4, (k, d.max())
        assert np.mean(d > 2e-6) < 0.02, (k, float(np.mean(d > 2e-6)))
    np.testing.assert_allclose(got[2][0][2], got[1][0][2], rtol=1e-5, atol=1e-6)   # the second step's losses (rank 0)


@pytest.mark.parametrize("model,y_dim,precision", [("M2", 513, "bf16x3"), ("M2_info", 1, "bf16x3")])
def test_direct_exchange_equals_the_process_group_exchange(model, y_dim, precision):
    """DVAE_ALLREDUCE=direct (dvae_allreduce_flat: slab sum + reduce-scatter by pull + all-gather by push over hipIpc-mapped peer buffers,
    one launch per rank on the step's stream) against the process-group all-reduce, two ranks sharing the one GPU: the parameters after
    two steps are bit-identical (at world 2 both paths add the two ranks' slab sums once), no bounded wait expired."""
    import torch.multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    got = {}
    for exchange in ("direct", "rccl"):
        q = ctx.Queue()
        port = 31000 + (os.getpid() + 13 * len(model) + y_dim + (7 if exchange == "direct" else 0)) % 2000
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, model, y_dim, precision, exchange)) for r in range(2)]
        for pr in procs:
            pr.start()
        res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
        got[exchange] = res
    for r in range(2):
        assert got["direct"][r][4] and not got["rccl"][r][4]                       # the direct path really ran
        assert not got["direct"][r][3], "a bounded wait for the peer expired"
        np.testing.assert_array_equal(got["direct"][r][2], got["rccl"][r][2])
        for k in got["rccl"][r][1]:
            np.testing.assert_array_equal(got["direct"][r][1][k], got["rccl"][r][1][k], err_msg=k)


def test_direct_exchange_at_four_ranks():
    """World 4 (four processes on the one GPU): the reduce-scatter shards, the pull order and the all-gather of dvae_allreduce_flat beyond
    two ranks.  The direct path adds the ranks' slab sums in rank order, gloo in its own: parameters after two steps agree to the Adam
    noise of a re-ordered fp32 sum (every replica identical within a run; no bounded wait expired)."""
    import torch.multiprocessing as mp
    import os
    ctx = mp.get_context("spawn")
    got = {}
    for exchange in ("direct", "rccl"):
        q = ctx.Queue()
        port = 33000 + (os.getpid() + (7 if exchange == "direct" else 0)) % 2000
        procs = [ctx.Process(target=_dp_worker, args=(r, 4, port, q, "M2", 513, "bf16x3", exchange)) for r in range(4)]
        for pr in procs:
            pr.start()
        res = sorted([q.get(timeout=400) for _ in procs], key=lambda t: t[0])
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
        got[exchange] = res
    for r in range(4):
        assert got["direct"][r][4] and not got["direct"][r][3]
        for k in got["rccl"][0][1]:
            np.testing.assert_array_equal(got["direct"][r][1][k], got["direct"][0][1][k], err_msg=k)      # replicas identical
            d = np.abs(got["direct"][r][1][k] - got["rccl"][r][1][k])
            assert d.max() <= 4.1e-4 and np.mean(d > 2e-6) < 0.02, (k, float(d.max()), float(np.mean(d > 2e-6)))


def _late_peer_worker(rank, world, port, q):
    import os, sys, time
    os.environ["DVAE_ALLREDUCE"] = "direct"
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    import importlib, numpy as np, torch, torch.distributed as dist
    import golden_util as gu
    tr_mod = importlib.import_module("disentangled-vae_amd.trainer")
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    tr = tr_mod.Trainer("M2", dims, gu.make_params("M2", dims, 21), batch=64, precision="fp32", process_group=dist.group.WORLD, world=world)
    x, y, e = gu.make_batch(dims, 64, 30 + rank)
    t = lambda a: torch.from_numpy(a).cuda()
    l1 = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()          # both ranks on time (default bound: 20 s)
    ok1 = not tr.direct.failed()
    tr.direct.set_timeout_ms(150)
    dist.barrier()
    if rank == 1:
        time.sleep(1.5)                                           # a checkpoint / validation / data stall longer than the bound
    t0 = time.time()
    l2 = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
    dt = time.time() - t0
    failed = tr.direct.failed()
    raised = False
    try:
        tr.state_dict()
    except RuntimeError:
        raised = True
    p = np.concatenate([tr.tensor_view(i).reshape(-1).cpu().numpy() for i in range(len(tr.names))])
    l3 = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()          # the step after: its forward runs on the NaN parameters
    q.put((rank, ok1, bool(np.all(np.isfinite(l1))), failed, raised, bool(np.isnan(l3[0])), float(np.mean(np.isnan(p))), dt))
    dist.barrier()
    tr.direct.close()
    dist.destroy_process_group()


def test_direct_exchange_late_peer_fails_in_band_on_every_rank():
    """a rank that arrives later than the bound of the in-kernel waits must not leave its peers with a stale sum.  Rank 1 sleeps
    1.5 s in front of a step whose bound is 150 ms: rank 0's launch gives up, stores its status into EVERY rank's header and fills its
    reduced gradient with NaN; rank 1's launch (which finds everything it waits for) sees the status and does the same.  Both ranks:
    failed() is True, every parameter is NaN after the step (its own loss was computed before the exchange), the next step's loss is NaN,
    state_dict() raises, nothing hangs."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35000 + os.getpid() % 2000
    procs = [ctx.Process(target=_late_peer_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rank, ok1, fin1, failed, raised, nan_loss, nan_frac, dt in res:
        assert ok1 and fin1, (rank, "the on-time step must succeed")
        assert failed and raised, (rank, failed, raised)
        assert nan_loss and nan_frac == 1.0, (rank, nan_loss, nan_frac)
        assert dt < 10.0, (rank, dt)


def _world8_worker(proc, nproc, port, q, n, n_slabs):
    """Two ranks of an eight-rank exchange hosted by ONE process (ranks 2 proc, 2 proc + 1; each on its own stream): four processes on the
    one GPU stay within the box's process limit.  Straight through the C ABI (include/dvae_train.h)."""
    import os, sys, ctypes
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    import importlib, numpy as np, torch, torch.distributed as dist
    N = importlib.import_module("disentangled-vae_amd.native")
    dp = importlib.import_module("disentangled-vae_amd.dp")
    lib = N.load()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=proc, world_size=nproc)
    world = 2 * nproc
    HB = dp.IPC_HANDLE_BYTES
    ranks = (2 * proc, 2 * proc + 1)
    comms, blobs = [], []
    for r in ranks:
        h = ctypes.c_void_p(); mine = (ctypes.c_ubyte * HB)()
        N.check(lib.dvae_comm_create(r, world, n, ctypes.byref(h), mine), "dvae_comm_create")
        comms.append(h); blobs.append(bytes(mine))
    gathered = [None] * nproc
    dist.all_gather_object(gathered, blobs)
    allb = b"".join(b for pair in gathered for b in pair)                    # rank order
    blob = (ctypes.c_ubyte * (HB * world)).from_buffer_copy(allb)
    for h in comms:
        N.check(lib.dvae_comm_connect(h, blob), "dvae_comm_connect")
    dist.barrier()
    outs, streams, keep = [], [torch.cuda.Stream(), torch.cuda.Stream()], []
    for call in range(3):                                                    # three calls: counters and buffer reuse across calls
        res = []
        for i, r in enumerate(ranks):
            g = torch.Generator().manual_seed(1000 * call + r)
            slabs = torch.randn(n_slabs, n, generator=g).cuda()
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            keep.append(slabs)
            res.append(out)
        torch.cuda.synchronize()
        for i, r in enumerate(ranks):
            N.check(lib.dvae_allreduce_flat(comms[i], N.ptr(keep[-2 + i]), n_slabs, n, N.ptr(res[i]), ctypes.c_void_p(streams[i].cuda_stream)),
                    "dvae_allreduce_flat")
        torch.cuda.synchronize()
        outs.append([o.cpu().numpy() for o in res])
    failed = []
    for h in comms:
        f = ctypes.c_int(0)
        N.check(lib.dvae_comm_status(h, ctypes.byref(f)), "dvae_comm_status")
        failed.append(bool(f.value))
    q.put((proc, outs, failed))
    dist.barrier()
    for h in comms:
        lib.dvae_comm_destroy(h)
    dist.destroy_process_group()


def test_direct_exchange_at_eight_ranks_padded_last_shard():
    """World 8 on the flat gradient of M2 y 513 (302 625 floats: shard = ceil(n / 8) padded to 64 = 37 888, the last shard holds 37 409 real
    elements and 479 of padding): every rank's result equals the sum over the 8 ranks of the rank's slab sums, the ranks' results are
    bit-identical, over three calls (counter and buffer reuse).  Eight processes on the one GPU would exceed the box's process limit, so four
    processes host two ranks each (same-process peers connect by pointer, the others through their hipIpc handles).  One GPU: a rehearsal of
    the protocol's indexing and hand-offs, not a measurement -- the exchange is UNMEASURED on multi-GPU hardware."""
    import torch.multiprocessing as mp
    n, n_slabs, nproc = 302625, 3, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37000 + os.getpid() % 2000
    procs = [ctx.Process(target=_world8_worker, args=(r, nproc, port, q, n, n_slabs)) for r in range(nproc)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for call in range(3):
        per_rank = []
        for r in range(8):
            g = torch.Generator().manual_seed(1000 * call + r)
            slabs = torch.randn(n_slabs, n, generator=g).numpy()
            t = slabs[0].copy()
            for k in range(1, n_slabs):
                t = t + slabs[k]                                              # the kernel's slab order, fp32
            per_rank.append(t)
        ref = np.zeros(n, np.float32)
        for r in range(8):
            ref = ref + per_rank[r]                                           # rank order, fp32, from zero: the kernel's sum
        for proc, outs, failed in res:
            assert not any(failed), (proc, failed)
            for o in outs[call]:
                np.testing.assert_array_equal(o, ref)


class FusedInfoImpl(FusedImpl):
    """M2_info on the fused path: gradients of the enc_dec_clf group are what enc_loss.backward() leaves,
    gradients of the auxiliary group are the (gamma - beta) accumulation the second backward produces (quirk Q4)."""

    def step(self, x, y, e):
        if self.tr is None:
            self.tr = trainer.Trainer(self.model, self.dims, self.p0, batch=x.shape[0], precision=self.precision)
        t = lambda a: None if a is None else torch.from_numpy(a).cuda()
        losses = self.tr.step(t(x), t(y), t(e)).cpu().numpy().astype(np.float64)
        g = self.tr.grads_numpy()
        # order of the stored reference losses: ELBO, recon, KL, enc_loss, classif_loss, aux_loss, aux_enc_loss
        return dict(losses=tuple(losses[:7]), grads_enc={k: v for k, v in g.items()},
                    grads_aux_total={k: v for k, v in g.items() if k.startswith("auxiliary.")}, _fused_info=True)


@pytest.mark.parametrize("name", ["M2info_full", "M2info_full_b1"])
def test_fused_m2info_matches_reference_vectors(vae_golden, name):
    case = [c for c in gu.CASES if c[0] == name][0]
    check_case(FusedInfoImpl("fp32"), vae_golden, case)


@pytest.mark.parametrize("seed", [31, 77, 123])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_fused_m2info_vs_oracle_full_batch(precision, seed):
    """(three parameter / batch draws since round 5: the raw-batch bound no longer rests on one seed)"""
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    B = 8192
    params = gu.make_params("M2_info", dims, seed)
    x, y, e = gu.make_batch(dims, B, seed + 1)
    # float32 oracle, like the reference: the classifier sees raw power spectra up to 1e4, its sigmoid saturates to
    # exactly 1.0f and log(1 - p + eps) then depends on the arithmetic width (fp64 would differ by 3e-3 here)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    out, g1, g2 = vo.m2info_losses_and_grads(p32, x, y, e, 0.5, 10.0, 1.0)
    tr = trainer.Trainer("M2_info", dims, params, batch=B, precision=precision, alpha=0.5, beta=10.0, gamma=1.0)
    t = lambda a: torch.from_numpy(a).cuda()
    losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    ref = np.array([out["ELBO"], out["recon"], out["kl"], out["enc_loss"], out["classif_loss"], out["aux_loss"], out["aux_enc_loss"]])
    np.testing.assert_allclose(losses[:7], ref, rtol=5e-3 if precision == "bf16" else 1e-4, atol=1e-5)
    g = tr.grads_numpy()
    # bf16x3 on the RAW batch: 1e-3 bounds rows hit by ReLU flips (~110 frames of this batch have a unit within 1e-5 of a tie, and a layer-2
    # flip moves every row of the layer-1 gradient); the same batch without its near-tie frames holds 1e-4 on every row of every tensor:
    # test_fused_m2info_tie_free_batch_vs_oracle (round 4; measured figures in profiles/r04_parity.json)
    tol = {"fp32": 1e-4, "bf16x3": 1e-3, "bf16": 0.3}[precision]
    # The classifier / auxiliary nets are ReLU MLPs: the reference's own gradient is discontinuous where a hidden
    # pre-activation is within rounding of zero, and a mask that flips in ONE frame moves ONE row of that layer's weight
    # gradient (and one bias element) by about one frame's contribution, ~1e-3 of the tensor's maximum at 8192 frames.
    # tests/diag/info_rows.py: under bf16x3 every other row agrees to ~2e-6; the fp32 policy shows the same isolated rows
    # at other seeds (and the float32 and float64 oracles differ by up to 0.75 on the saturated classifier).  So: every
    # tensor within `tol` of its maximum except at most 2 rows per ReLU-net tensor, and those within 1e-2.
    worst_clean = 0.0
    for k in params:
        gr = (np.asarray(g1[k], np.float64) + (np.asarray(g2[k], np.float64) if k in g2 else 0.0)).reshape(g[k].shape)   # aux: (gamma - beta) dBCE
        err = np.abs(g[k].astype(np.float64) - gr) / (np.abs(gr).max() + 1e-30)
        relu_net = k.startswith("auxiliary.") or ".classifier." in k
        if relu_net and precision != "bf16":
            rows = np.sort(err.reshape(err.shape[0], -1).max(axis=1))[::-1]
            assert rows[0] < 1e-2, (k, rows[:3])
            # a flip in ONE unit of this layer: at most two rows beyond the bound.  A flip one layer DOWNSTREAM moves every row of this
            # layer's gradient a little (seed 123 under the exact-fp32 policy: 45 rows of the classifier's first layer between 1e-4 and
            # 6.6e-4, none above): then every row must stay under 1e-3
            assert (rows >= tol).sum() <= 2 or rows[0] < 1e-3, (k, rows[:4])
            worst_clean = max(worst_clean, float(rows[rows < tol].max()) if (rows < tol).any() else 0.0)
        else:
            assert err.max() < tol, k
            worst_clean = max(worst_clean, float(err.max()))
    print(f"fused[M2_info,B{B},{precision}]: loss rel err {np.max(np.abs(losses[:7] - ref) / (np.abs(ref) + 1e-5)):.2e}, worst gradient error "
          f"(outside <= 2 ReLU-tie rows per tensor) {worst_clean:.2e}")


def _relu_margins(params, x, e):
    """float64 oracle: per frame, the smallest margin |pre| / (sum_k |w_k in_k| + |b|) over every hidden unit of the four ReLU layers of
    M2_info (classifier on x: layers 1, 2; auxiliary net on z: layers 1, 2).  A unit whose margin is below the relative error of an
    arithmetic's products can take the other ReLU branch under that arithmetic."""
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


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_fused_m2info_tie_free_batch_vs_oracle(precision):
    """Round 4: what is left of the M2_info gradient deviation once ReLU ties are out of the batch.
    A ReLU mask is a discontinuity of the reference's own gradient: a hidden pre-activation within the arithmetic's product error of zero
    takes either branch, and a flip in LAYER 2 of a side net moves EVERY row of its layer-1 weight gradient (dpre1 = W2^T dpre2 * mask1),
    which is why 'at most two rows per tensor' (test_fused_m2info_vs_oracle_full_batch) cannot bound the layer-1 tensors under 16-bit
    operands: at 8192 frames ~110 frames have a unit with margin < 1e-5, ~1070 with margin < 1e-4 (tests/diag/r04_parity_law.py).
    Here the oracle replaces every frame that has a unit with margin < 1e-4 by a frame whose margins are all >= 4e-4 (1067 of 8192), and on
    that batch -- same model, same sizes, same kernel -- every gradient tensor is within 1e-4 of its maximum with NO row exempted
    (measured 2.4e-5 under both policies; 7.0e-5 on the classifier's first layer at another seed, tests/diag/r04_parity_law.py)."""
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    B, delta = 8192, 1e-4
    params = gu.make_params("M2_info", dims, 31)
    x, y, e = gu.make_batch(dims, B, 32)
    replaced = 0
    for _ in range(4):                                                   # a replaced frame brings its own noise, hence its own z: iterate
        worst = _relu_margins(params, x, e)
        risky = np.flatnonzero(worst < delta)
        if risky.size == 0:
            break
        safe = np.flatnonzero(worst >= 4 * delta)
        src = safe[(np.arange(risky.size) * 7919) % safe.size]
        x[risky], y[risky], e[risky] = x[src], y[src], e[src]
        replaced += risky.size
    assert _relu_margins(params, x, e).min() >= delta and replaced < B // 4
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    out, g1, g2 = vo.m2info_losses_and_grads(p32, x, y, e, 0.5, 10.0, 1.0)
    tr = trainer.Trainer("M2_info", dims, params, batch=B, precision=precision, alpha=0.5, beta=10.0, gamma=1.0)
    t = lambda a: torch.from_numpy(a).cuda()
    losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    ref = np.array([out["ELBO"], out["recon"], out["kl"], out["enc_loss"], out["classif_loss"], out["aux_loss"], out["aux_enc_loss"]])
    np.testing.assert_allclose(losses[:7], ref, rtol=1e-4, atol=1e-5)
    g = tr.grads_numpy()
    worst_by = {}
    for k in params:
        gr = (np.asarray(g1[k], np.float64) + (np.asarray(g2[k], np.float64) if k in g2 else 0.0)).reshape(g[k].shape)
        worst_by[k] = float(np.max(np.abs(g[k].astype(np.float64) - gr)) / (np.abs(gr).max() + 1e-30))
    wk = max(worst_by, key=worst_by.get)
    print(f"fused[M2_info tie-free, {replaced} frames replaced, {precision}]: worst gradient error {worst_by[wk]:.2e} ({wk})")
    for k, v in worst_by.items():
        assert v < 1e-4, (k, v)


def test_evaluate_is_forward_only_and_matches_step_losses():
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 41)
    x, y, e = gu.make_batch(dims, 1000, 42)
    t = lambda a: torch.from_numpy(a).cuda()
    tr = trainer.Trainer("M2", dims, params, batch=1000, precision="fp32")
    before = tr.state_dict_numpy()
    ev = tr.evaluate(t(x), t(y), t(e)).cpu().numpy()
    after = tr.state_dict_numpy()
    for k in before:
        assert np.array_equal(before[k], after[k]), k               # no update
    st = tr.step(t(x), t(y), t(e)).cpu().numpy()
    np.testing.assert_array_equal(ev, st)                            # same forward, same loss scalars
    out, _ = vo.vae_loss_and_grads("M2", {k: v.astype(np.float64) for k, v in params.items()}, x.astype(np.float64),
                                   y.astype(np.float64), e.astype(np.float64))
    np.testing.assert_allclose(ev, [out["loss"], out["recon"], out["kl"]], rtol=1e-4)


def test_in_kernel_noise_is_standard_normal_and_reproducible():
    from scipy import stats
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    tr = trainer.Trainer("M2", dims, batch=4096, precision="fp32", seed=7)
    n1, n2 = tr.noise(1).cpu().numpy(), tr.noise(2).cpu().numpy()
    assert n1.shape == (4096, 16) and np.isfinite(n1).all()
    assert np.array_equal(n1, tr.noise(1).cpu().numpy())                      # a pure function of (seed, step, frame)
    assert not np.array_equal(n1, n2)
    flat = np.concatenate([n1.ravel(), n2.ravel()])
    assert abs(flat.mean()) < 0.01 and abs(flat.std() - 1) < 0.01
    assert stats.kstest(flat, "norm").pvalue > 1e-3
    assert abs(np.corrcoef(n1.ravel(), n2.ravel())[0, 1]) < 0.02             # steps are independent streams
    assert abs(np.corrcoef(n1[:, 0], n1[:, 1])[0, 1]) < 0.05                  # so are latent dimensions
    other = trainer.Trainer("M2", dims, batch=4096, precision="fp32", seed=8).noise(1).cpu().numpy()
    assert not np.array_equal(n1, other)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_step_without_noise_tensor_equals_step_on_the_drawn_noise(precision):
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 3)
    x, y, _ = gu.make_batch(dims, 200, 4)
    t = lambda a: torch.from_numpy(a).cuda()
    a = trainer.Trainer("M2", dims, params, batch=200, precision=precision, seed=11)
    b = trainer.Trainer("M2", dims, params, batch=200, precision=precision, seed=11)
    for step in (1, 2):
        la = a.step(t(x), t(y)).clone()                                       # noise drawn inside the rows kernel
        lb = b.step(t(x), t(y), b.noise(step)).clone()                        # the same numbers, passed in
        assert torch.equal(la, lb)
    assert torch.equal(a.params, b.params)
    e1, e2 = a.evaluate(t(x), t(y)), a.evaluate(t(x), t(y))
    assert not torch.equal(e1, e2)                                            # validation noise advances too


def test_device_side_loss_accumulation():
    dims = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    tr = trainer.Trainer("M2", dims, batch=96, precision="fp32", seed=2)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    tr.accumulate_losses(acc)
    want = np.zeros(3)
    for _ in range(5):
        x = torch.rand(96, 513, device="cuda", generator=g) + 0.01
        y = (torch.rand(96, 1, device="cuda", generator=g) > 0.5).float()
        want += tr.step(x, y).cpu().numpy()[:3].astype(np.float64)
    want += tr.evaluate(x, y).cpu().numpy()[:3].astype(np.float64)
    np.testing.assert_allclose(acc.cpu().numpy()[:3], want, rtol=1e-12)
    tr.accumulate_losses(None)
    tr.step(x, y)
    np.testing.assert_allclose(acc.cpu().numpy()[:3], want, rtol=1e-12)     # detached: no more additions


@pytest.mark.parametrize("model,y_dim,precision,n,B", [("M2", 513, "fp32", 700, 200), ("M2", 513, "bf16", 700, 200), ("M1", 0, "bf16", 700, 200),
                                                       ("M2_info", 1, "fp32", 700, 200), ("M2", 513, "bf16x3", 700, 200), ("M2_info", 1, "bf16x3", 700, 200),
                                                       ("M2", 513, "bf16x3", 21000, 20000), ("M2", 513, "bf16", 21000, 19990)])
def test_in_kernel_row_gather_equals_gathered_batch(model, y_dim, precision, n, B):
    """B not a multiple of 32: the edge tile goes through the gather too; the 20 000-frame cases run the persistent tile loop (gather
    table double-buffered across tiles, the next tile's x / label loads through it)."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 5)
    x, y, e = gu.make_batch(dims, n, 6)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    rows = torch.randperm(n, device="cuda", generator=g)[:B].contiguous()
    a = trainer.Trainer(model, dims, params, batch=B, precision=precision, seed=3)
    b = trainer.Trainer(model, dims, params, batch=B, precision=precision, seed=3)
    X, Y, E = t(x), t(y), t(e)[:B].contiguous()
    la = a.step(X, Y, E, rows=rows).clone()
    lb = b.step(X[rows].contiguous(), None if Y is None else Y[rows].contiguous(), E).clone()
    assert torch.equal(la, lb) and torch.equal(a.params, b.params)
    assert torch.equal(a.evaluate(X, Y, E, rows=rows), b.evaluate(X[rows].contiguous(), None if Y is None else Y[rows].contiguous(), E))
    with pytest.raises(ValueError):
        a.step(X, Y, E, rows=rows[:10])


@pytest.mark.parametrize("model,y_dim,precision,tol", [("M2", 513, "fp32", 2e-4), ("M2", 1, "bf16", 2e-2), ("M2_info", 1, "fp32", 5e-4),
                                                       ("M2", 513, "bf16x3", 2e-4), ("M2_info", 1, "bf16x3", 5e-4)])
def test_long_trajectory_tracks_the_cpu_reference_loop(model, y_dim, precision, tol):
    """120 consecutive steps (lr 1e-3: the parameters move by ~0.1) against the torch-CPU restatement of the reference
    loop on the same batches and noise: Adam moments, bias correction and the weight-copy refresh over many steps."""
    from oracle import torch_ref as tref
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 9)
    B, nsteps, lr = 256, 120, 1e-3
    x, y, e = gu.make_batch(dims, B * 4, 10)
    tp = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    ref = tref.Stepper(model, tp, lr=lr)
    tr = trainer.Trainer(model, dims, params, batch=B, precision=precision, lr=lr)
    rng = np.random.default_rng(0)
    lr_hist, lf_hist = [], []
    for s in range(nsteps):
        sl = slice((s % 4) * B, (s % 4 + 1) * B)
        en = rng.standard_normal((B, 16)).astype(np.float32)
        xb, yb = x[sl], (None if y is None else y[sl])
        out = ref.step(torch.from_numpy(xb), None if yb is None else torch.from_numpy(yb), torch.from_numpy(en))
        lf = tr.step(torch.from_numpy(xb).cuda(), None if yb is None else torch.from_numpy(yb).cuda(), torch.from_numpy(en).cuda())
        lr_hist.append(out[0]); lf_hist.append(float(lf[0]))
    lr_hist, lf_hist = np.array(lr_hist), np.array(lf_hist)
    assert lr_hist[-1] < 0.9 * lr_hist[0]                                        # it is actually learning
    np.testing.assert_allclose(lf_hist, lr_hist, rtol=tol)
    got = tr.state_dict_numpy()
    # Adam turns a gradient whose sign is rounding noise into a +-lr step, so single parameters may differ by a few lr;
    # the population must not: RMS drift against RMS movement, and the share of parameters off by more than 10 lr
    mv = np.concatenate([(tp[k].detach().numpy() - params[k]).ravel() for k in params])
    dr = np.concatenate([(got[k] - tp[k].detach().numpy()).ravel() for k in params])
    rms_moved, rms_drift = float(np.sqrt((mv ** 2).mean())), float(np.sqrt((dr ** 2).mean()))
    assert rms_moved > 0.01, rms_moved
    # bf16x3: gradients carry ~1e-4 of rounding, which Adam's sign-like early steps amplify over 120 steps (measured 0.023)
    assert rms_drift < {"bf16": 0.08, "bf16x3": 0.03, "fp32": 0.02}[precision] * rms_moved, (rms_moved, rms_drift)
    assert (np.abs(dr) > 10 * lr).mean() < (0.02 if precision == "bf16" else 2e-3), float((np.abs(dr) > 10 * lr).mean())
    print(f"trajectory[{model},{precision}]: rms drift / rms moved = {rms_drift / rms_moved:.4f}")


@pytest.mark.parametrize("y_dim", [1, 513])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_persistent_tile_loop_equals_the_sum_of_its_halves(precision, y_dim):
    """20 000 frames = 625 tiles run more than one tile per workgroup (the 8-wave kernel holds 256 workgroups); four 5 000-frame steps
    (157 tiles) do not: same gradient.  y_dim 513 runs the label prefetch across tiles (the next tile's labels are requested during
    this tile's backward phases and stay in registers until its BL1X)."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 11)
    B = 20000
    x, y, e = gu.make_batch(dims, B, 12)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def grads(xs, ys, es):
        tr = trainer.Trainer("M2", dims, params, batch=len(xs), precision=precision)
        assert (tr.plan.rows_grid < -(-len(xs) // 32)) == (len(xs) == B)          # only the full batch loops over tiles
        losses = tr.step(t(xs), t(ys), t(es)).cpu().numpy().astype(np.float64)
        return tr.grads_numpy(), losses
    full, lfull = grads(x, y, e)
    q = B // 4
    parts = [grads(x[i * q:(i + 1) * q], y[i * q:(i + 1) * q], e[i * q:(i + 1) * q]) for i in range(4)]
    np.testing.assert_allclose(lfull, np.mean([p[1] for p in parts], axis=0), rtol=1e-5)
    for k in full:
        mean = 0.25 * sum(p[0][k].astype(np.float64) for p in parts)
        assert np.abs(full[k] - mean).max() <= 1e-4 * np.abs(mean).max() + 1e-12, k   # summation order differs (slices, parts)


@pytest.mark.parametrize("model,y_dim,B,precision", [("M2", 513, 1000, "bf16"), ("M2", 513, 33, "fp32"), ("M2_info", 1, 257, "bf16"),
                                                       ("M1", 0, 8192, "bf16"), ("M2", 1, 20000, "fp32"), ("M2", 513, 1000, "bf16x3"),
                                                       ("M2_info", 1, 257, "bf16x3"), ("M2", 1, 20000, "bf16x3"),
                                                       ("M2", 513, 20000, "bf16x3"), ("M2", 513, 20000, "bf16"), ("M2", 513, 19990, "bf16x3")])
@pytest.mark.parametrize("gather", [False, True])
def test_kernels_stay_inside_their_buffers(model, y_dim, B, precision, gather):
    """Guard bands around the workspace, the parameter / moment buffers and the loss scalars survive train steps
    (stash tiles, gradient slabs, weight copies and partial sums are all addressed by hand in the kernels)."""
    import ctypes
    N = importlib.import_module("disentangled-vae_amd.native")
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    tr = trainer.Trainer(model, dims, batch=B, precision=precision, seed=1)
    G = 1 << 16                                              # 64 KiB of guard on each side

    def guarded(nbytes, dtype):
        raw = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        return raw, raw[G:G + nbytes].view(dtype)
    raw_ws, ws = guarded(tr.plan.workspace_bytes, torch.uint8)
    raws = {"ws": raw_ws}
    for name in ("params", "m", "v"):
        raw, view = guarded(4 * tr.plan.n_params, torch.float32)
        view.copy_(getattr(tr, name))
        setattr(tr, name, view)
        raws[name] = raw
    raw_l, losses = guarded(4 * tr.losses.numel(), torch.float32)
    tr.losses = losses
    raws["losses"] = raw_l
    tr.ws = ws
    go = tr.plan.grad_offset_bytes
    tr.flat_grad = tr.ws[go:go + 4 * tr.plan.n_params].view(torch.float32)
    N.check(tr.lib.dvae_train_init(ctypes.byref(tr.plan), N.ptr(tr.params), N.ptr(tr.ws), N.stream()), "dvae_train_init")
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    n = B + 1000 if gather else B                              # gather: the step's frames are rows of a larger frame store
    x = torch.rand(n, 513, device="cuda", generator=g) + 0.01
    y = (torch.rand(n, y_dim, device="cuda", generator=g) > 0.5).float() if y_dim else None
    rows = torch.randperm(n, device="cuda", generator=g)[:B].contiguous() if gather else None
    for _ in range(3):
        out = tr.step(x, y, rows=rows)
    tr.evaluate(x, y, rows=rows)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    for name, raw in raws.items():
        assert bool((raw[:G] == 0xA5).all()) and bool((raw[-G:] == 0xA5).all()), f"{name}: guard band overwritten"


@pytest.mark.parametrize("model,y_dim,B", [("M2", 513, 8192), ("M1", 0, 1000), ("M2", 1, 20000), ("M2", 513, 33)])
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_weight_gradients_from_raw_inputs_equal_the_stash_path(model, y_dim, B, precision):
    """DVAE_RAW_INPUTS=1 (opt-in): the weight-gradient kernel reads x / y from the fp32 input matrices (dword loads for ragged tiles,
    LDS-staged transposition for full ones) and the rows kernel writes no x / y stash.  Same operand values, same summation order:
    the gradients equal the default path's bit for bit."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 31)
    x, y, e = gu.make_batch(dims, B, 32)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    out = {}
    os.environ["DVAE_WGRAD"] = "wg4"            # the workgroup k-split kernel on both sides (steps of <= 128 frames default to the 2 x 2 kernel)
    try:
        for raw in (False, True):
            if raw:
                os.environ["DVAE_RAW_INPUTS"] = "1"
            try:
                tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
                losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
                out[raw] = (losses, tr.grads_numpy())
            finally:
                os.environ.pop("DVAE_RAW_INPUTS", None)
    finally:
        os.environ.pop("DVAE_WGRAD", None)
    np.testing.assert_array_equal(out[False][0], out[True][0])
    for k in out[False][1]:
        np.testing.assert_array_equal(out[False][1][k], out[True][1][k], err_msg=k)


@pytest.mark.parametrize("y_dim,B", [(513, 1000), (1, 300), (513, 20000)])
def test_label_lo_plane_on_demand_equals_always(y_dim, B, monkeypatch):
    """bf16x3: a label tile that one bf16 plane holds exactly (binary VAD / IBM labels) stores and multiplies no lo plane; the
    weight-gradient kernel reads the label lo plane only in launches where some tile needs it.  Sequence of steps with real-valued
    labels everywhere, in ONE tile, nowhere, and in another tile again (stale lo planes of tile slots that turned binary must
    not be read): losses and parameters equal the always-both-planes path (DVAE_YLO_ALWAYS=1) bit for bit, and the
    real-valued-label gradients match the float64 oracle within the bound of test_fused_step_vs_oracle (5e-5 of every tensor's maximum;
    round 3 had loosened this to 4e-4 for the 20 000-frame case: that was the L1 x GEMM's operand precision, fixed in round 4)."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 51)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(3)
    batches = []
    for step, pattern in enumerate(["all", "one", "none", "other", "none"]):
        x, y, e = gu.make_batch(dims, B, 60 + step)
        soft = rng.random(y.shape).astype(np.float32)                     # labels in (0, 1) with full fp32 mantissas
        if pattern == "all":
            y = soft
        elif pattern == "one":
            y[96:128] = soft[96:128]                                     # tile 3 only
        elif pattern == "other":
            y[-20:] = soft[-20:]                                         # the last (ragged or full) tile only
        batches.append((x, y, e))
    res = {}
    for always in (False, True):
        if always:
            monkeypatch.setenv("DVAE_YLO_ALWAYS", "1")
        tr = trainer.Trainer("M2", dims, params, batch=B, precision="bf16x3")
        out = []
        for x, y, e in batches:
            losses = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
            out.append((losses, tr.grads_numpy(), tr.state_dict_numpy()))
        res[always] = out
        monkeypatch.delenv("DVAE_YLO_ALWAYS", raising=False)
    for (la, ga, pa), (lb, gb, pb) in zip(res[False], res[True]):
        np.testing.assert_array_equal(la, lb)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    x, y, e = batches[0]
    out, grads, _ = _oracle_step("M2", dims, params, x.astype(np.float64), y.astype(np.float64), e.astype(np.float64))
    np.testing.assert_allclose(res[False][0][0], [out["loss"], out["recon"], out["kl"]], rtol=1e-5)
    for k in grads:
        assert _relmax(res[False][0][1][k], np.asarray(grads[k], np.float64).reshape(res[False][0][1][k].shape)) < x3_grad_bound(k), k


@needs_diag
@pytest.mark.parametrize("model,y_dim,B", [("M2", 513, 8192), ("M1", 0, 8192), ("M2", 1, 1000), ("M2", 513, 33), ("M2", 513, 20000)])
def test_twelve_wave_rows_kernel_vs_oracle(model, y_dim, B, monkeypatch):
    """Diagnostic builds, opt-in (DVAE_ROWS=3; measured slower, csrc/train_rows3.hip): the layer chain N-split over eight GEMM waves on
    16x16x32 MFMA tiles.  Same bars as the product kernel under the split-bf16 policy: losses 1e-5, every gradient tensor inside
    x3_grad_bound; the plan names the kernel that ran."""
    monkeypatch.setenv("DVAE_ROWS", "3")
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 11)
    x, y, e = gu.make_batch(dims, B, 12)
    out, grads, _ = _oracle_step(model, dims, params, x.astype(np.float64), None if y is None else y.astype(np.float64), e.astype(np.float64))
    tr = trainer.Trainer(model, dims, params, batch=B, precision="bf16x3")
    assert tr.plan.rows_kernel == 3
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for _ in range(2):                                              # (the second step: the 16-row-tile weight copies after an Adam refresh)
        losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
        assert np.all(np.isfinite(losses))
        if _ == 0:
            np.testing.assert_allclose(losses, [out["loss"], out["recon"], out["kl"]], rtol=1e-5)
            g = tr.grads_numpy()
            for k in grads:
                assert _relmax(g[k], np.asarray(grads[k], np.float64).reshape(g[k].shape)) < x3_grad_bound(k), k
    monkeypatch.setenv("DVAE_ROWS", "2")
    tr2 = trainer.Trainer(model, dims, params, batch=B, precision="bf16x3")
    assert tr2.plan.rows_kernel == 2
    for _ in range(2):
        l2 = tr2.step(t(x), t(y), t(e)).cpu().numpy()
    np.testing.assert_allclose(losses, l2, rtol=2e-6)               # second-step losses: both kernels' parameter updates agree


@needs_diag
@pytest.mark.parametrize("model,y_dim,B,precision", [("M2", 513, 8192, "bf16x3"), ("M2", 513, 3000, "fp32"), ("M2", 1, 5000, "bf16x3"),
                                                       ("M1", 0, 8192, "bf16"), ("M2_info", 1, 8192, "bf16x3"), ("M2", 513, 20000, "bf16x3")])
def test_optimizer_step_folded_into_the_weight_gradient_launch_equals_its_own_launch(model, y_dim, B, precision, monkeypatch):
    """Diagnostic builds, opt-in (DVAE_FOLD_APPLY=1; measured slower): dvae_train_step runs Adam + the weight-copy refresh +
    the loss scalars in the tail of the weight-gradient kernel (two launches per step) whenever that kernel's grid is one resident
    round of workgroups; unset or 0 = the three-launch step.  Same slab sums in the same order, same element arithmetic: losses,
    gradients, parameters and both Adam moments are equal bit for bit over a run of steps (ragged last tiles and partial k-slices
    included).  Whether the tail really ran is read off the profile (no apply launch); cases whose grid cannot fold are named."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 71)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batches = [gu.make_batch(dims, B, 80 + i) for i in range(4)]
    res = {}
    applies = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("DVAE_FOLD_APPLY", fold)
        tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
        tr.profile(True)
        out = []
        for x, y, e in batches:
            losses = tr.step(t(x), t(y) if y_dim else None, t(e)).cpu().numpy().copy()
            out.append((losses, tr.grads_numpy(), tr.state_dict_numpy(), tr.m.cpu().numpy().copy(), tr.v.cpu().numpy().copy()))
        applies[fold] = tr.profile_read()["apply"][1]
        tr.profile(False)
        res[fold] = out
    assert applies["0"] == len(batches)
    folded = applies["1"] == 0
    # (the tail needs ks > 1, a grid within the CU count and <= 120 blocks; when it cannot run, both arms are the three-launch step)
    print(f"fold[{model},y{y_dim},B{B},{precision}]: the optimizer tail {'ran' if folded else 'did NOT run (grid cannot fold)'}")
    assert folded or (model, y_dim, B, precision) != ("M2", 513, 8192, "bf16x3"), "the headline configuration must fold"
    for (la, ga, pa, ma, va), (lb, gb, pb, mb, vb) in zip(res["1"], res["0"]):
        assert np.all(np.isfinite(la))
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(va, vb)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


@needs_diag
@pytest.mark.parametrize("model,y_dim,B,precision", [("M2", 513, 8192, "bf16x3"), ("M2", 1, 5000, "bf16x3"), ("M1", 0, 8192, "bf16"),
                                                       ("M2", 513, 20000, "bf16x3"), ("M2", 513, 8192, "bf16"), ("M1", 0, 4096, "bf16x3")])
def test_deferred_optimizer_step_equals_the_three_launch_step(model, y_dim, B, precision, monkeypatch):
    """Round 4 (opt-in, DVAE_DEFER_APPLY=1): dvae_train_step_deferred -- two launches per step; the Adam update of step n runs on the chain waves of step n + 1's rows
    kernel (32 x 32 parameter tiles per wave, write-through stores, arrival counters, sc1 weight loads), the loss scalars come from the
    rows kernel's last workgroup -- against the three-launch step (DVAE_DEFER_APPLY=0): losses, gradients, parameters and both Adam
    moments equal bit for bit after every one of five steps (reading parameters flushes the pending update through apply_kernel, so
    the in-kernel form AND the flush are both compared), including a batch of more tiles than workgroups and a ragged last tile."""
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=16, h_dim=(128, 128))
    params = gu.make_params(model, dims, 71)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batches = [gu.make_batch(dims, B, 80 + i) for i in range(5)]
    res = {}
    for defer in ("1", "0"):
        monkeypatch.setenv("DVAE_DEFER_APPLY", defer)
        tr = trainer.Trainer(model, dims, params, batch=B, precision=precision)
        out = []
        for i, (x, y, e) in enumerate(batches):
            losses = tr.step(t(x), t(y) if y_dim else None, t(e))
            if defer == "1":
                import ctypes
                can = tr.lib.dvae_train_can_defer(ctypes.byref(tr.plan), N.ptr(tr.ws))
                assert tr.lib.dvae_train_pending(N.ptr(tr.ws)) == can, "a step that can defer its update did not (or the reverse)"
                assert can == 1 or (model, y_dim, B) != ("M2", 513, 8192), "the headline configuration must defer"
            if i in (1, 4):                                       # two of the five steps: parameters read after the step (= a flush)
                out.append((losses.cpu().numpy().copy(), tr.grads_numpy(), tr.state_dict_numpy(), tr.m.cpu().numpy().copy(), tr.v.cpu().numpy().copy()))
            else:                                                 # the others: the update stays pending and runs inside the next rows kernel
                out.append((losses.cpu().numpy().copy(), tr.grads_numpy(), None, None, None))
        res[defer] = out
    for (la, ga, pa, ma, va), (lb, gb, pb, mb, vb) in zip(res["1"], res["0"]):
        assert np.all(np.isfinite(la))
        np.testing.assert_array_equal(la, lb)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
        if pa is not None:
            np.testing.assert_array_equal(ma, mb)
            np.testing.assert_array_equal(va, vb)
            for k in pa:
                np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


@needs_diag
def test_deferred_optimizer_step_with_forks_evaluation_and_state_dict():
    """The pending update is applied before anything else looks at the parameters: a fork (another batch size over the same parameters)
    stepping in between, evaluate(), load_state_dict() -- the sequence equals the same sequence without deferral bit for bit."""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 72)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bA = [gu.make_batch(dims, 8192, 90 + i) for i in range(3)]
    bB = [gu.make_batch(dims, 1000, 95 + i) for i in range(2)]
    res = {}
    for defer in ("1", "0"):
        os.environ["DVAE_DEFER_APPLY"] = defer
        try:
            tr = trainer.Trainer("M2", dims, params, batch=8192, precision="bf16x3")
            fk = tr.fork(1000)
            log = []
            log.append(tr.step(*map(t, bA[0])).cpu().numpy().copy())
            log.append(fk.step(*map(t, bB[0])).cpu().numpy().copy())            # small batch: cannot defer (falls back), must see A's update
            log.append(tr.step(*map(t, bA[1])).cpu().numpy().copy())
            log.append(tr.evaluate(*map(t, bA[2])).cpu().numpy().copy())
            sd = tr.state_dict()
            tr.load_state_dict(sd)
            log.append(tr.step(*map(t, bA[2])).cpu().numpy().copy())
            log.append(fk.evaluate(*map(t, bB[1])).cpu().numpy().copy())
            res[defer] = (log, tr.state_dict_numpy(), tr.m.cpu().numpy().copy())
        finally:
            os.environ.pop("DVAE_DEFER_APPLY", None)
    for a, b in zip(res["1"][0], res["0"][0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res["1"][2], res["0"][2])
    for k in res["1"][1]:
        np.testing.assert_array_equal(res["1"][1][k], res["0"][1][k], err_msg=k)


@needs_diag
def test_deferred_optimizer_step_never_hangs_when_its_wait_runs_out(monkeypatch):
    """The arrival wait in front of the first weight load is bounded by wall time: with a bound of zero a workgroup that polls before the
    others have arrived gives up at once -- the launch completes, the sticky error word turns the loss into NaN (the trainer is to be
    discarded), nothing waits forever.  (Every workgroup is resident, so with the default bound of 2 s the wait is microseconds.)"""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 73)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, y, e = gu.make_batch(dims, 8192, 99)
    monkeypatch.setenv("DVAE_DEFER_TIMEOUT_MS", "0")
    monkeypatch.setenv("DVAE_DEFER_APPLY", "1")
    tr = trainer.Trainer("M2", dims, params, batch=8192, precision="bf16x3")
    first = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()                     # nothing pending yet: no wait
    assert np.all(np.isfinite(first))
    seen_nan = False
    for _ in range(4):
        l = tr.step(t(x), t(y), t(e)).cpu().numpy().copy()
        seen_nan = seen_nan or bool(np.isnan(l[0]))
    torch.cuda.synchronize()
    assert seen_nan, "a zero bound must trip on a 256-workgroup grid"


@needs_diag
def test_folded_optimizer_tail_never_hangs_when_its_wait_runs_out(monkeypatch):
    """The wait of the folded tail (a workgroup waiting for the other slices of its parameter block) is bounded: with a bound of zero
    polls every workgroup that arrives early gives up at once -- the launch completes, the sticky error word turns the step's loss
    into NaN (parameters are then partly updated: the trainer is to be discarded), and nothing waits forever."""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 5)
    x, y, e = gu.make_batch(dims, 8192, 6)
    t = lambda a: torch.from_numpy(a).cuda()
    monkeypatch.setenv("DVAE_FOLD_APPLY", "1")
    monkeypatch.setenv("DVAE_FOLD_MAX_POLLS", "0")
    tr = trainer.Trainer("M2", dims, params, batch=8192, precision="bf16x3")
    losses = tr.step(t(x), t(y), t(e)).cpu().numpy()
    assert np.isnan(losses[0])
    monkeypatch.delenv("DVAE_FOLD_MAX_POLLS")
    tr2 = trainer.Trainer("M2", dims, params, batch=8192, precision="bf16x3")      # a fresh workspace is unaffected
    assert np.all(np.isfinite(tr2.step(t(x), t(y), t(e)).cpu().numpy()))


def test_operand_range_of_the_split_fp16_planes_is_checked(monkeypatch):
    """bf16x3 multiplies the x block of encoder layer 1 on split-FP16 planes with fixed scales (finite for |x| <= 5.2e5, |w| <= 1023;
    csrc/fused_tiles.hpp: X16).  The reference (fp32 torch) takes any float32 -- spectra of int16-scaled audio reach 1e9 -- so a batch or a
    weight beyond the range is an ERROR on the trainer's first step, with the way out in the message; the fp32 policy takes the same batch;
    with the check switched off (DVAE_RANGE_CHECK=0) the step runs and its losses are not finite (what the check is there to prevent)."""
    dims = dict(x_dim=513, y_dim=513, z_dim=16, h_dim=(128, 128))
    params = gu.make_params("M2", dims, 3)
    x, y, e = gu.make_batch(dims, 256, 4)
    t = lambda a: torch.from_numpy(a).cuda()
    big = t(x) * 1.0e6
    tr = trainer.Trainer("M2", dims, params, batch=256, precision="bf16x3")
    with pytest.raises(ValueError, match="split-fp16"):
        tr.step(big, t(y), t(e))
    tr = trainer.Trainer("M2", dims, params, batch=256, precision="bf16x3")
    assert np.all(np.isfinite(tr.step(t(x), t(y), t(e)).cpu().numpy()[:3]))           # in range: fine, and checked only once
    wbig = {k: v.copy() for k, v in params.items()}
    wbig["encoder.hidden.0.weight"][3, 7] = 5000.0
    tr = trainer.Trainer("M2", dims, wbig, batch=256, precision="bf16x3")
    with pytest.raises(ValueError, match="layer-1 weights"):
        tr.step(t(x), t(y), t(e))
    tr = trainer.Trainer("M2", dims, params, batch=256, precision="fp32")
    assert np.all(np.isfinite(tr.step(big, t(y), t(e)).cpu().numpy()[:3]))
    monkeypatch.setenv("DVAE_RANGE_CHECK", "0")
    tr = trainer.Trainer("M2", dims, params, batch=256, precision="bf16x3")
    assert not np.all(np.isfinite(tr.step(big, t(y), t(e)).cpu().numpy()[:3]))

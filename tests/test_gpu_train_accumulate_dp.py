"""Data parallelism on the any-size fused train steps (disentangled-vae_amd/accumulate.py: AccumulatedStep with a process group): two
ranks sharing the one GPU, gloo in place of RCCL (the pattern of tests/test_gpu_fused.py:
test_two_rank_data_parallel_equals_single_process).  Functional checks, not a measurement of scaling.

One pair of workers runs every scenario for every geometry in one process each (three GPU processes with this one); the tests below
compare what the ranks sent back with single-process runs.
 (i)   one micro-batch of 48 per rank == a single trainer of batch 96, ksplit 2, bit for bit: rank r's slab is exactly twice slice r's
       slab of the single step (invB = fl(1 / 48) = 2 fl(1 / 96)), the two-operand sum of the exchange commutes, the scale 1 / 2 is exact.
 (ii)  two micro-batches of 32 per rank: replicas bit-identical; the exchanged gradient within GRAD_TOL of truth(case, 128); parameters
       after two steps within 4.1 lr of the single-process run -- Adam moves an element by at most about 1.002 lr in each of its first
       two steps, so two runs whose gradients differ in rounding can differ by twice that per step (the bound of the resident test).
 (iii) default noise: two ranks without eps_noise == the single trainer without eps_noise, bit for bit as in (i).
 (iv)  replicas_equal() is true, and false after one rank's parameter is perturbed through load_state_dict.
 (v)   a ONE-rank RCCL ("nccl") group in a process of its own: the reporting collectives on the backend the product runs on, which
       serves device tensors only."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import train_classifier_cases as cc
import train_generic_cases as gc
import train_info_cases as ic

pytestmark = pytest.mark.gpu
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")

DEV = "cuda:0"
LR = 1e-4
GEOMETRIES = {"generic": (1, 5, (48, 200)), "clf": ((48, 200), 2), "info": (3, 17, (129, 127))}
KINDS = list(GEOMETRIES)
NOISE_SEED = 5


def _make(mods, kind, B, ksplit, **kw):
    """mods: (G, C, I, gc, cc, ic) -- the worker imports its own."""
    Gm, Cm, Im, gcm, ccm, icm = mods
    case = GEOMETRIES[kind]
    if kind == "generic":
        return Gm.GenericTrainer(gcm.model_of(case), gcm.dims_of(case), gcm.inputs(case, 1)[0], batch=B, device=DEV, lr=LR, ksplit=ksplit, **kw)
    if kind == "clf":
        return Cm.ClassifierTrainer(ccm.dims_of(case), params=ccm.params_of(case), batch=B, device=DEV, lr=LR, ksplit=ksplit, **kw)
    a, b, g = icm.WEIGHTS
    return Im.InfoTrainer(icm.dims_of(case), params=icm.params_of(case), batch=B, device=DEV, lr=LR, alpha=a, beta=b, gamma=g, ksplit=ksplit, **kw)


def _inputs(mods, kind, B):
    return {"generic": mods[3], "clf": mods[4], "info": mods[5]}[kind].inputs(GEOMETRIES[kind], B)[1:]


def _worker(rank, world, port, q):
    import sys, traceback
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    try:
        import torch.distributed as dist
        import train_classifier_cases as ccm, train_generic_cases as gcm, train_info_cases as icm
        mods = tuple(importlib.import_module("disentangled-vae_amd." + n) for n in ("trainer_generic", "trainer_classifier", "trainer_info")) \
            + (gcm, ccm, icm)
        A = importlib.import_module("disentangled-vae_amd.accumulate")
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ.pop("DVAE_ALLREDUCE", None)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist.group.WORLD
        dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)
        out = {}
        for kind in KINDS:
            res = {}
            # (i) one micro-batch of 48 per rank, two steps on the same frames
            tr = _make(mods, kind, 48, 1)
            acc = A.AccumulatedStep(tr, pg)
            mine = tuple(None if a is None else dev(a[48 * rank:48 * rank + 48]) for a in _inputs(mods, kind, 96))
            for s in range(2):
                acc.micro(*mine)
                acc.apply()
                if s == 0:
                    res["i_grads"], res["i_losses"] = acc.grads_numpy(), acc.global_losses().numpy().copy()
                    res["i_counts"] = acc.global_counts().numpy().copy()
            res["i_state"] = dict(params=tr.state_dict_numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy())
            # (iv)
            res["iv_equal"] = acc.replicas_equal()
            if rank == 1:
                name = tr.names[0]
                t = tr.state_dict()[name]
                t.view(-1)[0] += 1.0
                tr.load_state_dict({name: t}, strict=False)
            res["iv_after"] = acc.replicas_equal()
            # (ii) two micro-batches of 32 per rank
            tr = _make(mods, kind, 32, 0)
            acc = A.AccumulatedStep(tr, pg, micro_batches=[32, 32])
            all_ = _inputs(mods, kind, 128)
            for s in range(2):
                for k in range(2):
                    lo = 64 * rank + 32 * k
                    acc.micro(*(None if a is None else dev(a[lo:lo + 32]) for a in all_))
                acc.apply()
                if s == 0:
                    res["ii_grads"] = acc.grads_numpy()
            res["ii_params"], res["ii_equal"] = tr.state_dict_numpy(), acc.replicas_equal()
            # (iii) default noise
            if kind != "clf":
                tr = _make(mods, kind, 48, 1, seed=NOISE_SEED)
                acc = A.AccumulatedStep(tr, pg, micro_batches=[48])
                for s in range(2):
                    acc.micro(*mine[:2])
                    acc.apply()
                res["iii_params"] = tr.state_dict_numpy()
            out[kind] = res
        # unequal frame counts across the ranks are refused on every rank, before anything touches the device
        try:
            A.AccumulatedStep(tr, pg, micro_batches=[48 + rank])
            out["unequal"] = "accepted"
        except ValueError as e:
            out["unequal"] = str(e)
        q.put((rank, out, None))
        dist.destroy_process_group()
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@functools.lru_cache(maxsize=None)
def _ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35000 + (os.getpid() * 3 + 1) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = []
    for _ in procs:
        got.append(q.get(timeout=300))
        if got[-1][2] is not None:
            for pr in procs:
                pr.kill()
            raise AssertionError(f"rank {got[-1][0]} failed:\n{got[-1][2]}")
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    got.sort(key=lambda t: t[0])
    return got[0][1], got[1][1]


MODS = (G, C, I, gc, cc, ic)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _single(kind, B, ksplit, seed=None, noise=True):
    tr = _make(MODS, kind, B, ksplit, **({} if seed is None else {"seed": seed}))
    batch = tuple(_dev(a) for a in _inputs(MODS, kind, B))
    if not noise:
        batch = batch[:2]
    out = {}
    for s in range(2):
        losses = tr.step(*batch).cpu().numpy().copy()
        if s == 0:
            out.update(grads=tr.grads_numpy(), losses=losses, counts=tr.counts.cpu().numpy().copy() if kind == "clf" else None)
    out.update(params=tr.state_dict_numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy(), ksplit=tr.plan.ksplit, slice_frames=tr.plan.slice_frames)
    return out


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_two_ranks_of_one_micro_batch_equal_the_single_trainer_bit_for_bit(kind):
    r0, r1 = (r[kind] for r in _ranks())
    one = _single(kind, 96, 2)
    assert one["ksplit"] == 2 and one["slice_frames"] == 48
    for k in one["params"]:
        assert _same(r0["i_state"]["params"][k], r1["i_state"]["params"][k]), k                 # replicas identical
        assert _same(r0["i_state"]["params"][k], one["params"][k]), k
        assert _same(r0["i_grads"][k], one["grads"][k]) and _same(r1["i_grads"][k], one["grads"][k]), k
    for part in ("m", "v"):
        assert _same(r0["i_state"][part], one[part]) and _same(r1["i_state"][part], one[part]), part
    mod = MODS[3 + KINDS.index(kind)]
    for r in (r0, r1):
        le = mod.loss_err(r["i_losses"][0] if kind == "clf" else r["i_losses"], one["losses"][0] if kind == "clf" else one["losses"])
        print(f"{kind}: mean of the ranks' losses against the single step's: {le:.2e}")
        assert le <= mod.LOSS_RTOL
    if kind == "clf":
        assert np.array_equal(r0["i_counts"], one["counts"]) and np.array_equal(r1["i_counts"], one["counts"])


@pytest.mark.parametrize("kind", KINDS)
def test_two_ranks_of_two_micro_batches(kind):
    r0, r1 = (r[kind] for r in _ranks())
    assert r0["ii_equal"] and r1["ii_equal"]
    mod = MODS[3 + KINDS.index(kind)]
    ge, name = mod.grad_err(r0["ii_grads"], mod.truth(GEOMETRIES[kind], 128)[1][0])
    one = _single(kind, 128, 0)
    worst = 0.0
    for k in one["params"]:
        assert _same(r0["ii_params"][k], r1["ii_params"][k]) and _same(r0["ii_grads"][k], r1["ii_grads"][k]), k
        worst = max(worst, float(np.max(np.abs(r0["ii_params"][k].astype(np.float64) - one["params"][k]))))
    print(f"{kind}: exchanged gradient against float64 {ge:.2e} ({name}); parameters after two steps off the single run by {worst / LR:.3f} lr")
    assert ge <= mod.GRAD_TOL, (ge, name)
    assert worst <= 4.1 * LR


@pytest.mark.parametrize("kind", ["generic", "info"])
def test_two_ranks_default_noise_equal_the_single_trainer(kind):
    r0, r1 = (r[kind] for r in _ranks())
    one = _single(kind, 96, 2, seed=NOISE_SEED, noise=False)
    assert one["ksplit"] == 2 and one["slice_frames"] == 48
    for k in one["params"]:
        assert _same(r0["iii_params"][k], one["params"][k]) and _same(r1["iii_params"][k], one["params"][k]), k


def test_replicas_equal_sees_a_perturbed_rank():
    for r in _ranks():
        for kind in KINDS:
            assert r[kind]["iv_equal"] is True and r[kind]["iv_after"] is False, kind
        assert "same number of frames" in r["unequal"] and "[48, 49]" in r["unequal"], r["unequal"]


def _rccl_worker(port, q):
    import sys, traceback
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here)); sys.path.insert(0, here)
    try:
        import torch.distributed as dist
        import train_classifier_cases as ccm
        Cm = importlib.import_module("disentangled-vae_amd.trainer_classifier")
        A = importlib.import_module("disentangled-vae_amd.accumulate")
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ.pop("DVAE_ALLREDUCE", None); os.environ.pop("LOCAL_RANK", None)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
        case = GEOMETRIES["clf"]
        _, x, y = ccm.inputs(case, 48)
        tr = Cm.ClassifierTrainer(ccm.dims_of(case), params=ccm.params_of(case), batch=48, device=DEV, lr=LR)
        acc = A.AccumulatedStep(tr, dist.group.WORLD)
        dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        acc.micro(dev(x), dev(y))
        own = acc.apply().cpu().numpy().copy()
        gl, gc_ = acc.global_losses(), acc.global_counts()
        q.put((dict(own=own, losses=gl.numpy().copy(), counts=gc_.numpy().copy(), own_counts=acc.counts.cpu().numpy().copy(),
                    devices=(str(gl.device), str(gc_.device)), equal=acc.replicas_equal(), backend=dist.get_backend()), None))
        dist.destroy_process_group()
    except Exception:
        q.put((None, traceback.format_exc()))


def test_reporting_collectives_on_an_rccl_group():
    """The product backend: a one-rank RCCL ("nccl") group on the GPU.  RCCL serves device tensors only, so global_losses(),
    global_counts() and replicas_equal() must hand it device tensors (a host tensor raises "No backend type associated with device
    type cpu"); one rank's mean and sum are its own values, handed back on the host."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=_rccl_worker, args=(36000 + (os.getpid() * 3 + 2) % 2000, q))
    pr.start()
    res, err = q.get(timeout=300)
    assert err is None, err
    pr.join(timeout=60)
    assert pr.exitcode == 0
    assert res["backend"] == "nccl" and res["devices"] == ("cpu", "cpu") and res["equal"] is True
    assert np.array_equal(res["losses"], res["own"]) and np.array_equal(res["counts"], res["own_counts"]) and res["counts"].sum() == 96

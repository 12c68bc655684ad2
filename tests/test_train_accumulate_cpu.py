"""Host-side refusals of gradient accumulation / data parallelism on the any-size train steps: the six entry points
dvae_train_{generic,clf,info}_{reduce,apply_flat} (include/dvae_train.h) and accumulate.AccumulatedStep.  No GPU: every refusal comes
before anything touches the device, so the pointers handed over are never dereferenced (non-null, 16-byte aligned fakes)."""
import ctypes
import importlib
import math

import pytest
import torch

native = importlib.import_module("disentangled-vae_amd.native")
T = importlib.import_module("disentangled-vae_amd.trainer")
G = importlib.import_module("disentangled-vae_amd.trainer_generic")
C = importlib.import_module("disentangled-vae_amd.trainer_classifier")
I = importlib.import_module("disentangled-vae_amd.trainer_info")
A = importlib.import_module("disentangled-vae_amd.accumulate")

E_BADARG = 1001
FAKE = ctypes.c_void_p(0x10000)          # never dereferenced
DIMS = dict(x_dim=513, y_dim=3, z_dim=17, h_dim=(129, 127))
HYPER = (1e-4, 0.9, 0.999, 1e-8)


def _err():
    return native.load().dvae_last_error().decode()


def _plans():
    return {"generic": G.make_plan("M2", DIMS, 48), "clf": C.make_plan([513, [48, 200], 2], 48), "info": I.make_plan(DIMS, 48)}


def _reduce(kind, plan, ws=FAKE, flat=FAKE, accumulate=0, weight=1.0, losses=FAKE, counts=FAKE, plan_ptr=True):
    lib = native.load()
    p = ctypes.byref(plan) if plan_ptr else None
    fn = getattr(lib, f"dvae_train_{kind}_reduce")
    if kind == "clf":
        return fn(p, ws, flat, accumulate, weight, losses, counts, None)
    return fn(p, ws, flat, accumulate, weight, losses, None)


def _apply_flat(kind, plan, params=FAKE, m=FAKE, v=FAKE, ws=FAKE, flat=FAKE, step=1, scale=1.0, plan_ptr=True):
    fn = getattr(native.load(), f"dvae_train_{kind}_apply_flat")
    return fn(ctypes.byref(plan) if plan_ptr else None, params, m, v, ws, flat, step, *HYPER, scale, None)


@pytest.mark.parametrize("kind", ["generic", "clf", "info"])
def test_reduce_refuses_bad_arguments(kind):
    plan = _plans()[kind]
    assert _reduce(kind, plan, plan_ptr=False) == E_BADARG and "null plan" in _err()
    for kw in (dict(ws=None), dict(flat=None), dict(losses=None)) + ((dict(counts=None),) if kind == "clf" else ()):
        assert _reduce(kind, plan, **kw) == E_BADARG and "null pointer" in _err(), kw
    assert _reduce(kind, plan, flat=ctypes.c_void_p(0x10004)) == E_BADARG and "16-byte" in _err()
    for acc in (2, -1):
        assert _reduce(kind, plan, accumulate=acc) == E_BADARG and "accumulate" in _err(), acc
    for w in (math.nan, math.inf, -math.inf):
        assert _reduce(kind, plan, weight=w) == E_BADARG and "finite" in _err(), w
    plan.workspace_bytes += 256
    assert _reduce(kind, plan) == E_BADARG and "changed" in _err()
    plan.workspace_bytes -= 256
    plan.ksplit += 1
    assert _reduce(kind, plan) == E_BADARG and "changed" in _err()


@pytest.mark.parametrize("kind", ["generic", "clf", "info"])
def test_apply_flat_refuses_bad_arguments(kind):
    plan = _plans()[kind]
    assert _apply_flat(kind, plan, plan_ptr=False) == E_BADARG and "null plan" in _err()
    for name in ("params", "m", "v", "ws", "flat"):
        assert _apply_flat(kind, plan, **{name: None}) == E_BADARG and "null pointer" in _err(), name
    assert _apply_flat(kind, plan, step=0) == E_BADARG and "1-based" in _err()
    for s in (math.nan, math.inf):
        assert _apply_flat(kind, plan, scale=s) == E_BADARG and "finite" in _err(), s
    plan.n_params += 64
    assert _apply_flat(kind, plan) == E_BADARG and "changed" in _err()


def _host_trainer(cls, plan, B=48):
    """A trainer object with host state only (no device, no library call): what AccumulatedStep reads before its first launch."""
    tr = cls.__new__(cls)
    tr.plan, tr.B, tr.device, tr.seed = plan, B, torch.device("cpu"), 0
    tr._shared = {"step_count": 0, "version": 0}
    tr._params = torch.zeros(plan.n_params)
    tr.losses = torch.zeros(1 if cls is C.ClassifierTrainer else 3)
    tr.names = []
    return tr


def test_accumulated_step_refusals(monkeypatch):
    monkeypatch.delenv("DVAE_ALLREDUCE", raising=False)
    with pytest.raises(TypeError, match="resident"):
        A.AccumulatedStep(T.Trainer.__new__(T.Trainer))
    with pytest.raises(TypeError, match="resident"):
        A.AccumulatedStep(object())
    plans = _plans()
    tr = _host_trainer(G.GenericTrainer, plans["generic"])
    monkeypatch.setenv("DVAE_ALLREDUCE", "direct")
    with pytest.raises(NotImplementedError, match="process group"):
        A.AccumulatedStep(tr)
    monkeypatch.setenv("DVAE_ALLREDUCE", "rccl")
    with pytest.raises(ValueError, match="micro_batches"):
        A.AccumulatedStep(tr, micro_batches=[])
    acc = A.AccumulatedStep(tr)
    assert acc.micro_batches == [48] and acc.world == 1
    with pytest.raises(RuntimeError, match="no micro-batch pending"):
        acc.apply()
    other = _host_trainer(G.GenericTrainer, G.make_plan("M2", DIMS, 20), 20)            # same class, its own parameters: not a fork
    x = torch.zeros(20, 513)
    with pytest.raises(ValueError, match="fork"):
        acc.micro(x, torch.zeros(20, 3), torch.zeros(20, 17), trainer=other)
    with pytest.raises(ValueError, match="fork"):
        acc.micro(x, torch.zeros(20, 2), trainer=_host_trainer(C.ClassifierTrainer, plans["clf"]))
    with pytest.raises(RuntimeError, match="no micro-batch pending"):                    # the refused calls left nothing pending
        acc.apply()
    clf = A.AccumulatedStep(_host_trainer(C.ClassifierTrainer, plans["clf"]))
    with pytest.raises(ValueError, match="no noise"):
        clf.micro(torch.zeros(48, 513), torch.zeros(48, 2), eps_noise=torch.zeros(48, 1))


def test_default_noise_needs_the_announced_sizes():
    tr = _host_trainer(G.GenericTrainer, _plans()["generic"])
    acc = A.AccumulatedStep(tr, micro_batches=[48, 48])
    other = _host_trainer(G.GenericTrainer, G.make_plan("M2", DIMS, 20), 20)
    other._shared, other._params = tr._shared, tr._params                                # a fork, as far as the host can tell
    with pytest.raises(ValueError, match="announce"):
        acc.micro(torch.zeros(20, 513), torch.zeros(20, 3), trainer=other)


def test_grad_scale_is_exact_for_equal_power_of_two_splits():
    acc = A.AccumulatedStep(_host_trainer(G.GenericTrainer, _plans()["generic"]))
    assert acc._grad_scale([48, 48]) == 0.5 and acc._grad_scale([48] * 4) == 0.25 and acc._grad_scale([48]) == 1.0
    acc.world = 2
    assert acc._grad_scale([48, 48, 20]) == 48 / (2 * 116)


def test_constructor_refusals_are_still_pinned():
    ref = dict(x_dim=513, y_dim=1, z_dim=16, h_dim=(128, 128))
    wide = dict(x_dim=513, y_dim=1, z_dim=32, h_dim=(256, 64))
    with pytest.raises(NotImplementedError, match="data-parallel") as e:
        G.GenericTrainer("M2", dict(ref, y_dim=7), batch=8, world=2)
    assert "AccumulatedStep" in str(e.value)
    for kw in (dict(world=2), dict(process_group=object()), dict(precision="bf16")):
        with pytest.raises(NotImplementedError, match="fp32, one GPU") as e:
            I.make_info_trainer(wide, batch=8, **kw)
        assert "z_dim 1..128" in str(e.value)
    with pytest.raises(NotImplementedError, match="data-parallel") as e:
        I.make_info_trainer(ref, generic=True, batch=8, world=2)
    assert "AccumulatedStep" in str(e.value)


def test_rccl_rank_on_another_device_is_refused(monkeypatch):
    """A trainer on another device than the group's rank expects: refused at construction, before anything touches the device (the
    process group is a stand-in: only its backend, rank and size are asked for)."""
    import torch.distributed as dist
    A.check_rank_device("gloo", 1, "cpu")                                               # ranks of a test rig may share a device
    A.check_rank_device("nccl", 1, "cuda:1")
    A.check_rank_device("nccl", 5, "cuda:1", local_rank="1")                            # the launcher's LOCAL_RANK decides
    for dev, lr in (("cuda:0", None), ("cpu", None), ("cuda:1", "0")):
        with pytest.raises(ValueError, match="cannot share a device"):
            A.check_rank_device("nccl", 1, dev, local_rank=lr)
    monkeypatch.delenv("DVAE_ALLREDUCE", raising=False)
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_backend", lambda group=None: "nccl")
    monkeypatch.setattr(dist, "all_gather_object", lambda *a, **k: pytest.fail("a collective before the refusal"))
    with pytest.raises(ValueError, match="expects its trainer on cuda:1"):
        A.AccumulatedStep(_host_trainer(G.GenericTrainer, _plans()["generic"]), process_group=object())


def test_small_collectives_run_where_the_backend_serves_them(monkeypatch):
    """RCCL serves device tensors only, gloo gets host tensors: global_losses / global_counts hand the collective a tensor on
    collective_device(backend, trainer.device) and return host tensors."""
    import torch.distributed as dist
    assert A.collective_device("nccl", "cuda:3") == torch.device("cuda:3") and A.collective_device("gloo", "cuda:3") == torch.device("cpu")
    seen = []

    def all_reduce(t, op=None, group=None):
        seen.append(t.device)
        t.mul_(2)                                                                       # two ranks holding the same values
    monkeypatch.delenv("DVAE_ALLREDUCE", raising=False)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_backend", lambda group=None: "gloo")
    monkeypatch.setattr(dist, "all_gather_object", lambda out, obj, group=None: out.__setitem__(slice(None), [obj] * len(out)))
    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    acc = A.AccumulatedStep(_host_trainer(C.ClassifierTrainer, _plans()["clf"]), process_group=object())
    acc.losses.fill_(3.0)
    acc.counts.copy_(torch.tensor([1, 2, 3, 4]))
    want = []
    for backend in ("gloo", "nccl"):
        acc._backend = backend
        monkeypatch.setattr(A, "collective_device", lambda b, d: want.append(b) or torch.device("cpu"))
        assert acc.global_losses().tolist() == [3.0] and acc.global_counts().tolist() == [2, 4, 6, 8]
        assert acc.mean_over_ranks(torch.tensor([1.0, 5.0])).tolist() == [1.0, 5.0]
    assert want == ["gloo"] * 3 + ["nccl"] * 3 and seen == [torch.device("cpu")] * 6
    assert acc.losses.tolist() == [3.0] and acc.counts.tolist() == [1, 2, 3, 4]         # the step's own tensors are left alone

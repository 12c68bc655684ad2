"""Gradient accumulation and data parallelism for the fused train steps of any covered size (GenericTrainer, ClassifierTrainer,
InfoTrainer of any mode; include/dvae_train.h: dvae_train_*_reduce / _apply_flat; csrc/train_tables.hip: train_generic_reduce_kernel).

One optimizer step = K micro-batches and one apply:

    acc = AccumulatedStep(trainer, micro_batches=[B, B, B_tail])
    for x, y in ...:
        acc.micro(x, y)            # rows + weight gradients + reduce: three launches; the slabs are summed into one flat gradient
    losses = acc.apply()           # [all-reduce of the flat gradient over the process group,] one Adam step over every parameter

The stash of a step is sized by the micro-batch, not by the effective batch.  With a process group every rank runs its own micro-batches
and apply() exchanges the flat gradient once: one collective per optimizer step (RCCL on a GPU node; gloo, staged through the host, on
test rigs whose ranks share a GPU).  A power-of-two number of equal micro-batches reproduces one large step bit for bit (DESIGN 4a'''').
PyTorch is plumbing: buffers, the stream, the noise generator, the collective."""
import hashlib
import os

import numpy as np
import torch

from . import clip, dp
from .trainer_classifier import ClassifierTrainer
from .trainer_generic import GenericTrainer
from .trainer_info import InfoTrainer

_KINDS = (GenericTrainer, ClassifierTrainer, InfoTrainer)


def check_rank_device(backend, rank, device, local_rank=None):
    """An RCCL ("nccl") rank owns one GPU: its trainer must sit on cuda:<LOCAL_RANK> (the launcher's variable; without one, the rank
    itself).  Ranks of any other backend may share a device (gloo test rigs), so nothing is asked of them.  Host logic only."""
    if backend != "nccl":
        return
    want = int(local_rank) if local_rank is not None else int(rank)
    device = torch.device(device)
    if device.type != "cuda" or device.index != want:
        raise ValueError(f"rank {rank} of the process group expects its trainer on cuda:{want}, got {device} (RCCL ranks cannot share a device)")


def collective_device(backend, device):
    """Where a small tensor must live to go through a collective of `backend`: RCCL serves device tensors only -- the trainer's device
    --, every other backend (gloo) gets host tensors.  Host logic only."""
    return torch.device(device) if backend == "nccl" else torch.device("cpu")


class AccumulatedStep:
    """Wraps one trainer (and, through micro(trainer=...), its forks).  `micro_batches`: the frames of the micro-batches of one
    optimizer step on this rank, in order -- needed up front only for the default noise; defaults to [trainer.B]."""

    def __init__(self, trainer, process_group=None, micro_batches=None):
        if not isinstance(trainer, _KINDS):
            raise TypeError(f"AccumulatedStep wraps a GenericTrainer, ClassifierTrainer or InfoTrainer, not {type(trainer).__name__}: the resident "
                            "Trainer has its own data parallelism (Trainer(..., world=, process_group=))")
        if dp.exchange_mode() == "direct":
            raise NotImplementedError("DVAE_ALLREDUCE=direct (the in-kernel peer exchange) exists on the resident step only; AccumulatedStep "
                                      "exchanges the flat gradient through the process group (DVAE_ALLREDUCE=rccl)")
        self.trainer = trainer
        self.pg = process_group
        self.micro_batches = [int(b) for b in (micro_batches if micro_batches is not None else [trainer.B])]
        if not self.micro_batches or min(self.micro_batches) < 1:
            raise ValueError(f"micro_batches must name at least one micro-batch of at least one frame, got {self.micro_batches}")
        self.rank, self.world, self._backend = 0, 1, None
        if process_group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(process_group), dist.get_world_size(process_group)
            self._backend = dist.get_backend(process_group)
            check_rank_device(self._backend, self.rank, trainer.device, os.environ.get("LOCAL_RANK"))
            totals = self._gather_objects(sum(self.micro_batches))
            if len(set(totals)) != 1:
                raise ValueError(f"every rank must bring the same number of frames to an optimizer step, got {totals}")
        self._has_noise = not isinstance(trainer, ClassifierTrainer)
        self._has_counts = isinstance(trainer, ClassifierTrainer)
        P = trainer.plan.n_params
        self.flat = torch.zeros(P, dtype=torch.float32, device=trainer.device)        # the flat gradient accumulator, the plan's layout
        self._pending = []                                                             # frames of the micro-batches since the last apply()
        self._scale = 1.0                                                              # grad_scale of the last apply()
        nl = trainer.losses.numel()
        self._loss_sum = torch.zeros(nl, dtype=torch.float64, device=trainer.device)
        self._zero = torch.zeros(nl, dtype=torch.float64, device=trainer.device)
        self._count_sum = torch.zeros(4, dtype=torch.int64, device=trainer.device)
        self.losses = torch.zeros(nl, dtype=torch.float32, device=trainer.device)      # B_k-weighted mean of the last step's micro-batches
        self.counts = torch.zeros(4, dtype=torch.int64, device=trainer.device)         # this rank's counts of the last step (classifier)
        self._noise = None                                                             # (step, the [world sum B_k, z] tensor)

    # ---- noise ----
    def noise(self, step):
        """The [world * sum B_k, z_dim] noise of optimizer step `step`: what a single trainer of that batch size would draw
        (GenericTrainer.noise).  Rank r's micro-batch k takes its rows in the order (rank, micro-batch, frame)."""
        tr = self.trainer
        n = self.world * sum(self.micro_batches)
        g = torch.Generator(device=tr.device).manual_seed((tr.seed * 0x9E3779B97F4A7C15 + int(step)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randn((n, tr.z_dim), generator=g, device=tr.device, dtype=torch.float32)

    def _default_noise(self, B):
        k = len(self._pending)
        if self._pending != self.micro_batches[:k] or k >= len(self.micro_batches) or self.micro_batches[k] != B:
            raise ValueError(f"default noise needs the micro-batches of a step as announced (micro_batches={self.micro_batches}); "
                             f"got {self._pending + [B]}: pass eps_noise, or announce the sizes")
        step = self.trainer.step_count + 1
        if self._noise is None or self._noise[0] != step:
            self._noise = (step, self.noise(step))
        lo = self.rank * sum(self.micro_batches) + sum(self.micro_batches[:k])
        return self._noise[1][lo:lo + B]

    # ---- one micro-batch ----
    def micro(self, x, y=None, eps_noise=None, rows=None, trainer=None):
        """rows + weight-gradient + reduce launches for one micro-batch on `trainer` (the wrapped one, or a fork() of it with another
        batch size).  Returns that trainer's loss tensor (no host sync): what a plain step on the micro-batch would have reported."""
        main = self.trainer
        tr = main if trainer is None else trainer
        if tr is not main and not (type(tr) is type(main) and getattr(tr, "_shared", None) is main._shared and tr._params is main._params):
            raise ValueError("micro(trainer=...) takes the wrapped trainer or a fork() of it")
        if self._has_noise:
            if eps_noise is None:
                eps_noise = self._default_noise(tr.B)
        elif eps_noise is not None:
            raise ValueError("the classifier step takes no noise")
        first = not self._pending
        weight = 1.0 if first else tr.B / self._pending[0]
        if self._has_counts:
            losses = tr._micro(self.flat, 0 if first else 1, weight, x, y, rows)
            self._count_sum.copy_(tr.counts) if first else self._count_sum.add_(tr.counts)
        else:
            losses = tr._micro(self.flat, 0 if first else 1, weight, x, y, eps_noise, rows)
        if first:                                                                       # (float64 sums of B_k * losses: one small kernel a micro-batch)
            torch.add(self._zero, losses, alpha=float(tr.B), out=self._loss_sum)
        else:
            self._loss_sum.add_(losses, alpha=float(tr.B))
        self._pending.append(tr.B)
        return losses

    def _grad_scale(self, pending):
        return float(pending[0]) / (float(self.world) * float(sum(pending)))           # (doubles)

    # ---- the optimizer step ----
    def apply(self, max_norm=None):
        """[All-reduce,] one Adam step with grad_scale = B_0 / (world * sum B_k).  Returns the B_k-weighted mean of the micro-batch
        losses of this rank as a device tensor (no host sync).  max_norm: clip the global norm of the step's gradient (all tensors at
        once, torch.nn.utils.clip_grad_norm_'s rule) to it on the device, behind the all-reduce -- every rank sees the same flat
        gradient, forms the same coefficient and the replicas stay equal; one more launch, no host sync; a gradient that is not finite
        skips the update and is counted (grad_norm, skipped_step_count(); DESIGN 4a'''')."""
        if not self._pending:
            raise RuntimeError("apply() with no micro-batch pending: call micro() first")
        if max_norm is not None:
            max_norm = clip.check_max_norm(max_norm)
        if self.pg is not None:
            dp.allreduce_flat_(self.flat, self.pg)                                      # one collective per optimizer step
        self._scale = self._grad_scale(self._pending)
        if max_norm is None:
            self.trainer._apply_flat(self.flat, self._scale)
        else:
            self.trainer._apply_flat_clipped(self.flat, self._scale, max_norm)
        torch.div(self._loss_sum, float(sum(self._pending)), out=self._loss_sum)
        self.losses.copy_(self._loss_sum)
        self.counts.copy_(self._count_sum)
        self._pending = []
        return self.losses

    # ---- reading state ----
    @property
    def grad_norm(self):
        """Device float32 [total_norm, coef] of the last apply(max_norm=...): the norm before clipping and the factor applied (0: the
        step was skipped).  No host sync."""
        return self.trainer.grad_norm

    def skipped_step_count(self):
        """Clipped steps the device skipped for a non-finite gradient since the last call (reads and resets the counter; synchronises,
        like bad_row_count())."""
        return self.trainer.skipped_step_count()

    def grads_numpy(self):
        """The accumulator per tensor times the scale apply() uses (would use, while micro-batches are pending): the gradient of the
        mean loss over the step's frames.  After apply() with a process group: the exchanged gradient.  Always the UNCLIPPED gradient:
        apply(max_norm=...) scales inside the optimizer launch and leaves the accumulator alone."""
        tr = self.trainer
        scale = self._grad_scale(self._pending) if self._pending else self._scale
        flat = (self.flat * scale).cpu().numpy()                                        # (float32 product, as the apply kernel's)
        out = {}
        for i, name in enumerate(tr.names):
            o, r, c = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i], tr.plan.tensor_cols[i]
            g = flat[o:o + r * c].copy()
            out[name] = g.reshape(r, c) if name.endswith("weight") else g
        return out

    def gaps_numpy(self):
        """The accumulator's floats that belong to no tensor (the 256-byte alignment gaps): zeros after any micro()."""
        tr = self.trainer
        mask = np.ones(tr.plan.n_params, bool)
        for i in range(len(tr.names)):
            o, n = tr.plan.tensor_offset[i], tr.plan.tensor_rows[i] * tr.plan.tensor_cols[i]
            mask[o:o + n] = False
        return self.flat.cpu().numpy()[mask]

    def _gather_objects(self, obj):
        import torch.distributed as dist
        out = [None] * self.world
        if self._backend == "nccl":                        # (the pickled object travels through the rank's own device)
            with torch.cuda.device(self.trainer.device):
                dist.all_gather_object(out, obj, group=self.pg)
        else:
            dist.all_gather_object(out, obj, group=self.pg)
        return out

    def sum_over_ranks(self, t):
        """A small tensor summed over the ranks, returned on the host (reporting only: synchronises).  The collective runs where the
        group's backend can serve it: on the trainer's device under RCCL, on the host otherwise."""
        t = t.detach().clone()
        if self.pg is None:
            return t.cpu()
        import torch.distributed as dist
        t = t.to(collective_device(self._backend, self.trainer.device))
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
        return t.cpu()

    def mean_over_ranks(self, t):
        """A small float tensor averaged over the ranks (dp.mean_scalars_), returned on the host; as sum_over_ranks."""
        t = t.detach().clone()
        if self.pg is None:
            return t.cpu()
        return dp.mean_scalars_(t.to(collective_device(self._backend, self.trainer.device)), self.world, self.pg).cpu()

    def global_losses(self):
        """The last step's losses averaged over the ranks (a small all-reduce on demand; reporting only)."""
        return self.mean_over_ranks(self.losses)

    def global_counts(self):
        """The last step's tp, tn, fp, fn summed over the ranks (classifier; int64)."""
        return self.sum_over_ranks(self.counts)

    def replicas_equal(self):
        """Whether every rank holds the same parameters, bit for bit: a checksum of the flat parameters compared across the ranks
        (host side, synchronises: for debugging)."""
        if self.pg is None:
            return True
        digest = hashlib.sha256(self.trainer._params.detach().cpu().numpy().tobytes()).hexdigest()
        return len(set(self._gather_objects(digest))) == 1

    # ---- validation ----
    def evaluate(self, x, y=None, rows=None, fork=None):
        """Forward and losses of the frames `rows` (int64 device tensor, any length) of the stores x / y, in pieces of at most trainer.B
        frames -- a shorter last piece runs on fork(b), a fork() of the wrapped trainer --: the frame-weighted mean of the pieces'
        losses as a float64 device tensor (no host sync).  No backward, no update, and no workspace beyond a micro-batch's.  The noise
        is what ONE trainer of len(rows) frames would draw for its evaluate(), so the result does not depend on the split."""
        main = self.trainer
        n = int(rows.shape[0])
        eps = None
        if self._has_noise:
            main._shared["eval_count"] = main._shared.get("eval_count", 0) + 1
            g = torch.Generator(device=main.device).manual_seed((main.seed * 0x9E3779B97F4A7C15 + (1 << 40) + main._shared["eval_count"])
                                                                & 0x7FFFFFFFFFFFFFFF)
            eps = torch.randn((n, main.z_dim), generator=g, device=main.device, dtype=torch.float32)
        tot = None
        for lo in range(0, n, main.B):
            b = min(main.B, n - lo)
            tr = main if b == main.B else fork(b)
            piece = rows[lo:lo + b].contiguous()
            out = tr.evaluate(x, y, rows=piece) if not self._has_noise else tr.evaluate(x, y, eps[lo:lo + b], rows=piece)
            tot = out.to(torch.float64) * b if tot is None else tot.add_(out, alpha=float(b))
        return tot / n

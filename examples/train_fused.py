"""The reference's training loop (scripts/training_M1.py / training_M2.py / training_M2_info_vad.py: epochs of train batches, a validation pass,
one checkpoint per epoch named `<M>_epoch_{:03d}_vloss_{:.2f}.pt`, the same two log files) on the MI355X-native path:
GPU-resident frame store (disentangled-vae_amd/frames.py) + fused train step (disentangled-vae_amd/trainer.py: make_trainer -- the resident
step at the reference's z 16 / h 128 128, the generic step of trainer_generic.py at any other covered size; M2_info through
trainer_info.py: make_info_trainer, the same choice for DeepGenerativeModel_v5).

    python examples/train_fused.py --model M2 --labels ibm_labels --h5 data/complete/processed/ntcd_timit/Clean_ibm_labels_upsampled.h5
    python examples/train_fused.py --model M2 --synthetic 200000            # no dataset at hand
    python examples/train_fused.py --model M2 --synthetic 200000 --y-dim 1 --z-dim 32 --h-dim 256 64      # the model examples/enhance_mcem.py takes
    python examples/train_fused.py --model M2_info --synthetic 200000 --z-dim 32 --h-dim 256 64            # ... with --labels classifier
    # scripts/training_M2_info_vad_pretrain.py: a classifier trained alone moves in, the decoder is fed its output, the encoder's
    # adversarial term is the entropy of the auxiliary net (alpha 0, gamma = beta)
    python examples/train_classifier.py --synthetic 40 --h-dim 256 64 --save models/clf.pt --prefix enc_dec_clf.classifier.
    python examples/train_fused.py --model M2_info --synthetic 200000 --z-dim 32 --h-dim 256 64 --decoder-label classifier \
        --aux-enc entropy --gamma 10 --init-classifier models/clf.pt
    python examples/enhance_mcem.py --synthetic 3 --z-dim 32 --h-dim 256 64 --labels classifier --score \
        --checkpoint models/fused_run/M2_info_epoch_001_vloss_<...>.pt

Gradient accumulation and data parallelism on the generic steps (disentangled-vae_amd/accumulate.py: AccumulatedStep):

    # one optimizer step per 4 micro-batches of --batch frames (the stash is sized by --batch): the same run as --batch 32768
    python examples/train_fused.py --model M2_info --synthetic 200000 --z-dim 32 --h-dim 256 64 --batch 8192 --accumulate 4
    # 8 ranks, one per GPU, started from here; each brings --accumulate x --batch frames to an optimizer step
    python examples/train_fused.py --model M2 --synthetic 2000000 --z-dim 32 --h-dim 256 64 --gpus 8
    # the global gradient norm of every optimizer step clipped to 5 on the device (behind the all-reduce; no host sync); the epoch
    # line gains the mean norm and the number of steps skipped for a gradient that was not finite
    python examples/train_fused.py --model M2_info --synthetic 200000 --z-dim 32 --h-dim 256 64 --batch 8192 --accumulate 4 --clip-norm 5

Checkpoints are plain state_dicts with the reference's keys: the reference's evaluate / reconstruct scripts load them.
Differences from the scripts, all deliberate: the batch size is a flag (the fused step is meant for thousands of
frames per step; `--batch 128` reproduces the scripts' setting).

The scripts' std_norm switch (M1 / M2; off in every script, as here without the flag):

    # the encoder reads (x - mean) / (std + 1e-8), the loss is scored against the raw frames; the statistics are the file's
    # X_train_mean / X_train_std where it has them, else those of the train split taken on the device (DeviceFrames.stats);
    # norm.pt beside the checkpoints holds them for examples/enhance_mcem.py --std-norm
    python examples/train_fused.py --model M2 --synthetic 200000 --y-dim 1 --z-dim 32 --h-dim 256 64 --std-norm
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
make_trainer = importlib.import_module("disentangled-vae_amd.trainer").make_trainer
make_info_trainer = importlib.import_module("disentangled-vae_amd.trainer_info").make_info_trainer
DeviceFrames = importlib.import_module("disentangled-vae_amd.frames").DeviceFrames
AccumulatedStep = importlib.import_module("disentangled-vae_amd.accumulate").AccumulatedStep


def synthetic(n, y_dim, seed):
    rng = np.random.default_rng(seed)
    scale = np.exp(np.random.default_rng(0).standard_normal((513, 1)) - 1)     # per-bin level shared by all splits
    X = (rng.standard_normal((513, n)) ** 2 * scale).astype(np.float32)
    Y = (rng.random((y_dim, n)) > 0.5).astype(np.float32) if y_dim else None
    return X, Y


class ClipLog:
    """--clip-norm: the epoch's mean total_norm over the steps that were made and the number the device skipped (a gradient that is
    not finite), summed on the device from the trainer's grad_norm after every step and read once per epoch."""

    def __init__(self, tr, max_norm):
        self.tr, self.max_norm = tr, max_norm
        self.stat = torch.zeros(2, dtype=torch.float64, device=tr.device)          # sum of the finite norms, their number

    def note(self):
        norm = self.tr.grad_norm[0]
        ok = torch.isfinite(norm)
        self.stat[0] += torch.where(ok, norm, torch.zeros_like(norm))
        self.stat[1] += ok

    def read(self):
        total, n = self.stat.cpu().tolist()
        self.stat.zero_()
        return total / max(n, 1.0), self.tr.skipped_step_count()


def run_epoch(data, trainers, train, shuffle, clip=None):   # trainers: [main, optional fork for the last, shorter batch]
    """One pass; returns mean (ELBO, recon, KL) over batches like the scripts (sum of batch means / number of batches).
    The sums are kept on the device by the step itself: no host sync, no extra kernels per step."""
    tot = torch.zeros(8, dtype=torch.float64, device=data.device)
    nb = 0
    for rows in data.index_batches(trainers[0].B, shuffle=shuffle):     # the rows kernel gathers the frames itself
        tr = trainers[0]
        if rows.shape[0] != tr.B:                               # last, shorter batch: same parameters, its own plan
            if len(trainers) == 1 or trainers[1].B != rows.shape[0]:
                trainers[1:] = [tr.fork(rows.shape[0])]
            tr = trainers[1]
        tr.accumulate_losses(tot)
        if not train:
            tr.evaluate(data.x, data.y, rows=rows)
        elif clip is None:
            tr.step(data.x, data.y, rows=rows)
        else:
            tr.step(data.x, data.y, rows=rows, max_norm=clip.max_norm)
            clip.note()
        nb += 1
    for tr in trainers:
        tr.accumulate_losses(None)
    return (tot[:3] / nb).cpu().tolist()


def micro_sizes(n, batch):
    """n frames as micro-batches of `batch` and a shorter last one."""
    return [batch] * (n // batch) + ([n % batch] if n % batch else [])


def run_epoch_accumulated(data, acc, forks, batch, k, epoch, seed, log, clip=None):
    """One training pass with one optimizer step per k micro-batches of `batch` frames on every rank; the epoch's tail is a shorter
    step whose last micro-batch runs on a fork.  With several ranks the permutation comes from a generator seeded alike on all of them,
    rank r takes the r-th share of every step, and a tail that does not divide over the ranks loses at most world - 1 frames.
    Returns the mean (ELBO, recon, KL) over the optimizer steps (and over the ranks)."""
    world, rank = acc.world, acc.rank
    gen = None
    if world > 1:
        gen = torch.Generator(device=data.device).manual_seed(seed * 1000003 + epoch)
    tot = torch.zeros(3, dtype=torch.float64, device=data.device)
    steps = 0
    for rows in data.index_batches(world * k * batch, shuffle=True, generator=gen):
        per = rows.shape[0] // world
        if per * world != rows.shape[0]:
            log(f"epoch {epoch}: the last step drops {rows.shape[0] - per * world} frames that do not divide over {world} ranks")
        if per == 0:
            break
        mine = rows[rank * per:(rank + 1) * per]
        acc.micro_batches = micro_sizes(per, batch)                  # announced: the default noise is that of one step on all these frames
        lo = 0
        for b in acc.micro_batches:
            acc.micro(data.x, data.y, rows=mine[lo:lo + b].contiguous(), trainer=forked(acc.trainer, forks, b))
            lo += b
        tot += acc.apply(max_norm=None if clip is None else clip.max_norm)[:3]
        if clip is not None:
            clip.note()
        steps += 1
    return acc.mean_over_ranks(tot / max(steps, 1)).tolist()      # (the collective runs where the group's backend serves it)


def forked(tr, forks, b):
    """`tr` for its own batch size, otherwise its fork of b frames (one is kept: the tail of an epoch has one size)."""
    if b == tr.B:
        return tr
    if b not in forks:
        forks.clear()
        forks[b] = tr.fork(b)
    return forks[b]


def run_validation_accumulated(data, acc, forks, group):
    """The validation pass of a run whose optimizer step has `group` frames: the scripts' mean of batch means over batches of `group`
    frames, each evaluated in pieces of at most one micro-batch (AccumulatedStep.evaluate), so that the workspace stays that of a
    micro-batch and --accumulate K logs what --batch K times as large logs."""
    tot = torch.zeros(3, dtype=torch.float64, device=data.device)
    nb = 0
    for rows in data.index_batches(group, shuffle=False):
        tot += acc.evaluate(data.x, data.y, rows, lambda b: forked(acc.trainer, forks, b))[:3]
        nb += 1
    return (tot / nb).cpu().tolist()


def launch_ranks(a):
    """--gpus N with no launcher in the environment: N fresh ranks as a CHILD process, `python -m torch.distributed.run ... train_fused.py
    <same arguments>`, started before this process has made a GPU call; nothing is exec'ed over a process that has."""
    import socket
    import subprocess
    backend = os.environ.get("DVAE_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if ndev < 1 or (backend == "nccl" and ndev < a.gpus):
        sys.stderr.write(f"train_fused.py: --gpus {a.gpus} over RCCL needs {a.gpus} visible GPUs, this node shows {ndev}: RCCL ranks cannot share "
                         "a device (DVAE_DIST_BACKEND=gloo rehearses the flow with the ranks sharing the visible devices)\n")
        raise SystemExit(2)
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write("train_fused.py: starting the ranks: " + " ".join(cmd) + "\n")
    raise SystemExit(subprocess.call(cmd, env=dict(os.environ)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["M1", "M2", "M2_info"], default="M2")
    ap.add_argument("--labels", choices=["vad_labels", "ibm_labels"], default="ibm_labels")
    ap.add_argument("--h5", default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic training frames instead of --h5")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--z-dim", type=int, default=16, help="latent width (1..128)")
    ap.add_argument("--h-dim", type=int, nargs=2, default=[128, 128], metavar=("H1", "H2"), help="hidden widths (1..512)")
    ap.add_argument("--y-dim", type=int, default=None, help="label width of M2 / M2_info on synthetic data (1..513; default: what --labels gives)")
    ap.add_argument("--alpha", type=float, default=0.0, help="M2_info: weight of BCE(classifier(x), y) in enc_loss")
    ap.add_argument("--beta", type=float, default=10.0, help="M2_info: weight of the adversarial -BCE(auxiliary(z), y) in enc_loss")
    ap.add_argument("--gamma", type=float, default=1.0, help="M2_info: weight of aux_loss = BCE(auxiliary(z.detach()), y)")
    ap.add_argument("--decoder-label", choices=["truth", "classifier"], default="truth",
                    help="M2_info: what the decoder is conditioned on, the true label or the classifier's soft output (training_M2_info_vad_pretrain.py:162-163)")
    ap.add_argument("--aux-enc", choices=["bce", "uniform", "entropy"], default="bce",
                    help="M2_info: the adversarial term on the encoder, binary_cross_entropy against the label, _v2 (targets 0.5) or _v3 (the entropy)")
    ap.add_argument("--init-classifier", default=None, metavar="CKPT",
                    help="M2_info: load the keys containing enc_dec_clf.classifier from this state_dict, strict=False (training_M2_info_vad_pretrain.py:102-113)")
    ap.add_argument("--out", default="models/fused_run")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="generic steps: one optimizer step per K micro-batches of --batch frames (the workspace is sized by --batch)")
    ap.add_argument("--gpus", type=int, default=1, metavar="N",
                    help="generic steps: N data-parallel ranks, one per GPU, one all-reduce of the flat gradient per optimizer step")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="X",
                    help="generic steps: clip the global gradient norm of every optimizer step to X on the device (all tensors at once; a "
                         "gradient that is not finite skips its update); the epoch log gains the mean norm and the skipped steps")
    ap.add_argument("--std-norm", action="store_true",
                    help="M1 / M2 (generic step): standardise the encoder input with the train split's per-bin mean and standard deviation, "
                         "from --h5 where the file has them, else computed on the device; writes norm.pt beside the checkpoints")
    ap.add_argument("--kl-weight", type=float, default=1.0, metavar="W",
                    help="generic steps: the objective is recon + W * KL (a beta-VAE weight; W >= 0); the log's Recon. and KL stay raw")
    ap.add_argument("--kl-warmup", type=int, default=0, metavar="N",
                    help="generic steps: the KL weight rises linearly to --kl-weight over the first N optimizer steps")
    ap.add_argument("--kl-floor", type=float, default=0.0, metavar="L",
                    help="generic steps: free bits per element, max(k, L) for every element k of the KL term (its minimum is 0.5)")
    a = ap.parse_args()
    if a.std_norm and a.model == "M2_info":
        ap.error("--std-norm applies to --model M1 / M2 (the reference's M2_info script loads the statistics without using them)")
    if a.accumulate < 1 or a.gpus < 1:
        ap.error("--accumulate and --gpus count from 1")
    if a.clip_norm is not None and not a.clip_norm > 0:
        ap.error("--clip-norm takes a positive number")
    rank, world, pg, device = 0, 1, None, "cuda:0"
    if a.gpus > 1:
        if "WORLD_SIZE" not in os.environ:
            launch_ranks(a)                         # (does not return)
        import torch.distributed as dist
        backend = os.environ.get("DVAE_DIST_BACKEND", "nccl")
        local = int(os.environ.get("LOCAL_RANK", 0))
        device = f"cuda:{local if backend == 'nccl' else local % max(torch.cuda.device_count(), 1)}"
        torch.cuda.set_device(device)
        dist.init_process_group(backend)
        rank, world, pg = dist.get_rank(), dist.get_world_size(), dist.group.WORLD
        if world != a.gpus:
            ap.error(f"--gpus {a.gpus} under a launcher of {world} ranks")
    accumulated = a.accumulate > 1 or world > 1
    if a.model == "M2_info":
        a.labels = "vad_labels"                     # scripts/training_M2_info_vad.py: VAD labels, alpha 0 / beta 10 / gamma 1
    y_dim = 0 if a.model == "M1" else (1 if a.labels == "vad_labels" else 513)
    if a.y_dim is not None and a.model != "M1":
        if a.h5:
            ap.error("--y-dim applies to --synthetic data; with --h5 the label file decides")
        y_dim = a.y_dim
    if a.h5:
        train, valid = DeviceFrames.from_hdf5(a.h5, "train", device), DeviceFrames.from_hdf5(a.h5, "validation", device)
    else:
        n = a.synthetic or 100000
        train, valid = DeviceFrames(*synthetic(n, y_dim, 1), device=device), DeviceFrames(*synthetic(max(n // 10, 1), y_dim, 2), device=device)
    if a.model == "M1":
        train.y = valid.y = None
    dims = dict(x_dim=513, y_dim=y_dim, z_dim=a.z_dim, h_dim=tuple(a.h_dim))
    kw = dict(batch=min(a.batch, len(train)), precision=a.precision, lr=a.lr, seed=a.seed, device=device)
    if accumulated or a.clip_norm is not None:
        kw["generic"] = True                        # accumulation, data parallelism of this kind and clipping are built on the generic steps
    kl_options = (a.kl_weight, a.kl_warmup, a.kl_floor) != (1.0, 0, 0.0)
    if kl_options:                                  # a weighted KL term goes to the generic steps too (ValueError for a negative value)
        kw.update(kl_weight=a.kl_weight, kl_warmup=a.kl_warmup, kl_floor=a.kl_floor)
    if a.model == "M2_info":                        # the resident step at the reference geometry, csrc/train_info.hip at any other covered size
        tr = make_info_trainer(dims, alpha=a.alpha, beta=a.beta, gamma=a.gamma, dec_label=a.decoder_label, aux_enc=a.aux_enc, **kw)
        if a.init_classifier:
            sd = torch.load(a.init_classifier, map_location="cpu")
            sd = {k: v for k, v in sd.items() if "enc_dec_clf.classifier" in k}
            if not sd:
                ap.error(f"--init-classifier: no key of {a.init_classifier} contains enc_dec_clf.classifier")
            tr.load_state_dict(sd, strict=False)
            print(f"classifier initialised from {a.init_classifier}: {len(sd)} tensors")
    else:
        if a.decoder_label != "truth" or a.aux_enc != "bce" or a.init_classifier:
            ap.error("--decoder-label, --aux-enc and --init-classifier apply to --model M2_info")
        if a.std_norm:
            stats = None
            if a.h5:
                from packages.data_handling import FrameFile
                stats = FrameFile(a.h5, "train").stats()
            source = "the file's" if stats is not None else "taken on the device from the train split"
            mean, std = (torch.as_tensor(t) for t in (stats if stats is not None else train.stats()))
            kw["std_norm"] = (mean, std)
            if rank == 0:
                os.makedirs(a.out, exist_ok=True)       # the shape of the reference's file: (513, 1)
                torch.save({"X_train_mean": mean.cpu().reshape(513, 1), "X_train_std": std.cpu().reshape(513, 1)}, os.path.join(a.out, "norm.pt"))
                print(f"std_norm: statistics {source}; mean {float(mean.min()):.3g} .. {float(mean.max()):.3g}, "
                      f"std {float(std.min()):.3g} .. {float(std.max()):.3g} -> {os.path.join(a.out, 'norm.pt')}")
        tr = make_trainer(a.model, dims, **kw)
    tv = tr if accumulated else tr.fork(min(a.batch, len(valid)))         # (accumulated: validated in micro-batch pieces, below)
    train_trainers, valid_trainers = [tr], [tv]
    log = (lambda *args, **kws: print(*args, **kws)) if rank == 0 else (lambda *args, **kws: None)
    acc, forks, vforks = (AccumulatedStep(tr, pg, micro_batches=[tr.B] * a.accumulate), {}, {}) if accumulated else (None, None, None)
    clip = None if a.clip_norm is None else ClipLog(tr, a.clip_norm)
    if rank == 0:
        os.makedirs(a.out, exist_ok=True)
        open(os.path.join(a.out, "output_epoch.log"), "w").close()
    log(f"{a.model} {dims}: {len(train)} training frames, {len(valid)} validation frames, batch {tr.B}, {a.precision}, {type(tr).__name__}"
        + (f", {a.accumulate} micro-batches a step on each of {world} rank(s)" if accumulated else "")
        + (f", KL weight {a.kl_weight:g} after {a.kl_warmup} warm-up steps, floor {a.kl_floor:g}" if kl_options else ""))
    for epoch in range(a.epochs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if accumulated:
            elbo, rec, kl = run_epoch_accumulated(train, acc, forks, tr.B, a.accumulate, epoch, a.seed, log, clip)
        else:
            elbo, rec, kl = run_epoch(train, train_trainers, True, True, clip)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if accumulated:                             # every rank validates the same replica
            velbo, vrec, vkl = run_validation_accumulated(valid, acc, vforks, min(tr.B * a.accumulate, len(valid)))
        else:
            velbo, vrec, vkl = run_epoch(valid, valid_trainers, False, False)
        clipped = ""
        if clip is not None:                        # (read once per epoch, on every rank: the counter is each replica's own)
            norm, skipped = clip.read()
            clipped = ", grad norm: {:.3f} (clipped to {:g}), skipped steps: {}".format(norm, a.clip_norm, skipped)
        if kl_options:                              # the train ELBO is the weighted objective, the validation ELBO the target weight's
            clipped += ", KL weight: {:.4f} (step {})".format(tr.kl_weight_next, tr.step_count)
        if rank != 0:                               # rank 0 writes logs and checkpoints
            continue
        lines = [f"Epoch: {epoch}",
                 "[Train]\t\t ELBO: {:.2f}, Recon.: {:.2f}, KL: {:.2f}".format(elbo, rec, kl) + clipped,
                 "[Validation]\t ELBO: {:.2f}, Recon.: {:.2f}, KL: {:.2f}".format(velbo, vrec, vkl)]
        with open(os.path.join(a.out, "output_epoch.log"), "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), f"   ({len(train) / dt / 1e6:.1f} M frames/s incl. shuffle)")
        torch.save({k: v.cpu() for k, v in tr.state_dict().items()},
                   os.path.join(a.out, "{}_epoch_{:03d}_vloss_{:.2f}.pt".format(a.model, epoch, velbo)))
    if pg is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

"""Train the audio label classifier on the MI355X-native path: the route the reference sketches in scripts/train_audio_net.py -- noisy
spectrogram frames in, the clean speech's VAD / IBM labels as targets, binary cross entropy, Adam at 1e-4, accuracy / precision /
recall / F1 per batch -- for the net `classify_batch` runs, Classifier([513, [h1, h2], y_dim]).

    python examples/train_classifier.py --synthetic 8 --snr 0 --labels vad
    python examples/train_classifier.py --synthetic 32 --snr -5 0 5 --labels ibm --h-dim 256 64 --epochs 5 --save clf.pt

Everything runs on the device: the mixtures (mix_at_snr_batch, laid out for the batch STFT), their power frames (the batch STFT on the
mixture buffer in place), the labels of the normalised clean speech on the same layout (vad_labels_batch, or the complex batch STFT and
ibm_labels_batch), the frame store (DeviceFrames) and the fused train step (ClassifierTrainer), which gathers each batch from the store
through rows=.  One line per epoch and split: BCE and the four ratios, each averaged over the batches as the reference's log averages them.
--save writes the state_dict (--prefix enc_dec_clf.classifier. : under the keys an M2_info trainer loads with strict=False).
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mixer = importlib.import_module("disentangled-vae_amd.mix")
H = importlib.import_module("disentangled-vae_amd.stft")
tdev = importlib.import_module("disentangled-vae_amd.target")
classify = importlib.import_module("disentangled-vae_amd.classify")
DeviceFrames = importlib.import_module("disentangled-vae_amd.frames").DeviceFrames
ClassifierTrainer = importlib.import_module("disentangled-vae_amd.trainer_classifier").ClassifierTrainer

FS = 16000


def synthetic_speech(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(FS * seconds)
    env = np.repeat((rng.random(n // 1600 + 1) > 0.45).astype(np.float64), 1600)[:n]       # 100 ms on / off
    tone = np.sin(2 * np.pi * (180 + 40 * (seed % 5)) * np.arange(n) / FS + rng.random())
    return env * (0.6 * tone + 0.4 * rng.standard_normal(n)) + 1e-4 * rng.standard_normal(n)


def synthetic_noise(seconds, seed, tilt):
    w = np.random.default_rng(seed).standard_normal(int(FS * seconds) + 1)
    return 0.1 * (w[1:] + tilt * w[:-1])


def noisy_frames(speech, banks, snrs, labels, seed):
    """(X [N, 513] noisy power frames, Y [N, y_dim] labels of the clean speech) on the device: every utterance under every noise at
    every SNR."""
    speech_index, noise_index, snr_db = mixer.condition_grid(len(speech), len(banks), snrs)
    grid = [speech[u] for u in speech_index]
    starts = mixer.draw_noise_starts(np.random.default_rng(seed), [len(b) for b in banks], noise_index, [len(s) for s in grid])
    mix = mixer.mix_at_snr_batch(grid, banks, noise_index, starts, snr_db, stft_layout=True)
    p = mix.plan
    X = mix.spec(layout=1).frames
    clean = mix.speech.y                                   # the peak-normalised speech in the mixtures' layout, end pads written
    if labels == "vad":
        Y = tdev.vad_labels_batch(clean, p["x0"], p["padded"], p["frames"], p["nfft"], p["hop"])[:, None]
    else:
        S = H.stft_packed(clean, p["frames"], p["x0"], p["padded"], mix.speech.lengths, False, 2).frames
        Y = tdev.ibm_labels_batch(S, p["frame_off"][:-1] * S.shape[1], p["frames"] * S.shape[1], np.full(len(grid), S.shape[1]))
    return X, Y.contiguous()


class Epoch:
    """Running means over the batches of one pass, kept on the device: BCE and accuracy / precision / recall / F1."""

    def __init__(self, device):
        self.sums, self.n = torch.zeros(5, dtype=torch.float64, device=device), 0

    def add(self, loss, counts):
        self.sums[0] += loss[0]
        self.sums[1:] += classify.f1_from_counts(counts)
        self.n += 1

    def line(self, tag):
        v = (self.sums / max(self.n, 1)).cpu().numpy()
        return (f"[{tag}]{' ' * (12 - len(tag))}Loss: {v[0]:.4f}    Accuracy: {v[1]:.4f}    Precision: {v[2]:.4f}    Recall: {v[3]:.4f}    "
                f"F1_score: {v[4]:.4f}"), v


def run_pass(data, trainers, batch, train, generator=None, clip_norm=None, norms=None):
    """clip_norm: every step clips its global gradient norm to it on the device; `norms` (float64 [2] on the device) collects the sum
    of the finite norms and their number, with no host sync."""
    ep = Epoch(data.device)
    for idx in data.index_batches(batch, shuffle=train, generator=generator):
        tr = trainers(idx.numel())
        if not train:
            loss = tr.evaluate(data.x, data.y, rows=idx)
        elif clip_norm is None:
            loss = tr.step(data.x, data.y, rows=idx)
        else:
            loss = tr.step(data.x, data.y, rows=idx, max_norm=clip_norm)
            norm = tr.grad_norm[0]
            ok = torch.isfinite(norm)
            norms[0] += torch.where(ok, norm, torch.zeros_like(norm))
            norms[1] += ok
        ep.add(loss, tr.counts)
    return ep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, required=True, metavar="N", help="number of synthetic 3-4 s utterances (a fifth of them, at least one, "
                    "is held out for validation) mixed with two synthetic noise banks")
    ap.add_argument("--snr", type=float, nargs="+", default=[0.0], help="target SNRs in dB")
    ap.add_argument("--labels", choices=["vad", "ibm"], default="vad")
    ap.add_argument("--h-dim", type=int, nargs=2, default=[128, 128], metavar=("H1", "H2"))
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, metavar="FILE")
    ap.add_argument("--prefix", default="", help="key prefix of the saved state_dict, e.g. enc_dec_clf.classifier.")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="X",
                    help="clip the global gradient norm of every step to X on the device (a gradient that is not finite skips its update); "
                         "the epoch log gains the mean norm and the skipped steps")
    a = ap.parse_args()
    if a.clip_norm is not None and not a.clip_norm > 0:
        ap.error("--clip-norm takes a positive number")
    if a.synthetic < 2:
        ap.error("--synthetic: at least two utterances (one is held out)")
    speech = [synthetic_speech(3.0 + 0.25 * (i % 5), a.seed + i) for i in range(a.synthetic)]
    banks = [synthetic_noise(10.0, 1000 + b, 0.9 * b) for b in range(2)]
    n_val = max(1, a.synthetic // 5)
    sets = {}
    for split, utts, seed in (("train", speech[n_val:], a.seed), ("valid", speech[:n_val], a.seed + 1)):
        X, Y = noisy_frames(utts, banks, a.snr, a.labels, seed)
        sets[split] = DeviceFrames.from_rows(X, Y)
        print(f"- {split}: {len(utts)} utterances x {len(banks)} noises x {len(a.snr)} SNRs -> {len(sets[split])} frames, "
              f"{float(Y.mean()):.3f} of the labels active")
    y_dim = sets["train"].y.shape[1]
    main_tr = ClassifierTrainer([513, list(a.h_dim), y_dim], batch=a.batch, device=sets["train"].device, lr=a.lr, seed=a.seed)
    forks = {a.batch: main_tr}

    def trainers(n):                                       # the last, shorter batch of a pass: a fork over the same parameters and moments
        if n not in forks:
            forks[n] = main_tr.fork(n)
        return forks[n]

    print(f"Classifier [513, {list(a.h_dim)}, {y_dim}], {a.labels} labels, batch {a.batch}, Adam lr {a.lr:g}")
    gen = torch.Generator(device=sets["train"].device).manual_seed(a.seed)
    first = last = None
    norms = torch.zeros(2, dtype=torch.float64, device=sets["train"].device)
    for epoch in range(a.epochs):
        t_line, t = run_pass(sets["train"], trainers, a.batch, True, gen, a.clip_norm, norms).line("Train")
        if a.clip_norm is not None:                        # read once per epoch; the counter is shared by the forks
            total, n = norms.cpu().tolist()
            norms.zero_()
            t_line += f"    Grad norm: {total / max(n, 1.0):.4f} (clipped to {a.clip_norm:g})    Skipped steps: {main_tr.skipped_step_count()}"
        v_line, _ = run_pass(sets["valid"], trainers, a.batch, False).line("Validation")
        print(f"Epoch: {epoch}\n{t_line}\n{v_line}")
        first, last = (t[0] if first is None else first), t[0]
    bad = sum(tr.bad_row_count() for tr in forks.values())
    print(f"train BCE {first:.4f} -> {last:.4f} over {a.epochs} epochs ({main_tr.step_count} steps); gather indices refused: {bad}")
    if a.save:
        torch.save({k: v.cpu() for k, v in main_tr.state_dict(prefix=a.prefix).items()}, a.save)
        print("wrote", a.save)


if __name__ == "__main__":
    main()

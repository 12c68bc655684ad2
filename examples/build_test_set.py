"""The noisy test set of the reference's scripts/create_test_set.py:89-125 on the MI355X-native path: every clean utterance mixed with
a random segment of a long noise recording at every target SNR in one call (disentangled-vae_amd/mix.py: mix_at_snr_batch, five
launches whatever the number of conditions), then written as <name>_s.wav, <name>_n.wav and <name>_x.wav like the reference.

    python examples/build_test_set.py --speech a.wav b.wav --noise cafe.wav car.wav --snr -5 0 5 --out test_set/
    python examples/build_test_set.py --synthetic 8 --snr -5 0 5        # no data at hand: speech-like signals and noise banks from a seed
    python examples/build_test_set.py --speech a.wav --noise CAFE-CAFE-1.wav --noise-fs 48000      # raw recordings, resampled on the device

Every utterance meets every noise recording at every SNR (NTCD-TIMIT's layout: each utterance under 6 noises x 6 SNRs).  The segment
starts come from a seeded numpy Generator; the reference draws them from the global np.random inside a thread pool, so its choice
is not reproducible and no parity with it is claimed.  The noise recordings are at 16 kHz, or with --noise-fs N at N Hz (the raw
48 kHz QUT recordings, any channel count): those are brought to 16 kHz on the device by packages/dataset/qut_database.py:
preprocess_noise_many (first channel, one launch for all of them; a file named like the car recording gets the reference's cut) and
stay there for the mixer.  <out>/stats.npy holds p, Ps, Pn, k, norm and the achieved SNR
of every mixture (mix.STATS), <out>/conditions.txt their names.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mixer = importlib.import_module("disentangled-vae_amd.mix")
from packages.dataset import qut_database
FS = 16000


def read_wav(path, fs_want=FS, channels=False):
    fs, w = wavfile.read(path)
    if fs != fs_want:
        raise ValueError(f"{path}: {fs_want} Hz expected, got {fs}")  # create_test_set.py:98: 'Unexpected sampling rate'
    if channels:
        w = w.reshape(len(w), -1)                                     # [n, C], as soundfile hands the reference its recordings
    elif w.ndim != 1:
        raise ValueError(f"{path}: one channel expected")
    return w.astype(np.float64) / 32768.0 if w.dtype == np.int16 else w.astype(np.float32 if w.dtype == np.float32 else np.float64)


def synthetic_speech(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(FS * seconds)
    env = np.repeat((rng.random(n // 800 + 1) > 0.5).astype(np.float64), 800)[:n]      # 50 ms on/off "speech"
    return env * rng.standard_normal(n) * np.sin(2 * np.pi * 220 * np.arange(n) / FS + rng.random())


def synthetic_noise(seconds, seed, tilt, fs=FS):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(int(fs * seconds) + 1)
    return 0.1 * (w[1:] + tilt * w[:-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speech", nargs="*", default=[], help="clean utterances (16 kHz wav)")
    ap.add_argument("--noise", nargs="*", default=[], help="long noise recordings (16 kHz wav), each longer than every utterance")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic 3-4 s utterances (and two 10 s noise banks) instead of files")
    ap.add_argument("--noise-fs", type=int, default=FS, metavar="N", help="sampling rate of the noise recordings (or of the synthetic banks): "
                    "anything but 16000 is resampled to 16 kHz on the device, first channel, before mixing")
    ap.add_argument("--snr", type=float, nargs="+", default=[-15.0, -10.0, -5.0, 0.0, 5.0], help="target SNRs in dB (create_test_set.py:142)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the segment starts")
    ap.add_argument("--float32", action="store_true", help="keep the outputs in float32 on the device (one more rounding)")
    ap.add_argument("--out", default="test_set")
    a = ap.parse_args()
    if a.synthetic:
        speech = [synthetic_speech(3.0 + 0.25 * (i % 5), i) for i in range(a.synthetic)]
        names = [f"synthetic_{i:02d}" for i in range(a.synthetic)]
        banks, noise_names = [synthetic_noise(10.0, 1000 + b, 0.9 * b, a.noise_fs) for b in range(2)], ["white", "pink"]
        if a.noise_fs != FS:
            banks = [np.stack([b, -b], axis=1) for b in banks]        # two channels, like a raw recording
    else:
        if not a.speech or not a.noise:
            ap.error("give --speech and --noise files, or --synthetic N")
        speech, names = [read_wav(p) for p in a.speech], [os.path.splitext(os.path.basename(p))[0] for p in a.speech]
        banks, noise_names = [read_wav(p, a.noise_fs, a.noise_fs != FS) for p in a.noise], [os.path.splitext(os.path.basename(p))[0] for p in a.noise]

    t0 = time.perf_counter()
    if a.noise_fs != FS:
        car = qut_database._TEST_FILES["car"][:-4]
        raw = {("car" if name == car else f"{i}:{name}"): b for i, (name, b) in enumerate(zip(noise_names, banks))}
        banks = list(qut_database.preprocess_noise_many(raw, a.noise_fs, FS).values())          # on the device, in the order given
    speech_index, noise_index, snr_db = mixer.condition_grid(len(speech), noise_names, a.snr)
    grid = [speech[u] for u in speech_index]                       # the same array many times: packed and uploaded once
    starts = mixer.draw_noise_starts(np.random.default_rng(a.seed), [len(b) for b in banks], noise_index, [len(s) for s in grid])
    mix = mixer.mix_at_snr_batch(grid, banks, noise_index, starts, snr_db, out_dtype=torch.float32 if a.float32 else torch.float64)
    stats = mix.stats.cpu().numpy()
    dt = time.perf_counter() - t0

    os.makedirs(a.out, exist_ok=True)
    conditions = [f"{names[u]}_{noise_names[b]}_snr{s:+g}" for u, b, s in zip(speech_index, noise_index, snr_db)]
    for tag, batch in (("s", mix.speech), ("n", mix.noise), ("x", mix.mixture)):
        for name, w in zip(conditions, batch.numpy()):
            wavfile.write(os.path.join(a.out, f"{name}_{tag}.wav"), FS, w)
    np.save(os.path.join(a.out, "stats.npy"), stats)
    with open(os.path.join(a.out, "conditions.txt"), "w") as f:
        f.write("\n".join(conditions) + "\n")
    print(f"{len(conditions)} mixtures ({len(speech)} utterances x {len(banks)} noises x {len(a.snr)} SNRs) in {dt:.3f} s "
          f"({len(conditions) / dt:.0f} mixtures/s), written to {a.out}/")
    print(f"{'condition':<36}{'requested':>10}{'achieved':>12}{'peak':>8}   (dB)")
    peaks = [max(np.abs(w).max() for w in ws) for ws in zip(mix.speech.numpy(), mix.noise.numpy(), mix.mixture.numpy())]
    for name, want, row, peak in zip(conditions, snr_db, stats, peaks):
        print(f"{name:<36}{want:>10.1f}{row[5]:>12.6f}{peak:>8.3f}")


if __name__ == "__main__":
    main()

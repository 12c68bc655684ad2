"""QUT-NOISE for the test-set builder (reference packages/dataset/qut_database.py:20-115, called from scripts/create_test_set.py:74-82):
which recordings make the test set, how a raw recording is brought to the working rate, and which segment of it meets an utterance.

Same names, signatures and return values as the reference; written on os.walk / pathlib like ntcd_timit.py here.  The listings and
`noise_segment` are host logic.  `preprocess_noise` resamples with the polyphase resampler of disentangled-vae_amd/resample.py: on
the device when a GPU is present, with its numpy restatement otherwise.  The reference asks librosa.resample, which is not available to
this repository, so parity with it is unpinned; the filter is resample.resample_taps.  `preprocess_noise_many` is this project's own:
every recording in one launch, left on the device for mix_at_snr_batch.
"""
import importlib
import os
from pathlib import Path

import numpy as np
import torch

_TEST_FILES = {"cafe": "CAFE-CAFE-1.wav", "car": "CAR-WINDOWNB-1.wav", "home": "HOME-KITCHEN-1.wav", "street": "STREET-CITY-1.wav"}
_CAR_MINUTES = (1.5, 43)                 # the part of the car recording that is kept


def _resampler():
    return importlib.import_module("disentangled-vae_amd.resample")


def _wavs_below(prefix):
    """Every .wav whose path starts with the string `prefix` (a directory with its trailing separator, or a directory plus the head
    of a name, as the reference's string concatenation into a recursive glob allows)."""
    root = prefix if os.path.isdir(prefix) else os.path.dirname(prefix)
    hits = []
    for d, _, files in os.walk(root):
        hits += [os.path.join(d, f) for f in files if f.endswith(".wav") and os.path.join(d, f).startswith(prefix)]
    return sorted(hits)


def noise_list(input_noise_dir, dataset_type='test'):
    """{noise type: path relative to input_noise_dir} of the four recordings of the test set.  Only 'test' is defined (the reference
    prints 'Not implemented' for the other subsets and then fails on an unbound name; here they list nothing)."""
    if dataset_type != 'test':
        print('Not implemented')
        return {}
    names = {v: k for k, v in _TEST_FILES.items()}
    found = {}
    for path in _wavs_below(input_noise_dir):
        if os.path.basename(path) in names:
            found[names[os.path.basename(path)]] = os.path.relpath(path, input_noise_dir)
    return found


def _car_cut(fs):
    return tuple(int(m * 60 * fs) for m in _CAR_MINUTES)


def preprocess_noise(noise_audio, key, fs_noise, fs):
    """The first channel of the [n, C] recording noise_audio (fs_noise Hz) at fs Hz; for key == 'car' only the part between 1.5 min
    and 43 min.  numpy in, numpy out (float64 once resampled).  fs == fs_noise returns the first channel as it is: the reference
    raises UnboundLocalError there."""
    noise_audio = np.asarray(noise_audio)
    if fs == fs_noise:
        out = noise_audio[:, 0]
    elif torch.cuda.is_available():
        out = _resampler().resample_batch([noise_audio], fs_noise, fs, channel=0).numpy()[0]
    else:
        rs = _resampler()
        taps, p, q, _ = rs.resample_taps(fs_noise, fs)
        out = rs.resample_numpy(noise_audio[:, 0], taps, p, q)
    if key == 'car':
        lo, hi = _car_cut(fs)
        out = out[lo:hi]
    return out


def preprocess_noise_many(noise_audios, fs_noise, fs):
    """preprocess_noise of every recording of {key: [n, C] array} in one launch -> {key: 1-D tensor on the device}; its values, as a
    list, are the noise_banks of mix_at_snr_batch.  The recordings share their channel count.  Needs the GPU."""
    keys = list(noise_audios)
    if fs == fs_noise:
        dev = importlib.import_module("disentangled-vae_amd.ragged").device()
        out = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(noise_audios[k])[:, 0])).to(dev) for k in keys}
    else:
        batch = _resampler().resample_batch([np.asarray(noise_audios[k]) for k in keys], fs_noise, fs, channel=0)
        out = {k: batch[u] for u, k in enumerate(keys)}
    if 'car' in out:
        lo, hi = _car_cut(fs)
        out['car'] = out['car'][lo:hi]
    return out


def noise_list_preprocessed(preprocessed_noise_dir, dataset_type='test'):
    """{file stem: path} of the preprocessed recordings below preprocessed_noise_dir + dataset_type."""
    return {Path(p).stem: p for p in _wavs_below(preprocessed_noise_dir + dataset_type)}


def noise_segment(noise_audios, noise_type, speech):
    """A random segment of noise_audios[noise_type] as long as speech; the start is drawn from the global np.random, as the reference
    draws it.  An unknown noise type prints 'Error' and then fails on the unbound result, as the reference does."""
    if noise_type not in noise_audios:
        print('Error')
        raise UnboundLocalError(f"no noise recording of type {noise_type!r}")
    bank = noise_audios[noise_type]
    start = np.random.randint(len(bank) - len(speech))
    return bank[start:start + len(speech)]

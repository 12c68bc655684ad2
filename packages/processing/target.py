"""Drop-in replacement for the label makers of the reference's packages/processing/target.py that the scripts use
(create_train_set.py, create_video_train_files.py, reconstruct_*.py, run_metrics.py): `clean_speech_VAD`,
`clean_speech_IBM`, `noise_robust_clean_speech_IBM` -- same keyword signatures, numpy in, numpy float32 out.

The frame bookkeeping (window / hop sizes, the end-pad rule in Python doubles, quirk Q6) is done on the host as the
reference does it; the per-frame energies, the global extrema and the thresholds run in the HIP kernels of
csrc/target.hip (labels agree bit for bit with the label files the reference wrote for data/subset).  librosa is
not imported and there is no CPU path: without a GPU these functions raise.  The reference's never-called
`noise_aware_IBM` / `threshold_IBM` experiments are not carried over.

Beyond the reference: `clean_speech_VAD_many`, `clean_speech_IBM_many` and `noise_robust_clean_speech_IBM_many`, lists in
and lists out, equal element by element (value, dtype and shape) to the single-utterance functions and computed as one
ragged batch per call (any window and hop, `center` either way, float32 / float64 signals, C- or Fortran-ordered spectrograms).
"""
import math

import numpy as np
import torch

from packages import _native


def _frames_for(n_samples, fs, wlen_sec, hop_percent, center, pad_at_end):
    nfft = int(wlen_sec * fs)
    hopsamp = int(hop_percent * nfft)
    padded = n_samples
    if pad_at_end:
        utt_len = n_samples / fs
        if math.ceil(utt_len / wlen_sec / hop_percent) != int(utt_len / wlen_sec / hop_percent):
            padded += hopsamp
    if center:
        padded += 2 * int(nfft // 2)
    if padded < nfft:
        raise ValueError("Input signal length=%d is too small for frame_length=%d" % (padded, nfft))
    return nfft, hopsamp, padded, 1 + (padded - nfft) // hopsamp


def clean_speech_VAD(speech_t,
                     fs=16e3,
                     wlen_sec=50e-3,
                     hop_percent=0.25,
                     center=True,
                     pad_mode='reflect',
                     pad_at_end=True,
                     vad_threshold=1.70):
    """Time-domain VAD: frame energy > 10**vad_threshold * (energy of the quietest frame).  Returns (1, T) float32."""
    T = _native.target_dev()
    y = np.asarray(speech_t)
    nfft, hopsamp, padded, frames = _frames_for(len(y), fs, wlen_sec, hop_percent, center, pad_at_end)
    if center:                                  # the end-pad zeros sit inside the reflect padding: materialise both
        if padded - 2 * int(nfft // 2) > len(y):
            y = np.pad(y, (0, hopsamp), mode='constant')
        y = np.pad(y, int(nfft // 2), mode=pad_mode)
    vad = T.vad_labels(torch.from_numpy(np.ascontiguousarray(y)), nfft, hopsamp, frames, vad_threshold)
    return vad.cpu().numpy()[None]


def clean_speech_IBM(speech_tf,
                     eps=1e-8,
                     ibm_threshold=50):
    """Ideal binary mask: bins within `ibm_threshold` dB of the loudest bin of the utterance.  float32, same shape."""
    T = _native.target_dev()
    S = np.asarray(speech_tf)
    if S.dtype != np.complex64:
        raise TypeError("clean_speech_IBM: the HIP path reproduces the float32 arithmetic of complex64 input (got %s)" % S.dtype)
    return T.ibm_labels(torch.from_numpy(np.ascontiguousarray(S)), eps, ibm_threshold).cpu().numpy()


def noise_robust_clean_speech_IBM(speech_t,
                                  speech_tf,
                                  fs=16e3,
                                  wlen_sec=50e-3,
                                  hop_percent=0.25,
                                  center=True,
                                  pad_mode='reflect',
                                  pad_at_end=True,
                                  vad_threshold=1.70,
                                  eps=1e-8,
                                  ibm_threshold=50):
    """IBM gated by the time-domain VAD (labels robust to noise before / after the speech)."""
    vad = clean_speech_VAD(speech_t, fs=fs, wlen_sec=wlen_sec, hop_percent=hop_percent, center=center,
                           pad_mode=pad_mode, pad_at_end=pad_at_end, vad_threshold=vad_threshold)
    return clean_speech_IBM(speech_tf, eps=eps, ibm_threshold=ibm_threshold) * vad


def _vad_batch(speech_list, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold):
    """clean_speech_VAD's host preparation per signal, the signals packed into one buffer -> (device vad [sum T], frame counts)."""
    T = _native.target_dev()
    ys, frames = [], []
    for u, y in enumerate(speech_list):
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError("clean_speech_VAD_many: signal %d is not 1-D (shape %s)" % (u, y.shape))
        nfft, hopsamp, padded, T_u = _frames_for(len(y), fs, wlen_sec, hop_percent, center, pad_at_end)
        if center:
            if padded - 2 * int(nfft // 2) > len(y):
                y = np.pad(y, (0, hopsamp), mode='constant')
            y = np.pad(y, int(nfft // 2), mode=pad_mode)
        ys.append(y)
        frames.append(T_u)
    # the kernel reads float32 as float32 and anything else as float64 (what the single call uploads); float32 samples convert to
    # double exactly, so a mixed list shares one float64 buffer
    dt = np.float32 if all(y.dtype == np.float32 for y in ys) else np.float64
    n = np.array([len(y) for y in ys], np.int64)
    x0 = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    buf = np.empty(int(n.sum()), dt)
    for y, a in zip(ys, x0):
        buf[a:a + len(y)] = y
    vad = T.vad_labels_batch(torch.from_numpy(buf), x0, n, frames, nfft, hopsamp, vad_threshold)
    return vad, frames


def _split(flat, counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [flat[a:b] for a, b in zip(off[:-1], off[1:])]


def clean_speech_VAD_many(speech_list,
                          fs=16e3,
                          wlen_sec=50e-3,
                          hop_percent=0.25,
                          center=True,
                          pad_mode='reflect',
                          pad_at_end=True,
                          vad_threshold=1.70):
    """[clean_speech_VAD(s, ...) for s in speech_list] in one batch: (1, T_u) float32 each, bit for bit."""
    speech_list = list(speech_list)
    if not speech_list:
        return []
    vad, frames = _vad_batch(speech_list, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold)
    return [v[None] for v in _split(vad.cpu().numpy(), frames)]


def _ibm_batch(S_list, eps, ibm_threshold, gate=None, g0=None):
    T = _native.target_dev()
    Ss = [np.asarray(S) for S in S_list]
    for u, S in enumerate(Ss):
        if S.dtype != np.complex64:
            raise TypeError("clean_speech_IBM: the HIP path reproduces the float32 arithmetic of complex64 input (got %s)" % S.dtype)
        if S.ndim != 2:
            raise ValueError("clean_speech_IBM_many: spectrogram %d is not 2-D (shape %s)" % (u, S.shape))
    count = np.array([S.size for S in Ss], np.int64)
    e0 = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    buf = np.empty(int(count.sum()), np.complex64)
    for S, a in zip(Ss, e0):
        buf[a:a + S.size] = S.ravel(order='C')       # the row-major matrix the single call makes contiguous
    mask = T.ibm_labels_batch(torch.from_numpy(buf), e0, count, [S.shape[1] for S in Ss], eps, ibm_threshold, gate, g0).cpu().numpy()
    return [m.reshape(S.shape) for m, S in zip(_split(mask, count), Ss)]


def clean_speech_IBM_many(S_list,
                          eps=1e-8,
                          ibm_threshold=50):
    """[clean_speech_IBM(S, eps, ibm_threshold) for S in S_list] in one batch (each mask against its own spectrogram's peak)."""
    S_list = list(S_list)
    return _ibm_batch(S_list, eps, ibm_threshold) if S_list else []


def noise_robust_clean_speech_IBM_many(speech_list,
                                       S_list,
                                       fs=16e3,
                                       wlen_sec=50e-3,
                                       hop_percent=0.25,
                                       center=True,
                                       pad_mode='reflect',
                                       pad_at_end=True,
                                       vad_threshold=1.70,
                                       eps=1e-8,
                                       ibm_threshold=50):
    """[noise_robust_clean_speech_IBM(s, S, ...) for s, S in zip(speech_list, S_list)]: the VAD stays on the device and gates the mask
    in the mask kernel when every spectrogram has one column per VAD frame (any other shapes: numpy's broadcast of the single call)."""
    speech_list, S_list = list(speech_list), list(S_list)
    if len(speech_list) != len(S_list):
        raise ValueError("noise_robust_clean_speech_IBM_many: %d signals for %d spectrograms" % (len(speech_list), len(S_list)))
    if not S_list:
        return []
    vad, frames = _vad_batch(speech_list, fs, wlen_sec, hop_percent, center, pad_mode, pad_at_end, vad_threshold)
    shapes = [np.shape(S) for S in S_list]
    if all(len(sh) == 2 and sh[1] == T_u for sh, T_u in zip(shapes, frames)):
        g0 = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64)
        return _ibm_batch(S_list, eps, ibm_threshold, vad, g0)
    vads = [v[None] for v in _split(vad.cpu().numpy(), frames)]
    return [m * v for m, v in zip(_ibm_batch(S_list, eps, ibm_threshold), vads)]

"""Host side of STFT / ISTFT: integer / indexing decisions in Python doubles exactly
as the reference makes them (packages/processing/stft.py:34-50: window length, hop,
the floating-point end-pad rule, quirk Q6), then the C ABI of csrc/stft.hip
(host entries and dispatch; the kernels are in csrc/stft_fwd.hip and
csrc/istft.hip).  No CPU transform exists here: without the library or a GPU
these functions raise.
"""
import math
import os

import numpy as np
import torch

from . import native as N
from . import ragged as R
from .ragged import WaveBatch  # noqa: F401  (istft_batch returns it; importable from here as before)


def sizes(fs, wlen_sec, hop_percent, what="STFT"):
    """nfft / hop exactly as packages/processing/stft.py:34-37 (raises on non-integer window)."""
    if wlen_sec * fs != int(wlen_sec * fs):
        raise ValueError("wlen_sample of %s is not an integer." % what)
    nfft = int(wlen_sec * fs)
    hopsamp = int(hop_percent * nfft)
    return nfft, hopsamp


def needs_end_pad(n, fs, wlen_sec, hop_percent):
    """packages/processing/stft.py:45-47, same operation order in Python doubles (bit-exact
    frame indexing depends on it: some exact multiples of the hop ARE padded)."""
    utt_len = n / fs
    return math.ceil(utt_len / wlen_sec / hop_percent) != int(utt_len / wlen_sec / hop_percent)


def frame_count(n_padded, nfft, hop):
    """librosa.util.frame: 1 + (len - n_fft) // hop."""
    if n_padded < nfft:
        raise ValueError("Input signal length=%d is too small to analyze with n_fft=%d" % (n_padded, nfft))
    return 1 + (n_padded - nfft) // hop


_window_cache = {}


def window_f64(win, nfft, device):
    """Periodic window as float64 on `device` (librosa: scipy.signal.get_window(win, n, fftbins=True))."""
    key = (str(win), int(nfft), str(device))
    w = _window_cache.get(key)
    if w is None:
        from scipy.signal import get_window
        w = torch.from_numpy(np.ascontiguousarray(get_window(win, nfft, fftbins=True), dtype=np.float64)).to(device)
        _window_cache[key] = w
    return w


def stft_device(x_dev, window, nfft, hop, T, layout=0):
    """x_dev: 1-D float32/float64 CUDA tensor already padded.  layout 0 -> complex64 [F, T];
    layout 1 -> float32 power frames [T, F]; layout 2 -> complex64 [T, F] (frame-major: the values of layout 0 in the memory
    order of librosa's Fortran-ordered result; `.T` of it is the reference's array, strides included)."""
    lib = N.load()
    if not x_dev.is_cuda or x_dev.dim() != 1 or x_dev.dtype not in (torch.float32, torch.float64):
        raise TypeError("stft_device: 1-D float32/float64 CUDA tensor required")
    x_dev = x_dev.contiguous()
    F = nfft // 2 + 1
    if layout == 0:
        out = torch.empty((F, T), dtype=torch.complex64, device=x_dev.device)
    elif layout == 2:
        out = torch.empty((T, F), dtype=torch.complex64, device=x_dev.device)
    else:
        out = torch.empty((T, F), dtype=torch.float32, device=x_dev.device)
    N.check(lib.dvae_stft(N.ptr(x_dev), 1 if x_dev.dtype == torch.float64 else 0, x_dev.numel(), N.ptr(window), nfft, hop, T,
                          N.ptr(out), layout, N.stream()), "dvae_stft")
    return out


def window_f32(nfft, device):
    """torch.hann_window(nfft) (periodic, float32) on `device`: the window of the reference's stft_pytorch (stft.py:141)."""
    key = ("hann_f32", int(nfft), str(device))
    w = _window_cache.get(key)
    if w is None:
        w = torch.hann_window(window_length=nfft).to(device)
        _window_cache[key] = w
    return w


def f32_transform_covers(x_dev, nfft, hop, T):
    """dvae_stft_f32: nfft 1024 / hop 256, float32 signal, 32-bit byte offsets."""
    return (nfft == 1024 and hop == 256 and x_dev.dtype == torch.float32 and x_dev.numel() * 4 < 2 ** 31 and T * 513 * 8 < 2 ** 31
            and os.environ.get("DVAE_STFT_F32", "1") != "0")


def stft_device_f32(x_dev, nfft, hop, T, layout=2):
    """The float32-ARITHMETIC transform (torch.stft's on a float32 tensor: packages/processing/stft.py:123-152): x_dev 1-D float32 CUDA
    tensor already padded -> layout 2: complex64 [T, F] (frame-major; `.T` is the [F, T] result), layout 1: float32 [T, F] re^2 + im^2."""
    lib = N.load()
    if not x_dev.is_cuda or x_dev.dim() != 1 or x_dev.dtype != torch.float32:
        raise TypeError("stft_device_f32: 1-D float32 CUDA tensor required")
    x_dev = x_dev.contiguous()
    F = nfft // 2 + 1
    out = torch.empty((T, F), dtype=torch.complex64 if layout == 2 else torch.float32, device=x_dev.device)
    N.check(lib.dvae_stft_f32(N.ptr(x_dev), x_dev.numel(), N.ptr(window_f32(nfft, x_dev.device)), nfft, hop, T, N.ptr(out), layout, N.stream()),
            "dvae_stft_f32")
    return out


def istft_device(S_dev, window, nfft, hop, n_frames, start, out_len):
    """S_dev: complex64 [F, >= n_frames] CUDA tensor -> float32 [out_len].  A tensor whose memory is frame-major (the `.T` view of
    a contiguous [T, F] tensor, e.g. of stft_device(..., layout=2)) is read in place by the frame-major kernel; anything else is
    made row-contiguous first."""
    lib = N.load()
    if not S_dev.is_cuda or S_dev.dtype != torch.complex64 or S_dev.dim() != 2 or S_dev.shape[0] != nfft // 2 + 1:
        raise TypeError("istft_device: complex64 [nfft/2+1, T] CUDA tensor required")
    y = torch.empty((out_len,), dtype=torch.float32, device=S_dev.device)
    if S_dev.shape[1] > 1 and S_dev.stride(0) == 1 and S_dev.stride(1) >= S_dev.shape[0] and nfft == 1024 and hop == 256:
        # the frame-major walk needs no scratch; the A/B switches that route it to the two-pass kernels do (frames in double)
        two_pass = os.environ.get("DVAE_STFT_LEGACY") is not None or os.environ.get("DVAE_ISTFT_2PASS") is not None
        ws = torch.empty(max(lib.dvae_istft_workspace_bytes(n_frames, nfft), 16) if two_pass else 16, dtype=torch.uint8, device=S_dev.device)
        N.check(lib.dvae_istft_frames(N.ptr(S_dev), n_frames, S_dev.stride(1), N.ptr(window), nfft, hop, start, N.ptr(y), out_len,
                                      N.ptr(ws), N.stream()), "dvae_istft_frames")
        return y
    ws = torch.empty(max(lib.dvae_istft_workspace_bytes_hop(n_frames, nfft, hop), 16), dtype=torch.uint8, device=S_dev.device)
    S_dev = S_dev.contiguous()
    N.check(lib.dvae_istft(N.ptr(S_dev), n_frames, S_dev.shape[1], N.ptr(window), nfft, hop, start, N.ptr(y), out_len,
                           N.ptr(ws), N.stream()), "dvae_istft")
    return y


def f32_inverse_covers(S_dev, nfft, hop):
    """dvae_istft_f32: nfft 1024 / hop 256, complex64 [513, T], 32-bit byte offsets."""
    return (nfft == 1024 and hop == 256 and S_dev.dtype == torch.complex64 and S_dev.dim() == 2 and S_dev.shape[0] == 513
            and max(S_dev.shape[1] * 513, S_dev.shape[1] * S_dev.stride(1) if S_dev.stride(0) == 1 else 0) * 8 < 2 ** 31
            and os.environ.get("DVAE_ISTFT_F32", "1") != "0")


def istft_device_f32(S_dev, nfft, hop, n_frames, start, out_len):
    """The float32-ARITHMETIC inverse transform (torch.istft's on a complex64 tensor: packages/processing/stft.py:154-190): S_dev
    complex64 [513, >= n_frames] CUDA tensor -> float32 [out_len].  Frame-major memory (the `.T` view of a contiguous [T, 513] tensor,
    what stft_pytorch returns) is read in place; a row-contiguous tensor is transposed on the device first."""
    lib = N.load()
    if not S_dev.is_cuda or S_dev.dtype != torch.complex64 or S_dev.dim() != 2 or S_dev.shape[0] != nfft // 2 + 1:
        raise TypeError("istft_device_f32: complex64 [nfft/2+1, T] CUDA tensor required")
    y = torch.empty((out_len,), dtype=torch.float32, device=S_dev.device)
    w = window_f32(nfft, S_dev.device)
    if S_dev.shape[1] > 1 and S_dev.stride(0) == 1 and S_dev.stride(1) >= S_dev.shape[0]:
        N.check(lib.dvae_istft_f32(N.ptr(S_dev), n_frames, S_dev.stride(1), 1, N.ptr(w), nfft, hop, start, N.ptr(y), out_len, None, N.stream()),
                "dvae_istft_f32")
        return y
    S_dev = S_dev.contiguous()
    ws = torch.empty((n_frames, nfft // 2 + 1), dtype=torch.complex64, device=S_dev.device)
    N.check(lib.dvae_istft_f32(N.ptr(S_dev), n_frames, S_dev.shape[1], 0, N.ptr(w), nfft, hop, start, N.ptr(y), out_len, N.ptr(ws), N.stream()),
            "dvae_istft_f32")
    return y


def stft_numpy(x, fs, wlen_sec, win, hop_percent, center, pad_mode, pad_at_end, dtype, layout=0):
    """numpy in / numpy out body of packages.processing.stft.stft."""
    nfft, hop = sizes(fs, wlen_sec, hop_percent, "STFT")
    x = np.asarray(x)
    if not np.issubdtype(x.dtype, np.floating):
        raise TypeError("stft: audio must be floating point (as librosa requires)")
    x_ = x
    if pad_at_end and needs_end_pad(len(x), fs, wlen_sec, hop_percent):
        x_ = np.pad(x, (0, hop), mode="constant")
    # pad_at_end=False: the reference leaves x_ undefined (quirk Q7); here it means "no end pad"
    if center:
        x_ = np.pad(x_, int(nfft // 2), mode=pad_mode)
    T = frame_count(len(x_), nfft, hop)
    dev = R.device()
    xin = np.ascontiguousarray(x_, dtype=np.float64 if x_.dtype != np.float32 else np.float32)
    # the complex result is computed frame-major (whole frames leave the kernel as contiguous rows) and returned as the
    # transpose view: a Fortran-ordered [F, T] array, which is also what librosa.stft hands the reference
    out = stft_device(torch.from_numpy(xin).to(dev), window_f64(win, nfft, dev), nfft, hop, T, 2 if layout == 0 else layout)
    res = out.cpu().numpy()
    if layout == 0:
        res = res.T
        if np.dtype(dtype) != res.dtype:
            res = res.astype(dtype)
    return res


def istft_numpy(Sxx, fs, wlen_sec, win, hop_percent, center, dtype, max_len):
    """numpy in / numpy out body of packages.processing.stft.istft (librosa.istft semantics)."""
    nfft, hop = sizes(fs, wlen_sec, hop_percent, "iSTFT")
    S = np.asarray(Sxx)
    if S.ndim != 2 or S.shape[0] != 1 + nfft // 2:
        raise ValueError("istft: expected a [%d, T] spectrogram" % (1 + nfft // 2))
    n_frames = S.shape[1]
    if max_len:
        padded = max_len + nfft if center else max_len
        n_frames = min(n_frames, int(np.ceil(padded / hop)))
    ntot = nfft + hop * (n_frames - 1)
    start = nfft // 2 if center else 0
    if max_len is None:
        out_len = ntot - 2 * (nfft // 2) if center else ntot
    else:
        out_len = int(max_len)
    dev = R.device()
    # frame-major on the device (each frame one contiguous row): free for a Fortran-ordered S (what stft() returns), one host
    # transpose for a C-ordered one
    S_dev = torch.from_numpy(np.ascontiguousarray(S.T, dtype=np.complex64)).to(dev).T
    y = istft_device(S_dev, window_f64(win, nfft, dev), nfft, hop, n_frames, start, out_len).cpu().numpy()
    if np.dtype(dtype) != y.dtype:
        y = y.astype(dtype)
    if max_len:
        y = y[:int(max_len * fs)]      # quirk Q8: max_len is already in samples, so this is a no-op
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# Ragged batches (dvae_stft_batch / dvae_istft_batch): U utterances packed end to end, nfft 1024 / hop 256 (every caller of the
# reference).  The per-utterance decisions (end pad, centre pad, frame count, max_len truncation) are the single-signal ones above,
# made on the host; the offset tables are checked here before upload, and the kernels check them again against the buffers' extents.

BATCH_NFFT, BATCH_HOP = 1024, 256
_SLOTS = 2048                      # one round of waves, as the single-signal walks (256 CUs x 4 SIMDs x 2 resident waves)


def batch_covers(nfft, hop):
    return nfft == BATCH_NFFT and hop == BATCH_HOP


def plan_stft_batch(lengths, fs=16000, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_at_end=True):
    """Per-utterance padding and frame counts of stft() for signals of the given lengths, packed end to end.  Returns a dict of
    numpy int64 arrays: end_pad (0 / 1), padded (samples after end and centre padding), frames (T_u), frame_off [U + 1] (first output
    row of each utterance), x0 (first sample of each padded signal in the packed buffer), plus nfft / hop.  Raises ValueError for a
    signal shorter than nfft after padding (librosa's message)."""
    nfft, hop = sizes(fs, wlen_sec, hop_percent, "STFT")
    lengths = [int(n) for n in lengths]
    if not lengths:
        raise ValueError("stft_batch: no signals")
    end_pad = np.array([1 if pad_at_end and needs_end_pad(n, fs, wlen_sec, hop_percent) else 0 for n in lengths], np.int64)
    padded = np.array(lengths, np.int64) + hop * end_pad + (2 * (nfft // 2) if center else 0)
    frames = np.array([frame_count(int(p), nfft, hop) for p in padded], np.int64)
    frame_off, x0 = R.prefix(frames), R.prefix(padded)[:-1]
    return dict(nfft=nfft, hop=hop, end_pad=end_pad, padded=padded, frames=frames, frame_off=frame_off, x0=x0)


def batch_chunk(frames):
    """Frames per work item: the least rounds of the 2048 wave slots times the frames a wave walks per round.  ceil(T_total / 2048),
    the single-signal choice, leaves up to one partial item per utterance beyond the slots (256 utterances of 5 s: ~2 130 items,
    a second round for 80 waves); a slightly longer chunk keeps the items inside one round."""
    frames = np.asarray(frames, np.int64)
    c0 = max(1, -(-int(frames.sum()) // _SLOTS))
    best = None
    for c in range(c0, 2 * c0 + 2):
        cost = -(-int((-(-frames // c)).sum()) // _SLOTS) * c
        if best is None or cost < best[0]:
            best = (cost, c)
    return best[1]


def stft_tables(frames, x0, padded, n_total, chunk):
    """The int64 table of dvae_stft_batch, [items (U + 1) | frame_off (U + 1) | x0 (U)], after checking that the signals do not
    overlap and lie inside the n_total packed samples, and that every frame lies inside its own signal."""
    frames, x0, padded = (np.asarray(a, np.int64) for a in (frames, x0, padded))
    U = frames.size
    if not (x0.size == U and padded.size == U and U > 0):
        raise ValueError("stft_batch: frames, x0 and padded lengths need one entry per utterance")
    if np.any(frames < 1):
        raise ValueError(f"stft_batch: every utterance needs at least one frame (frames {frames.tolist()[:16]})")
    R.monotone("stft_batch: signal offsets", x0)
    if x0[0] < 0 or np.any(x0[:-1] + padded[:-1] > x0[1:]) or x0[-1] + padded[-1] > n_total:
        raise ValueError("stft_batch: signals overlap or leave the packed buffer")
    if np.any((frames - 1) * BATCH_HOP + BATCH_NFFT > padded):
        raise ValueError("stft_batch: frames beyond the end of their signal")
    if np.any(padded * 8 >= 2 ** 31) or np.any(frames * 513 * 8 >= 2 ** 31):
        raise ValueError("stft_batch: an utterance of 2 GB or more (use the single-signal stft)")
    return np.concatenate([R.item_prefix(frames, chunk), R.prefix(frames), x0]).astype(np.int64)


def istft_tables(f0, nfr, y0, out_len, gcol, T_total, y_total, ldg, chunk):
    """The int64 table of dvae_istft_batch, [items (U + 1) | f0 | nfr | y0 | len | gcol], after checking that every utterance's
    frames lie inside the packed spectrogram, its output inside y (at an even offset, no overlaps) and its gain columns inside the
    gain plane (ldg = None: no gain)."""
    f0, nfr, y0, out_len, gcol = (np.asarray(a, np.int64) for a in (f0, nfr, y0, out_len, gcol))
    U = f0.size
    if U == 0 or any(a.size != U for a in (nfr, y0, out_len, gcol)):
        raise ValueError("istft_batch: the tables need one entry per utterance")
    if np.any(nfr < 1) or np.any(out_len < 0):
        raise ValueError("istft_batch: every utterance needs at least one frame and a non-negative length")
    R.monotone("istft_batch: frame offsets", f0)
    R.monotone("istft_batch: output offsets", y0)
    if f0[0] < 0 or np.any(f0[:-1] + nfr[:-1] > f0[1:]) or f0[-1] + nfr[-1] > T_total:
        raise ValueError("istft_batch: frames overlap or leave the packed spectrogram")
    if y0[0] < 0 or np.any(y0 % 2) or np.any(y0[:-1] + out_len[:-1] > y0[1:]) or y0[-1] + out_len[-1] > y_total:
        raise ValueError("istft_batch: outputs overlap, leave the output buffer or start at an odd sample")
    if ldg is not None and (np.any(gcol < 0) or np.any(gcol + nfr > ldg) or 513 * ldg * 4 >= 2 ** 31):
        raise ValueError("istft_batch: gain columns outside the gain plane (or a plane of 2 GB or more)")
    return np.concatenate([R.item_prefix(nfr, chunk), f0, nfr, y0, out_len, gcol]).astype(np.int64)


class SpecBatch:
    """A ragged batch of spectrograms on the device, as stft_batch returns it.  frames: [sum T_u, 513] frame-major, complex64
    (layout 2) or float32 power (layout 1); utterance u is rows frame_off[u]:frame_off[u + 1] -- the memory order of librosa's
    Fortran-ordered [513, T_u] result, so spec(u) = those rows' `.T`.  counts: T_u; lengths: the signals' own lengths."""

    def __init__(self, frames, counts, lengths, nfft, hop, center, layout):
        self.frames, self.nfft, self.hop, self.center, self.layout = frames, nfft, hop, center, layout
        self.counts = [int(c) for c in counts]
        self.lengths = [int(n) for n in lengths]
        self.frame_off = R.prefix(self.counts)

    def __len__(self):
        return len(self.counts)

    def spec(self, u):
        """Utterance u as a [513, T_u] view on the device."""
        return self.frames[int(self.frame_off[u]):int(self.frame_off[u + 1])].T

    def numpy(self):
        """Every utterance as a host array [513, T_u] (Fortran-ordered views of one host copy)."""
        h = self.frames.cpu().numpy()
        return [h[a:b].T for a, b in zip(self.frame_off[:-1], self.frame_off[1:])]


def stft_packed(x_dev, frames, x0, padded, lengths=None, center=False, layout=2):
    """The batch transform of signals already padded and packed on the device (x_dev: 1-D float32 / float64 CUDA tensor; utterance
    u's padded signal is x_dev[x0[u] : x0[u] + padded[u]], T_u = frames[u]) -> SpecBatch."""
    lib = N.load()
    if not x_dev.is_cuda or x_dev.dim() != 1 or x_dev.dtype not in (torch.float32, torch.float64):
        raise TypeError("stft_batch: 1-D float32/float64 CUDA tensor required")
    if layout not in (1, 2):
        raise ValueError(f"stft_batch: layout 1 (power frames) or 2 (complex frames), got {layout}")
    x_dev = x_dev.contiguous()
    frames = np.asarray(frames, np.int64)
    T_total = int(frames.sum())
    chunk = batch_chunk(frames)
    tab = stft_tables(frames, x0, padded, x_dev.numel(), chunk)
    U = frames.size
    out = torch.empty((T_total, BATCH_NFFT // 2 + 1), dtype=torch.complex64 if layout == 2 else torch.float32, device=x_dev.device)
    tab_dev = R.upload(tab, x_dev.device)
    N.check(lib.dvae_stft_batch(N.ptr(x_dev), R.f64_flag(x_dev), x_dev.numel(), N.ptr(window_f64("hann", BATCH_NFFT, x_dev.device)),
                                BATCH_NFFT, BATCH_HOP, U, N.ptr(tab_dev), int(tab[U]), chunk, T_total, N.ptr(out), layout, N.stream()), "dvae_stft_batch")
    return SpecBatch(out, frames, padded if lengths is None else lengths, BATCH_NFFT, BATCH_HOP, center, layout)


def stft_batch(signals, fs=16000, wlen_sec=64e-3, win="hann", hop_percent=0.25, center=False, pad_mode="reflect", pad_at_end=True, layout=2):
    """stft() of every signal in one launch (nfft 1024 / hop 256 only): the reference's per-utterance end pad, centre pad and frame
    count on the host, the padded signals packed into one buffer and copied to the device once.  Returns a SpecBatch whose every
    frame is bit-identical to stft_device(..., layout) of that utterance alone."""
    nfft, hop = sizes(fs, wlen_sec, hop_percent, "STFT")
    if not batch_covers(nfft, hop):
        raise ValueError(f"stft_batch: nfft {nfft} / hop {hop}: the batch transform covers nfft 1024 / hop 256; use stft() per signal")
    if win != "hann":
        raise ValueError("stft_batch: the batch transform uses the periodic Hann window")
    xs = [np.asarray(x) for x in signals]
    for x in xs:
        if x.ndim != 1 or not np.issubdtype(x.dtype, np.floating):
            raise TypeError("stft_batch: every signal must be a 1-D floating-point array (as librosa requires)")
    plan = plan_stft_batch([len(x) for x in xs], fs, wlen_sec, hop_percent, center, pad_at_end)
    # float32 samples convert to double exactly, and the kernel computes in double whatever it reads: one buffer type serves all
    dt = np.float32 if all(x.dtype == np.float32 for x in xs) else np.float64
    buf = np.empty(int(plan["padded"].sum()), dt)
    for x, e, a, p in zip(xs, plan["end_pad"], plan["x0"], plan["padded"]):
        x_ = np.pad(x, (0, hop), mode="constant") if e else x
        if center:
            x_ = np.pad(x_, int(nfft // 2), mode=pad_mode)
        buf[a:a + p] = x_
    dev = R.device()
    return stft_packed(torch.from_numpy(buf).to(dev), plan["frames"], plan["x0"], plan["padded"], [len(x) for x in xs], center, layout)


def istft_plan(counts, max_len, nfft, hop, center):
    """istft_numpy's per-utterance frame truncation and output length: (n_frames, out_len, start) lists."""
    U = len(counts)
    mls = list(max_len) if isinstance(max_len, (list, tuple, np.ndarray)) else [max_len] * U
    if len(mls) != U:
        raise ValueError(f"istft_batch: {len(mls)} max_len entries for {U} utterances")
    nfr, lens = [], []
    for T, ml in zip(counts, mls):
        n_frames = int(T)
        if ml:
            padded = ml + nfft if center else ml
            n_frames = min(n_frames, int(np.ceil(padded / hop)))
        ntot = nfft + hop * (n_frames - 1)
        if ml is None:
            out_len = ntot - 2 * (nfft // 2) if center else ntot
        else:
            out_len = int(ml)
        nfr.append(n_frames)
        lens.append(max(out_len, 0))
    return nfr, lens, (nfft // 2 if center else 0)


def istft_batch(spec, max_len=None, gain=None, gain_cols=None, center=None):
    """istft() of every utterance of a SpecBatch (complex frames) in one launch -> WaveBatch, bit-identical per utterance to
    istft_device.  max_len: None, one value or one per utterance (istft_numpy's truncation: n_frames = min(T, ceil(padded / hop))).
    gain: None, a float32 CUDA tensor [513, ldg] or a pair of them (McemBatch's bin-major Wiener gains), utterance u's frame t
    scaled by column gain_cols[u] + t, re = g xr and im = g xi in float32; with a pair, two WaveBatches come back from one launch."""
    lib = N.load()
    if not isinstance(spec, SpecBatch) or spec.layout != 2:
        raise TypeError("istft_batch: a SpecBatch of complex frames (layout 2) required")
    if not batch_covers(spec.nfft, spec.hop):
        raise ValueError(f"istft_batch: nfft {spec.nfft} / hop {spec.hop}: the batch transform covers nfft 1024 / hop 256; use istft() per signal")
    center = spec.center if center is None else center
    S = spec.frames
    if not (S.is_cuda and S.dtype == torch.complex64 and S.dim() == 2 and S.shape[1] == 513 and S.is_contiguous()):
        raise TypeError("istft_batch: frames must be a contiguous complex64 [T, 513] CUDA tensor")
    U = len(spec)
    nfr, lens, start = istft_plan(spec.counts, max_len, spec.nfft, spec.hop, center)
    y0 = R.prefix((np.asarray(lens, np.int64) + 63) // 64 * 64)
    y_total = max(int(y0[-1]), 2)
    planes = None if gain is None else (list(gain) if isinstance(gain, (list, tuple)) else [gain])
    ldg = None
    if planes is not None:
        if not 1 <= len(planes) <= 2:
            raise ValueError("istft_batch: one or two gain planes")
        ldg = planes[0].shape[1] if planes[0].dim() == 2 else -1
        for g in planes:
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 2 and g.shape == (513, ldg)):
                raise TypeError("istft_batch: gains must be contiguous float32 CUDA tensors [513, ldg] of one shape")
        if gain_cols is None:
            raise ValueError("istft_batch: gain_cols (the first gain column of each utterance) is required with a gain")
    gcol = np.zeros(U, np.int64) if gain_cols is None else np.asarray(gain_cols, np.int64)
    chunk = batch_chunk(nfr)
    tab = istft_tables(spec.frame_off[:-1], nfr, y0[:-1], lens, gcol, S.shape[0], y_total, ldg, chunk)
    tab_dev = R.upload(tab, S.device)
    ys = [torch.empty(y_total, dtype=torch.float32, device=S.device) for _ in range(1 if planes is None else len(planes))]
    g0 = planes[0] if planes else None
    g1 = planes[1] if planes and len(planes) > 1 else None
    N.check(lib.dvae_istft_batch(N.ptr(S), S.shape[0], N.ptr(window_f64("hann", BATCH_NFFT, S.device)), BATCH_NFFT, BATCH_HOP, U, N.ptr(tab_dev),
                                 int(tab[U]), chunk, start, N.ptr(ys[0]), y_total, N.ptr(g0), N.ptr(g1), ldg or 0,
                                 N.ptr(ys[1]) if g1 is not None else None, N.stream()), "dvae_istft_batch")
    out = [WaveBatch(y, y0[:-1], lens) for y in ys]
    return out[0] if planes is None or len(planes) == 1 else tuple(out)

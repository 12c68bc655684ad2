"""Resampling on the device: the rational polyphase resampler of include/dvae.h (dvae_resample_batch) for a ragged batch of signals in
one launch -- the step in front of mix -> stft -> MCEM -> Wiener -> istft -> score that brings the raw 48 kHz / 44.1 kHz noise
recordings to 16 kHz (the reference's packages/dataset/qut_database.py:63-83, preprocess_noise, which asks librosa.resample).  The
outputs stay on the device as a WaveBatch that mix_at_snr_batch takes as its noise banks.

librosa.resample (resampy's kaiser_best table) is not available to this repository: parity with it is unpinned, the contract is the
header's algorithm (restated in numpy by tests/estoi_ref.py::resample), with the Kaiser-windowed sinc of metrics.stoi_taps for any
target rate unless the caller brings taps.  resample_taps, phase_major, resample_run, resample_tables and resample_numpy are host
logic and need no GPU; resample_packed and resample_batch raise without the library or a GPU.
"""
from fractions import Fraction

import numpy as np
import torch

from . import native as N
from . import ragged as R

RESAMPLE_SPAN, RESAMPLE_MAX_RUN, UNIFORM_P = 1240, 4096, 16        # DVAE_RESAMPLE_SPAN, DVAE_RESAMPLE_MAX_RUN, kRsUniformP (csrc/resample.hip)
MAX_RATIO, MAX_L, MAX_LEN, MAX_STRIDE = 1 << 15, 1 << 24, 1 << 31, 1 << 20


def _rate(name, fs):
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs <= 0:
        raise ValueError(f"resample_batch: {name} must be a positive integer (got {fs!r})")
    return int(fs)


def resample_ratio(fs_in, fs_out):
    """p / q = fs_out / fs_in reduced.  ValueError for fs_in == fs_out (nothing to resample) and a ratio beyond what the kernel takes."""
    f = Fraction(_rate("fs_out", fs_out), _rate("fs_in", fs_in))
    p, q = f.numerator, f.denominator
    if p == q:
        raise ValueError(f"resample_batch: fs_in == fs_out ({fs_in} Hz): nothing to resample")
    if max(p, q) > MAX_RATIO:
        raise ValueError(f"resample_batch: {fs_in} Hz -> {fs_out} Hz needs a {p} / {q} resampler, beyond what the kernel takes")
    return p, q


def resample_taps(fs_in, fs_out):
    """-> (taps float64 [2 L + 1], p, q, L): the Kaiser-windowed sinc of metrics.stoi_taps (Octave's resample: 60 dB, cutoff at the
    lower Nyquist rate) for any target rate, normalised to sum 1, for scipy.signal.resample_poly(x, p, q, window=taps);
    p / q = fs_out / fs_in reduced.  fs_out = 10000 gives the bits of stoi_taps(fs_in)."""
    p, q = resample_ratio(fs_in, fs_out)
    fc = 1.0 / (2.0 * max(p, q))
    L = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return h / np.sum(h), p, q, L


def check_taps(taps, p, q):
    """Caller's taps as float64 [2 L + 1] -> (taps, L).  ValueError unless 1-D, odd, at least 3 and finite, with p != q in range."""
    h = np.ascontiguousarray(taps, np.float64)
    if h.ndim != 1 or h.size < 3 or h.size % 2 == 0 or not np.all(np.isfinite(h)):
        raise ValueError(f"resample_batch: taps must be a finite 1-D array of odd length >= 3 (got shape {h.shape})")
    L = (h.size - 1) // 2
    if not (1 <= p <= MAX_RATIO and 1 <= q <= MAX_RATIO and p != q and L <= MAX_L):
        raise ValueError(f"resample_batch: p != q in 1 ... 2^15 and L <= 2^24 are required (got p {p}, q {q}, L {L})")
    return h, L


def phase_major(taps, p):
    """The taps as the kernel reads them: float64 [p, 2 L / p + 1], row j0 = taps[j0::p], zeros past the row's own count."""
    h = np.asarray(taps, np.float64)
    nt = (h.size - 1) // p + 1
    out = np.zeros((p, nt))
    for j0 in range(min(p, h.size)):
        row = h[j0::p]
        out[j0, :row.size] = row
    return out


def resample_run(p, q, L):
    """The outputs per work item (dvae_resample_run; rs_plan in csrc/resample.hip): the largest multiple of 64 p (p <= 16 and such a
    run fits; else of 64), at most RESAMPLE_MAX_RUN, whose input span ceil((run - 1) q / p) + 1 + nt fits RESAMPLE_SPAN samples.
    0: the smallest run does not fit."""
    nt = 2 * L // p + 1
    room = RESAMPLE_SPAN - nt - 1
    if room < 1:
        return 0
    rmax = room * p // q + 1
    unit = 64 * p if p <= UNIFORM_P and 64 * p <= rmax else 64
    if rmax < unit:
        return 0
    return unit * max(1, min(rmax, RESAMPLE_MAX_RUN) // unit)


def resampled_length(n, p, q):
    return -(-np.asarray(n, np.int64) * p // q)


def resample_tables(x_view, p, q, L, stride=1, out_layout=None):
    """The host side of dvae_resample_batch -> dict: `table`, the int64 table [items (U + 1) | x0 (U) | len (U) | y0 (U)]; `U`,
    `n_items`, `run`; `out0` and `out_len` (ceil(len p / q)) per signal and `n_out`, the element count the output buffer needs.

    x_view: (x0, lengths, n_x): the first element and the samples of every signal, sample i at x0 + i stride, in a buffer of n_x
    elements.  out_layout: None (the outputs packed end to end at multiples of 64 samples) or (y0, n_y).
    ValueError naming the signal for an empty one, one of more than 2^31 samples, one that leaves the input buffer and output ranges
    that overlap or leave theirs; ValueError for a stride outside 1 ... 2^20 and a ratio / filter that does not fit the kernel's tile."""
    x0, length = (np.asarray(a, np.int64).reshape(-1) for a in x_view[:2])
    n_x, U, stride = int(x_view[2]), x0.size, int(stride)
    if U == 0 or length.size != U:
        raise ValueError(f"resample_batch: the tables need one entry per signal (got {U} offsets, {length.size} lengths)")
    if not 1 <= stride <= MAX_STRIDE:
        raise ValueError(f"resample_batch: stride {stride}: 1 ... 2^20 is required")
    run = resample_run(p, q, L)
    if run == 0:
        raise ValueError(f"resample_batch: 64 outputs at {p} / {q} with {2 * L // p + 1} taps each need more than the {RESAMPLE_SPAN} "
                         "input samples a tile holds")

    def first(mask):
        bad = np.flatnonzero(mask)
        return int(bad[0]) if bad.size else None

    u = first(length < 1)
    if u is not None:
        raise ValueError(f"resample_batch: signal {u} is empty")
    u = first(length > MAX_LEN)
    if u is not None:
        raise ValueError(f"resample_batch: signal {u} has {int(length[u])} samples: more than 2^31")
    u = first((x0 < 0) | (x0 + (length - 1) * stride >= n_x))
    if u is not None:
        raise ValueError(f"resample_batch: signal {u} ({int(length[u])} samples from {int(x0[u])} at stride {stride}) leaves its buffer "
                         f"({n_x} elements)")
    out_len = resampled_length(length, p, q)
    if out_layout is None:
        y0 = R.prefix((out_len + 63) // 64 * 64)[:-1]
        n_out = int(y0[-1] + out_len[-1])
    else:
        y0, n_out = np.asarray(out_layout[0], np.int64).reshape(-1), int(out_layout[1])
        if y0.size != U:
            raise ValueError(f"resample_batch: y0 has {y0.size} entries for {U} signals")
        u = first((y0 < 0) | (y0 + out_len > n_out))
        if u is not None:
            raise ValueError(f"resample_batch: signal {u} of the output ([{int(y0[u])}, {int(y0[u] + out_len[u])})) leaves its buffer "
                             f"({n_out} elements)")
        order = np.argsort(y0, kind="stable")
        clash = np.flatnonzero(y0[order][:-1] + out_len[order][:-1] > y0[order][1:])
        if clash.size:
            raise ValueError(f"resample_batch: the output ranges of signals {int(order[clash[0]])} and {int(order[clash[0] + 1])} overlap")
    items = R.item_prefix(out_len, run)
    return {"table": np.concatenate([items, x0, length, y0]).astype(np.int64), "U": U, "n_items": int(items[-1]), "run": run,
            "out0": y0, "out_len": out_len, "n_out": n_out}


_taps_dev = {}


def _device_taps(taps, p, dev):
    """The phase-major taps of one filter on one device, built and uploaded once."""
    key = (str(dev), p, taps.size, hash(taps.tobytes()))
    if key not in _taps_dev:
        _taps_dev[key] = R.upload(phase_major(taps, p).reshape(-1), dev)
    return _taps_dev[key]


def resample_packed(buf, tab, taps, p, q, stride=1, out_dtype=torch.float64, n_out=None, out=None):
    """dvae_resample_batch on a packed device buffer: buf a 1-D float32 / float64 CUDA tensor, tab the int64 table of resample_tables
    over it (its `table`), taps the float64 [2 L + 1] filter (not yet phase-major).  n_out: the element count of the output buffer
    (default: the end of the last output range); out: a preallocated 1-D tensor of out_dtype to write into instead.
    -> the output buffer on the device.  Nothing is synchronised: the call enqueues on the current stream."""
    lib = N.load()
    dev = R.check_packed("resample_batch", [("signals", buf)])
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"resample_batch: out_dtype float32 or float64 (got {out_dtype})")
    taps, L = check_taps(taps, p, q)
    tab = np.asarray(tab, np.int64)
    U = (tab.size - 1) // 4
    if U < 1 or tab.size != 4 * U + 1:
        raise ValueError(f"resample_batch: a table of 4 U + 1 entries is required (got {tab.size})")
    n_items = int(tab[U])
    if n_out is None:
        n_out = int(np.max(tab[3 * U + 1:] + resampled_length(tab[2 * U + 1:3 * U + 1], p, q)))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n_out, dtype=out_dtype, device=dev)
        if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dim() == 1 and out.dtype == out_dtype and out.is_contiguous()
                and out.numel() == n_out):
            raise TypeError(f"resample_batch: the output must be a contiguous 1-D {out_dtype} tensor of {n_out} elements on {dev}")
        tab_dev, taps_dev = R.upload(tab, dev), _device_taps(taps, p, dev)
        N.check(lib.dvae_resample_batch(N.ptr(buf), buf.numel(), R.f64_flag(buf), int(stride), N.ptr(out), n_out, R.f64_flag(out), U,
                                        N.ptr(tab_dev), n_items, N.ptr(taps_dev), p, q, L, N.stream()), "dvae_resample_batch")
    return out


def _flat_signals(signals, channel):
    """The signals as 1-D arrays / tensors of interleaved samples -> (flat list, samples per signal, channels)."""
    x = [signals] if torch.is_tensor(signals) or isinstance(signals, np.ndarray) else list(signals)
    if not x:
        raise ValueError("resample_batch: no signals")
    flat, lengths, C = [], [], None
    for u, a in enumerate(x):
        if not (torch.is_tensor(a) or isinstance(a, np.ndarray)):
            a = np.asarray(a)
        nd = a.dim() if torch.is_tensor(a) else a.ndim
        if nd not in (1, 2) or (nd == 2) != (channel is not None):
            raise ValueError(f"resample_batch: signal {u} has {nd} dimensions: 1-D, or [n, C] with `channel` given, is required")
        if not (a.dtype.is_floating_point if torch.is_tensor(a) else np.issubdtype(a.dtype, np.floating)):
            raise TypeError(f"resample_batch: signal {u} is not floating point ({a.dtype})")
        c = int(a.shape[1]) if nd == 2 else 1
        if a.shape[0] == 0 or c == 0:
            raise ValueError(f"resample_batch: signal {u} is empty")
        if a.shape[0] > MAX_LEN:
            raise ValueError(f"resample_batch: signal {u} has {int(a.shape[0])} samples: more than 2^31")
        if C is not None and c != C:
            raise ValueError(f"resample_batch: signal {u} has {c} channels, signal 0 {C}: one stride serves the whole batch")
        C = c
        if nd == 2 and not 0 <= int(channel) < c:
            raise ValueError(f"resample_batch: signal {u} has no channel {channel} ({c} channels)")
        lengths.append(int(a.shape[0]))
        flat.append(a.contiguous().reshape(-1) if torch.is_tensor(a) else np.ascontiguousarray(a).reshape(-1))
    return flat, lengths, C


def resample_batch(signals, fs_in, fs_out, taps=None, channel=None, out_dtype=torch.float64):
    """Every signal resampled from fs_in to fs_out Hz in one launch.

    signals: a list of numpy arrays or CUDA tensors (or one), float32 or float64: 1-D, or [n, C] with `channel` given -- the channel is
    read in place at a stride of C, as the reference's noise_audio[:, 0]; host arrays are packed into one pinned buffer and uploaded
    once.  taps: the caller's own odd-length filter [2 L + 1] for scipy.signal.resample_poly(x, p, q, window=taps) in place of
    resample_taps(fs_in, fs_out).  out_dtype: float64, or float32 (one more rounding of the double result).
    -> WaveBatch on the device, signal u of ceil(n_u p / q) samples.  ValueError naming the signal for an empty one and one of more
    than 2^31 samples; ValueError for fs_in == fs_out.  Nothing is synchronised: the call enqueues on the current stream."""
    if taps is None:
        taps, p, q, L = resample_taps(fs_in, fs_out)
    else:
        p, q = resample_ratio(fs_in, fs_out)
        taps, L = check_taps(taps, p, q)
    flat, lengths, C = _flat_signals(signals, channel)
    # the table is built (and refuses) before anything is uploaded or the library is loaded
    offs, _, total = R.view(flat)
    t = resample_tables((offs + (0 if channel is None else int(channel)), lengths, total), p, q, L, C)
    dev = R.find_device(flat)
    with torch.cuda.device(dev):
        buf = R.pack(flat, "resample_batch: signals", dev, ("signal", "signals"))
    y = resample_packed(buf, t["table"], taps, p, q, C, out_dtype, t["n_out"])
    return R.WaveBatch(y, t["out0"], t["out_len"])


def resample_numpy(x, taps, p, q, block=1 << 15):
    """The contract of dvae_resample_batch in float64 numpy, a block of outputs at a time (the sum of an output's products in the order
    of numpy's matrix product, not the kernel's: equal within the rounding of nt terms, not bit for bit) -> float64 [ceil(n p / q)].
    What preprocess_noise runs where no GPU is present."""
    x = np.asarray(x, np.float64).reshape(-1)
    h, L = check_taps(taps, p, q)
    n, n_out = x.size, int(resampled_length(x.size, p, q))
    hp = phase_major(h, p)
    nt = hp.shape[1]
    out = np.zeros(n_out)
    t = np.arange(nt)
    for k0 in range(0, n_out, block):
        k = np.arange(k0, min(k0 + block, n_out), dtype=np.int64)
        j0 = (L - k * q) % p
        src0 = (k * q + j0 - L) // p
        lo, hi = int(src0[0]), int(src0[-1]) + nt
        seg = np.zeros(hi - lo)
        a, b = max(lo, 0), min(hi, n)
        if b > a:
            seg[a - lo:b - lo] = x[a:b]
        out[k] = p * np.einsum("kt,kt->k", seg[(src0 - lo)[:, None] + t[None, :]], hp[j0])
    return out

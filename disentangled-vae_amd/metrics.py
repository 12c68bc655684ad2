"""Scoring on the device: the scale-invariant energy ratios of the reference's packages/metrics.py:12-82 (si_sdr_components,
energy_ratios, si_sdr_leroux) for a ragged batch of utterances in three launches (include/dvae.h: dvae_si_ratios_batch), the last
stage of stft -> MCEM -> Wiener -> istft -> score (scripts/run_metrics.py:86-131).  Only the U x 3 results need to cross to the host.
No CPU arithmetic exists here: without the library or a GPU the scoring functions raise; ratio_tables is host logic and needs neither.

Intelligibility: stoi_batch / estoi_batch (include/dvae.h: dvae_estoi_batch, six launches) score STOI (Taal et al. 2011) and ESTOI
(Jensen & Taal 2016) as the header writes the algorithm out, laid out the way the pystoi package does it -- run_metrics.py:117-138
calls stoi(s_t, s_hat_t, fs, extended=True).  pystoi is not available to this repository: parity with the package is unpinned, the
contract is the header's algorithm (restated in numpy by tests/estoi_ref.py).  stoi_tables is host logic and needs no GPU.
"""
from fractions import Fraction

import numpy as np
import torch

from . import native as N
from . import ragged as R

SI_CHUNK = 4096            # samples per work item (DVAE_SI_CHUNK): fixed, so an utterance's sums never depend on the rest of the batch
NAMES = ("s_hat", "s", "n")
SUMS = ("dot_s", "ss", "dot_n", "nn", "e_noise_art", "e_art", "s_target", "e_noise")      # the columns of the [U, 8] sums


def ratio_tables(views, totals, trim=0):
    """The int64 table of dvae_si_ratios_batch, [items (U + 1) | s_hat0 (U) | s0 (U) | n0 (U) | len (U)].

    views: (offsets, lengths) of the utterances inside the packed buffers of s_hat, s and n, in that order; the third may be None or
    left out (no noise: n0 is zero).  totals: the element count of each buffer.  trim: samples dropped at both ends of every utterance
    (run_metrics.py:117-121 cuts 0.05 s "to remove bursts") by moving the offsets.  ValueError naming the utterance for unequal
    lengths between the views of one utterance, for an utterance not longer than 2 * trim, and for one outside its buffer."""
    views = [v for v in views if v is not None]
    if len(views) not in (2, 3) or len(totals) < len(views):
        raise ValueError("si_ratios_batch: views of s_hat and s (and n), with the element count of each buffer")
    offs, length, U = R.paired_views("si_ratios_batch", NAMES, views, totals, trim)
    cols = offs + [np.zeros(U, np.int64)] * (3 - len(offs))
    return np.concatenate([R.item_prefix(length, SI_CHUNK)] + cols + [length]).astype(np.int64)


def si_ratios_packed(bufs, tab, want_ratios=True, want_sums=False):
    """dvae_si_ratios_batch on packed device buffers: bufs = [s_hat, s] or [s_hat, s, n] (1-D float32 / float64 CUDA tensors on one
    device), tab the table of ratio_tables over them.  -> (ratios [U, 3] or None, sums [U, 8] or None), float64 on the device."""
    lib = N.load()
    bufs = [b for b in bufs if b is not None]
    dev = R.check_packed("si_ratios_batch", list(zip(NAMES, bufs)))
    tab = np.asarray(tab, np.int64)
    U = (tab.size - 1) // 5
    if U < 1 or tab.size != 5 * U + 1:
        raise ValueError(f"si_ratios_batch: a table of 5 U + 1 entries is required (got {tab.size})")
    n_items = int(tab[U])
    with torch.cuda.device(dev):
        ratios = torch.empty((U, 3), dtype=torch.float64, device=dev) if want_ratios else None
        sums = torch.empty((U, 8), dtype=torch.float64, device=dev) if want_sums else None
        ws = torch.empty(lib.dvae_si_ratios_workspace_bytes(n_items), dtype=torch.uint8, device=dev)
        tab_dev = R.upload(tab, dev)
        n = bufs[2] if len(bufs) == 3 else None
        f64 = R.f64_flag
        N.check(lib.dvae_si_ratios_batch(N.ptr(bufs[0]), bufs[0].numel(), f64(bufs[0]), N.ptr(bufs[1]), bufs[1].numel(), f64(bufs[1]),
                                         N.ptr(n), n.numel() if n is not None else 0, f64(n), U, N.ptr(tab_dev), n_items,
                                         N.ptr(ratios), N.ptr(sums), N.ptr(ws), N.stream()), "dvae_si_ratios_batch")
    return ratios, sums


def _score(s_hat, s, n, trim, return_sums):
    args = [R.as_list(a, f"si_ratios_batch: {name}") for a, name in zip((s_hat, s, n), NAMES) if a is not None]
    # the table is built (and refuses) before anything is uploaded or the library is loaded
    views = [R.view(a) for a in args]
    tab = ratio_tables([(o, l) for o, l, _ in views], [t for _, _, t in views], trim)
    dev = R.find_device(*args)
    with torch.cuda.device(dev):
        bufs = [R.pack(a, f"si_ratios_batch: {name}", dev) for a, name in zip(args, NAMES)]
    return si_ratios_packed(bufs, tab, True, return_sums)


def energy_ratios_batch(s_hat, s, n, trim=0, return_sums=False):
    """energy_ratios (packages/metrics.py:39-60) of every utterance: s_hat (estimate), s (clean speech), n (noise), each a WaveBatch
    or a list of 1-D numpy arrays / tensors (float32 or float64; host lists are packed and uploaded once).  trim: samples dropped at
    both ends of every utterance.  -> float64 CUDA tensor [U, 3] of SI-SDR, SI-SIR, SI-SAR in dB (and the [U, 8] sums of
    dvae_si_ratios_batch with return_sums)."""
    if n is None:
        raise ValueError("energy_ratios_batch: the noise is required (si_sdr_batch is the form without it)")
    ratios, sums = _score(s_hat, s, n, trim, return_sums)
    return (ratios, sums) if return_sums else ratios


def si_sdr_batch(s_hat, s, trim=0, return_sums=False):
    """si_sdr_leroux (packages/metrics.py:62-82) of every utterance -> float64 CUDA tensor [U] in dB."""
    ratios, sums = _score(s_hat, s, None, trim, return_sums)
    return (ratios[:, 0], sums) if return_sums else ratios[:, 0]


# ---- STOI / ESTOI ------------------------------------------------------------------------------------------------------------------------

STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_MINFREQ, STOI_SEG = 10000, 256, 128, 512, 15, 150, 30
STOI_RES_RUN, STOI_FRAME_RUN, STOI_SEG_RUN = 256, 16, 8          # DVAE_ESTOI_RES_RUN (times p), DVAE_ESTOI_FRAME_RUN, DVAE_ESTOI_SEG_RUN
STOI_NAMES = ("x", "y")
INFO = ("resampled", "kept_frames", "segments")                   # the columns of the [U, 3] info


def stoi_frames_silent(n):
    """Frames of the silent-frame removal in n samples: starts i = 0, 128, ... with i + 256 <= n (es_frames_silent in csrc/estoi.hip)."""
    n = np.asarray(n, np.int64)
    return np.where(n >= STOI_FRAME, (n - STOI_FRAME) // STOI_HOP + 1, 0)


def stoi_frames_spec(n):
    """Frames of the spectra in n samples: starts i = 0, 128, ... with i + 256 < n, strict (es_frames_spec in csrc/estoi.hip)."""
    n = np.asarray(n, np.int64)
    return np.where(n > STOI_FRAME, (n - STOI_FRAME - 1) // STOI_HOP + 1, 0)


def stoi_window():
    return np.hanning(STOI_FRAME + 2)[1:-1]


def stoi_band_edges():
    """int64 [16]: band b sums the bins [edges[b], edges[b + 1]) nearest to 150 * 2^((2 b -+ 1) / 6) Hz of the 512-point spectrum at 10 kHz."""
    f = np.linspace(0, STOI_FS, STOI_NFFT + 1)[:STOI_NFFT // 2 + 1]
    cf = STOI_MINFREQ * 2.0 ** (np.arange(STOI_BANDS, dtype=np.float64) / 3.0)
    lo = [int(np.argmin(np.square(f - c * 2.0 ** (-1.0 / 6.0)))) for c in cf]
    hi = [int(np.argmin(np.square(f - c * 2.0 ** (1.0 / 6.0)))) for c in cf]
    if lo[1:] != hi[:-1]:
        raise RuntimeError("stoi_band_edges: the third-octave bands do not tile")
    return np.asarray(lo + hi[-1:], np.int64)


def stoi_taps(fs):
    """-> (taps float64 [2 L + 1] or None when fs == 10000, p, q, L): the Kaiser-windowed sinc that pystoi takes from Octave's
    resample, normalised to sum 1, for scipy.signal.resample_poly(x, p, q, window=taps); p / q = 10000 / fs reduced."""
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs <= 0:
        raise ValueError(f"stoi_batch: fs must be a positive integer (got {fs!r})")
    f = Fraction(STOI_FS, int(fs))
    p, q = f.numerator, f.denominator
    if p == q:
        return None, 1, 1, 0
    if max(p, q) > 1 << 15:
        raise ValueError(f"stoi_batch: fs = {fs} needs a {p} / {q} resampler, beyond what the kernel takes")
    fc = 1.0 / (2.0 * max(p, q))
    L = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return h / np.sum(h), p, q, L


def stoi_tables(views, totals, fs, trim=0):
    """The host side of dvae_estoi_batch -> dict: `table`, the int64 table [items_res (U + 1) | items_frame (U + 1) | items_seg (U + 1) |
    x0 (U) | y0 (U) | len (U) | r0 (U) | f0 (U)]; `taps`, `p`, `q`, `L` (stoi_taps); `bands` (stoi_band_edges); `window`; `U`, `n_res`,
    `n_frames` (the workspace extents: resampled samples and frames of all utterances) and `resampled`, `frames` per utterance.

    views: (offsets, lengths) of the utterances inside the packed buffers of x (clean) and y (processed); totals: the element count of
    each buffer; trim: samples dropped at both ends of every utterance by moving the offsets.  ValueError naming the utterance for
    unequal lengths, for an utterance not longer than 2 * trim, and for one outside its buffer; ValueError for an fs that is not a
    positive integer."""
    taps, p, q, L = stoi_taps(fs)
    if len(views) != 2 or len(totals) < 2:
        raise ValueError("stoi_batch: views of x and y, with the element count of each buffer")
    offs, length, U = R.paired_views("stoi_batch", STOI_NAMES, views, totals, trim)
    if np.any(length > 1 << 31):
        raise ValueError("stoi_batch: an utterance of more than 2^31 samples")
    n10 = -(-length * p // q)
    J = stoi_frames_silent(n10)
    items = [np.maximum(1, -(-n10 // (STOI_RES_RUN * p))), np.maximum(1, -(-J // STOI_FRAME_RUN)),
             np.maximum(1, -(-np.maximum(J - STOI_SEG, 0) // STOI_SEG_RUN))]
    table = np.concatenate([R.prefix(i) for i in items] + offs + [length, R.prefix(n10)[:-1], R.prefix(J)[:-1]]).astype(np.int64)
    return {"table": table, "taps": taps, "p": p, "q": q, "L": L, "bands": stoi_band_edges(), "window": stoi_window(), "U": U,
            "n_res": int(n10.sum()), "n_frames": int(J.sum()), "resampled": n10, "frames": J}


_stoi_consts = {}


def _stoi_device_consts(t, dev):
    """The window, the band edges and the taps of one sampling ratio on one device, uploaded once."""
    key = (str(dev), t["p"], t["q"])
    if key not in _stoi_consts:
        _stoi_consts[key] = (R.upload(t["window"], dev), R.upload(t["bands"], dev), None if t["taps"] is None else R.upload(t["taps"], dev))
    return _stoi_consts[key]


def stoi_packed(bufs, t, extended=False, return_info=False, return_tob=False, table=None):
    """dvae_estoi_batch on packed device buffers: bufs = [x, y] (1-D float32 / float64 CUDA tensors on one device), t what stoi_tables
    returned over them (table: another int64 table in place of t's).  -> d [U] float64 on the device (and info [U, 3] int64, and the
    debug output tob [2, n_frames, 15], NaN where no frame was written)."""
    lib = N.load()
    dev = R.check_packed("stoi_batch", list(zip(STOI_NAMES, bufs)))
    tab = np.asarray(t["table"] if table is None else table, np.int64)
    U = t["U"]
    if tab.size != 8 * U + 3:
        raise ValueError(f"stoi_batch: a table of 8 U + 3 entries is required (got {tab.size})")
    n_items = [int(t["table"][c * (U + 1) + U]) for c in range(3)]
    with torch.cuda.device(dev):
        d = torch.empty(U, dtype=torch.float64, device=dev)
        info = torch.empty((U, 3), dtype=torch.int64, device=dev) if return_info else None
        tob = torch.full((2, max(t["n_frames"], 1), STOI_BANDS), float("nan"), dtype=torch.float64, device=dev) if return_tob else None
        ws = torch.empty(lib.dvae_estoi_workspace_bytes(t["n_res"], t["n_frames"], n_items[2], U), dtype=torch.uint8, device=dev)
        window, bands, taps = _stoi_device_consts(t, dev)
        tab_dev = R.upload(tab, dev)
        f64 = R.f64_flag
        N.check(lib.dvae_estoi_batch(N.ptr(bufs[0]), bufs[0].numel(), f64(bufs[0]), N.ptr(bufs[1]), bufs[1].numel(), f64(bufs[1]), U,
                                     N.ptr(tab_dev), n_items[0], n_items[1], n_items[2], t["n_res"], t["n_frames"], N.ptr(taps), t["p"], t["q"],
                                     t["L"], N.ptr(window), N.ptr(bands), 1 if extended else 0, N.ptr(d), N.ptr(info), N.ptr(tob), N.ptr(ws),
                                     N.stream()), "dvae_estoi_batch")
    out = (d,) + ((info,) if return_info else ()) + ((tob,) if return_tob else ())
    return out if len(out) > 1 else d


def stoi_batch(x, y, fs, extended=False, trim=0, return_info=False):
    """STOI (extended=True: ESTOI) of every utterance, pystoi's argument order and default: x the clean speech, y the processed
    speech, each a WaveBatch or a list of 1-D numpy arrays / tensors (float32 or float64; host lists are packed and uploaded once),
    fs their sampling rate (a positive integer; anything but 10 kHz is resampled on the device).  trim: samples dropped at both ends of
    every utterance.  -> float64 CUDA tensor [U] (and the int64 [U, 3] of resampled length, kept frames and segments with
    return_info).  An utterance with fewer than 30 spectral frames scores 1e-5."""
    args = [R.as_list(a, f"si_ratios_batch: {name}") for a, name in zip((x, y), STOI_NAMES)]     # (the messages have always said si_ratios_batch)
    views = [R.view(a) for a in args]
    t = stoi_tables([(o, l) for o, l, _ in views], [n for _, _, n in views], fs, trim)      # refuses before anything is uploaded
    dev = R.find_device(*args)
    with torch.cuda.device(dev):
        bufs = [R.pack(a, f"si_ratios_batch: {name}", dev) for a, name in zip(args, STOI_NAMES)]
    return stoi_packed(bufs, t, extended, return_info)


def estoi_batch(x, y, fs, trim=0, return_info=False):
    """stoi_batch(..., extended=True)."""
    return stoi_batch(x, y, fs, True, trim, return_info)

"""Scoring on the device: the scale-invariant energy ratios of the reference's packages/metrics.py:12-82 (si_sdr_components,
energy_ratios, si_sdr_leroux) for a ragged batch of utterances in three launches (include/dvae.h: dvae_si_ratios_batch), the last
stage of stft -> MCEM -> Wiener -> istft -> score (scripts/run_metrics.py:86-131).  Only the U x 3 results need to cross to the host.
No CPU arithmetic exists here: without the library or a GPU the scoring functions raise; ratio_tables is host logic and needs neither.
"""
import numpy as np
import torch

from . import native as N
from . import stft as H

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
    trim = int(trim)
    if trim < 0:
        raise ValueError(f"si_ratios_batch: trim must not be negative (got {trim})")
    offs = [np.asarray(o, np.int64).reshape(-1) for o, _ in views]
    lens = [np.asarray(n, np.int64).reshape(-1) for _, n in views]
    U = offs[0].size
    if U == 0:
        raise ValueError("si_ratios_batch: no utterances")
    for name, o, n in zip(NAMES, offs, lens):
        if o.size != U or n.size != U:
            raise ValueError(f"si_ratios_batch: {name} holds {max(o.size, n.size)} utterances, s_hat {U}")
    for name, n in zip(NAMES[1:], lens[1:]):
        bad = np.flatnonzero(n != lens[0])
        if bad.size:
            u = int(bad[0])
            raise ValueError(f"si_ratios_batch: utterance {u}: s_hat has {int(lens[0][u])} samples, {name} {int(n[u])}")
    short = np.flatnonzero(lens[0] <= 2 * trim)
    if short.size:
        u = int(short[0])
        raise ValueError(f"si_ratios_batch: utterance {u} has {int(lens[0][u])} samples: "
                         + (f"not longer than 2 * trim = {2 * trim}" if trim else "at least one is needed"))
    for name, o, total in zip(NAMES, offs, totals):
        bad = np.flatnonzero((o < 0) | (o + lens[0] > int(total)))
        if bad.size:
            u = int(bad[0])
            raise ValueError(f"si_ratios_batch: utterance {u} of {name} ([{int(o[u])}, {int(o[u] + lens[0][u])})) leaves its buffer ({int(total)} elements)")
    length = lens[0] - 2 * trim
    cols = [o + trim for o in offs] + [np.zeros(U, np.int64)] * (3 - len(offs))
    return np.concatenate([H._items(length, SI_CHUNK)] + cols + [length]).astype(np.int64)


def _utterances(x, name):
    """A WaveBatch as it is; anything else as a list of 1-D arrays / tensors (one array or tensor: a batch of one)."""
    if isinstance(x, H.WaveBatch):
        y = x.y
        if not (torch.is_tensor(y) and y.is_cuda and y.dim() == 1 and y.dtype in (torch.float32, torch.float64)):
            raise TypeError(f"si_ratios_batch: {name}: a WaveBatch over a 1-D float32 / float64 CUDA tensor is required")
        return x
    x = [x] if torch.is_tensor(x) or isinstance(x, np.ndarray) else list(x)
    if not x:
        raise ValueError(f"si_ratios_batch: {name}: no utterances")
    for u, a in enumerate(x):
        if getattr(a, "ndim", None) != 1:
            raise ValueError(f"si_ratios_batch: {name}: utterance {u} is not a 1-D array or tensor")
    return x


def _view(x):
    """(offsets, lengths, element count) of the packed buffer that _buffer makes of x."""
    if isinstance(x, H.WaveBatch):
        return x.offsets, x.lengths, x.y.numel()
    lengths = [int(a.shape[0]) for a in x]
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64), lengths, int(np.sum(lengths))


def _buffer(x, name, dev):
    """The packed 1-D float32 / float64 CUDA tensor of x: a WaveBatch's own, device tensors concatenated, host arrays packed into
    one pinned buffer and uploaded once."""
    if isinstance(x, H.WaveBatch):
        return x.y.contiguous()
    if all(torch.is_tensor(a) and a.is_cuda for a in x):
        dt = torch.float32 if all(a.dtype == torch.float32 for a in x) else torch.float64
        return torch.cat([a.to(dt) for a in x]).contiguous()
    if any(torch.is_tensor(a) and a.is_cuda for a in x):
        raise TypeError(f"si_ratios_batch: {name} mixes host and device utterances")
    xs = [a.detach().numpy() if torch.is_tensor(a) else np.asarray(a) for a in x]
    for u, a in enumerate(xs):
        if not np.issubdtype(a.dtype, np.floating):
            raise TypeError(f"si_ratios_batch: {name}: utterance {u} is not floating point ({a.dtype})")
    # float32 samples convert to double exactly, and the kernels compute in double whatever they read: one buffer type serves all
    dt = torch.float32 if all(a.dtype == np.float32 for a in xs) else torch.float64
    host = torch.empty(sum(len(a) for a in xs), dtype=dt, pin_memory=True)
    h, o = host.numpy(), 0
    for a in xs:
        h[o:o + len(a)] = a
        o += len(a)
    return host.to(dev, non_blocking=True)


def _device(args):
    for a in args:
        if isinstance(a, H.WaveBatch) and torch.is_tensor(a.y) and a.y.is_cuda:
            return a.y.device
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
        if isinstance(a, (list, tuple)):
            for t in a:
                if torch.is_tensor(t) and t.is_cuda:
                    return t.device
    return H._device()


def si_ratios_packed(bufs, tab, want_ratios=True, want_sums=False):
    """dvae_si_ratios_batch on packed device buffers: bufs = [s_hat, s] or [s_hat, s, n] (1-D float32 / float64 CUDA tensors on one
    device), tab the table of ratio_tables over them.  -> (ratios [U, 3] or None, sums [U, 8] or None), float64 on the device."""
    lib = N.load()
    bufs = [b for b in bufs if b is not None]
    dev = bufs[0].device
    for name, b in zip(NAMES, bufs):
        if not (torch.is_tensor(b) and b.is_cuda and b.dim() == 1 and b.dtype in (torch.float32, torch.float64) and b.is_contiguous()):
            raise TypeError(f"si_ratios_batch: {name}: a contiguous 1-D float32 / float64 CUDA tensor is required")
        if b.device != dev:
            raise ValueError(f"si_ratios_batch: {name} lives on {b.device}, s_hat on {dev}")
    tab = np.asarray(tab, np.int64)
    U = (tab.size - 1) // 5
    if U < 1 or tab.size != 5 * U + 1:
        raise ValueError(f"si_ratios_batch: a table of 5 U + 1 entries is required (got {tab.size})")
    n_items = int(tab[U])
    with torch.cuda.device(dev):
        ratios = torch.empty((U, 3), dtype=torch.float64, device=dev) if want_ratios else None
        sums = torch.empty((U, 8), dtype=torch.float64, device=dev) if want_sums else None
        ws = torch.empty(lib.dvae_si_ratios_workspace_bytes(n_items), dtype=torch.uint8, device=dev)
        tab_dev = H._upload(tab, dev)
        n = bufs[2] if len(bufs) == 3 else None
        f64 = lambda b: 1 if b is not None and b.dtype == torch.float64 else 0
        N.check(lib.dvae_si_ratios_batch(N.ptr(bufs[0]), bufs[0].numel(), f64(bufs[0]), N.ptr(bufs[1]), bufs[1].numel(), f64(bufs[1]),
                                         N.ptr(n), n.numel() if n is not None else 0, f64(n), U, N.ptr(tab_dev), n_items,
                                         N.ptr(ratios), N.ptr(sums), N.ptr(ws), N.stream()), "dvae_si_ratios_batch")
    return ratios, sums


def _score(s_hat, s, n, trim, return_sums):
    args = [_utterances(a, name) for a, name in zip((s_hat, s, n), NAMES) if a is not None]
    # the table is built (and refuses) before anything is uploaded or the library is loaded
    views = [_view(a) for a in args]
    tab = ratio_tables([(o, l) for o, l, _ in views], [t for _, _, t in views], trim)
    dev = _device(args)
    with torch.cuda.device(dev):
        bufs = [_buffer(a, name, dev) for a, name in zip(args, NAMES)]
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

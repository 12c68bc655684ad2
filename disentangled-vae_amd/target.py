"""Device side of the label makers (include/dvae.h: dvae_vad_labels, dvae_ibm_labels) and the fused front end
wav -> (power frames [T,513], labels [T,y_dim]) in the training layout (reference scripts/create_train_set.py:133-194)."""
import numpy as np
import torch

from . import native as N
from . import ragged as R
from . import stft as H


def _dev(t):
    if t.is_cuda:
        return t
    if not torch.cuda.is_available():
        raise RuntimeError("label kernels need the MI355X HIP path (no CPU fallback)")
    return t.cuda()


def vad_labels(y, nfft, hop, frames, vad_threshold=1.70):
    """y: 1-D float32/float64 samples (center padding, if any, already applied; the zero end-pad is implied).  -> (frames) float32."""
    lib = N.load()
    y = _dev(y)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float64)
    y = y.contiguous()
    vad = torch.empty(frames, dtype=torch.float32, device=y.device)
    ws = torch.empty(lib.dvae_vad_workspace_bytes(frames), dtype=torch.uint8, device=y.device)
    N.check(lib.dvae_vad_labels(N.ptr(y), 1 if y.dtype == torch.float64 else 0, y.numel(), nfft, hop, frames, float(vad_threshold),
                                N.ptr(vad), N.ptr(ws), N.stream()), "dvae_vad_labels")
    return vad


def ibm_labels(S, eps=1e-8, ibm_threshold=50, vad_gate=None):
    """S: complex64 (rows, cols).  -> float32 mask of the same shape; vad_gate (cols) multiplies each column."""
    lib = N.load()
    S = _dev(S)
    if S.dtype != torch.complex64:
        raise TypeError(f"ibm_labels: complex64 expected, got {S.dtype}")
    S = S.contiguous()
    rows, cols = S.shape
    mask = torch.empty((rows, cols), dtype=torch.float32, device=S.device)
    ws = torch.empty(lib.dvae_ibm_workspace_bytes(), dtype=torch.uint8, device=S.device)
    gate = None if vad_gate is None else _dev(vad_gate).to(torch.float32).contiguous()
    N.check(lib.dvae_ibm_labels(N.ptr(torch.view_as_real(S)), rows, cols, float(eps), float(ibm_threshold), N.ptr(gate), N.ptr(mask),
                                N.ptr(ws), N.stream()), "dvae_ibm_labels")
    return mask


def utterance_to_frames(speech, labels="vad_labels", fs=16000, wlen_sec=64e-3, hop_percent=0.25, vad_threshold=1.70, eps=1e-8,
                        ibm_threshold=50, device="cuda:0"):
    """One utterance of the training-set builder (scripts/create_train_set.py:133-170) without leaving the GPU:
    speech (float64 samples as soundfile returns them) -> peak-normalise -> STFT (hann, center=False, end-pad rule)
    -> X = |S|^2 as [T, 513] float32 rows, Y = VAD [T, 1] or IBM [T, 513] rows (the layout the train step reads)."""
    lib = N.load()
    speech = np.asarray(speech, dtype=np.float64)
    speech = speech / np.max(np.abs(speech))                              # create_train_set.py:137
    nfft, hop = H.sizes(fs, wlen_sec, hop_percent, "STFT")
    n = len(speech)
    pad = hop if H.needs_end_pad(n, fs, wlen_sec, hop_percent) else 0
    x = torch.from_numpy(speech).to(device)
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    T = H.frame_count(n + pad, nfft, hop)
    w = H.window_f64("hann", nfft, x.device)
    X = H.stft_device(x, w, nfft, hop, T, 1)                              # power frames, training layout
    if labels == "vad_labels":
        Y = vad_labels(x, nfft, hop, T, vad_threshold)[:, None]
    elif labels == "ibm_labels":
        # the mask is elementwise against the global peak: computed on the frame-major complex frames it IS the [T, 513] label rows
        Y = ibm_labels(H.stft_device(x, w, nfft, hop, T, 2), eps, ibm_threshold)
    else:
        raise ValueError(labels)
    return X, Y


# ---------------------------------------------------------------------------------------------------------------------------------
# Ragged batches (dvae_peak_normalise_batch, dvae_vad_labels_batch, dvae_ibm_labels_batch): a whole split of utterances packed end to
# end and labelled in a fixed handful of launches, bit-identical per utterance to the single-signal calls above.  The offset tables
# are checked here before upload (ValueError, as stft_tables), and the kernels check them again against the buffers' extents.

PEAK_CHUNK = 4096          # samples per work item of the peak normalisation
IBM_CHUNK = 4096           # bins per work item of the mask
VAD_ITEMS = 8192           # work items the VAD chunk aims at (one wave each: 8 rounds of 1024 four-wave workgroups)


def peak_tables(x0, lengths, n_total, chunk=PEAK_CHUNK):
    """The int64 table of dvae_peak_normalise_batch, [items (U + 1) | x0 (U) | len (U)]."""
    x0, lengths = R.segments("peak_normalise_batch", x0, lengths, n_total)
    return np.concatenate([R.item_prefix(lengths, chunk), x0, lengths]).astype(np.int64)


def vad_chunk(frames):
    """Frames per VAD work item: about VAD_ITEMS items over the batch, one frame per wave for small batches."""
    return max(1, -(-int(np.sum(frames)) // VAD_ITEMS))


def vad_tables(x0, n, frames, n_total, nfft, hop, chunk):
    """The int64 table of dvae_vad_labels_batch, [items (U + 1) | x0 (U) | n (U) | frame_off (U + 1)]: utterance u's samples are
    x[x0[u] : x0[u] + n[u]] and its frames may reach n[u] + hop (the implied zero end pad of dvae_vad_labels)."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    x0, n = R.segments("vad_labels_batch", x0, n, n_total)
    if frames.size != x0.size:
        raise ValueError("vad_labels_batch: frames need one entry per utterance")
    if np.any(frames < 1):
        raise ValueError(f"vad_labels_batch: every utterance needs at least one frame (frames {frames.tolist()[:16]})")
    if np.any((frames - 1) * hop + nfft > n + hop):
        raise ValueError("vad_labels_batch: frames beyond the end of their signal and its end pad")
    return np.concatenate([R.item_prefix(frames, chunk), x0, n, R.prefix(frames)]).astype(np.int64)


def ibm_tables(e0, count, cols, n_total, chunk=IBM_CHUNK, g0=None, n_gate=0):
    """The int64 table of dvae_ibm_labels_batch, [items (U + 1) | e0 (U) | count (U) | cols (U) | g0 (U)]: segment u is a row-major
    (count / cols, cols) matrix at S[e0[u]:]; with a gate (g0 given), its column j is scaled by gate[g0[u] + j] (n_gate entries)."""
    e0, count = R.segments("ibm_labels_batch", e0, count, n_total)
    cols = np.asarray(cols, np.int64).reshape(-1)
    if cols.size != e0.size or np.any(cols < 1) or np.any(count % cols):
        raise ValueError("ibm_labels_batch: every segment needs a column count that divides its length")
    if g0 is None:
        g0 = np.zeros_like(e0)
    else:
        g0 = np.asarray(g0, np.int64).reshape(-1)
        if g0.size != e0.size or np.any(g0 < 0) or np.any(g0 + cols > n_gate):
            raise ValueError(f"ibm_labels_batch: gate columns outside the gate ({n_gate} entries)")
    return np.concatenate([R.item_prefix(count, chunk), e0, count, cols, g0]).astype(np.int64)


def _vector(t, what, dtypes):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: a torch tensor is required")
    if t.dim() != 1:
        raise ValueError(f"{what}: a 1-D packed buffer is required (got shape {tuple(t.shape)})")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: {' / '.join(str(d) for d in dtypes)} required, got {t.dtype}")


def peak_normalise_batch(x_dev, x0, lengths):
    """x_dev: 1-D float64 CUDA tensor of packed signals, utterance u at x_dev[x0[u] : x0[u] + lengths[u]].  Divides every utterance in
    place by its max |x| (numpy's `speech / np.max(np.abs(speech))` bit for bit; samples outside the utterances are not touched) and
    returns the peaks, float64 [U] on the device (0 for an all-zero utterance, which then holds NaN)."""
    lib = N.load()
    _vector(x_dev, "peak_normalise_batch", (torch.float64,))
    tab = peak_tables(x0, lengths, x_dev.numel())
    if not (x_dev.is_cuda and x_dev.is_contiguous()):
        raise TypeError("peak_normalise_batch: normalises in place: a contiguous CUDA tensor is required")
    U = tab.size // 3
    n_items = int(tab[U])
    peak = torch.empty(U, dtype=torch.float64, device=x_dev.device)
    ws = torch.empty(lib.dvae_peak_normalise_workspace_bytes(n_items), dtype=torch.uint8, device=x_dev.device)
    tab_dev = R.upload(tab, x_dev.device)
    N.check(lib.dvae_peak_normalise_batch(N.ptr(x_dev), x_dev.numel(), U, N.ptr(tab_dev), n_items, PEAK_CHUNK, N.ptr(peak), N.ptr(ws), N.stream()),
            "dvae_peak_normalise_batch")
    return peak


def vad_labels_batch(x_dev, x0, n, frames, nfft, hop, vad_threshold=1.70):
    """vad_labels of every utterance of a packed buffer (x_dev: 1-D float32 / float64; utterance u's samples x_dev[x0[u] : x0[u] + n[u]],
    centre padding, if any, already applied, the zero end pad implied past n[u]; frames[u] frames of nfft samples every hop).  Any
    nfft / hop.  -> float32 [sum frames], utterance u at rows frame_off[u] : frame_off[u + 1], bit-identical to vad_labels on it alone."""
    lib = N.load()
    _vector(x_dev, "vad_labels_batch", (torch.float32, torch.float64))
    frames = np.asarray(frames, np.int64).reshape(-1)
    chunk = vad_chunk(frames)
    tab = vad_tables(x0, n, frames, x_dev.numel(), nfft, hop, chunk)
    x_dev = _dev(x_dev).contiguous()
    U, T_total = frames.size, int(frames.sum())
    n_items = int(tab[U])
    vad = torch.empty(T_total, dtype=torch.float32, device=x_dev.device)
    ws = torch.empty(lib.dvae_vad_batch_workspace_bytes(T_total, n_items), dtype=torch.uint8, device=x_dev.device)
    tab_dev = R.upload(tab, x_dev.device)
    N.check(lib.dvae_vad_labels_batch(N.ptr(x_dev), R.f64_flag(x_dev), x_dev.numel(), int(nfft), int(hop), float(vad_threshold),
                                      U, N.ptr(tab_dev), n_items, chunk, T_total, N.ptr(vad), N.ptr(ws), N.stream()), "dvae_vad_labels_batch")
    return vad


def ibm_labels_batch(S_flat, e0, count, cols, eps=1e-8, ibm_threshold=50, gate=None, g0=None):
    """ibm_labels of every segment of a packed complex64 tensor (any shape, read as its flat contiguous elements): segment u is the
    row-major (count[u] / cols[u], cols[u]) matrix at element e0[u]; gate (float32, 1-D) scales its column j by gate[g0[u] + j].
    -> float32 mask of S_flat's shape, bit-identical per segment to ibm_labels on it alone; elements outside every segment are
    unspecified."""
    lib = N.load()
    if not torch.is_tensor(S_flat) or S_flat.dtype != torch.complex64:
        raise TypeError(f"ibm_labels_batch: complex64 expected, got {getattr(S_flat, 'dtype', type(S_flat))}")
    if gate is not None:
        _vector(gate, "ibm_labels_batch: gate", (torch.float32,))
        if g0 is None:
            raise ValueError("ibm_labels_batch: g0 (each segment's first gate entry) is required with a gate")
    tab = ibm_tables(e0, count, cols, S_flat.numel(), IBM_CHUNK, g0 if gate is not None else None, gate.numel() if gate is not None else 0)
    S = _dev(S_flat).contiguous()
    U = tab.size // 5
    n_items = int(tab[U])
    mask = torch.empty(S.shape, dtype=torch.float32, device=S.device)
    ws = torch.empty(lib.dvae_ibm_batch_workspace_bytes(n_items), dtype=torch.uint8, device=S.device)
    gate = None if gate is None else _dev(gate).contiguous()
    tab_dev = R.upload(tab, S.device)
    N.check(lib.dvae_ibm_labels_batch(N.ptr(torch.view_as_real(S)), S.numel(), float(eps), float(ibm_threshold), U, N.ptr(tab_dev), n_items,
                                      IBM_CHUNK, N.ptr(gate), gate.numel() if gate is not None else 0, N.ptr(mask), N.ptr(ws), N.stream()),
            "dvae_ibm_labels_batch")
    return mask


class FrameBatch:
    """The training rows of a batch of utterances, as utterances_to_frames returns them: X [sum T_u, 513] float32 power frames and Y
    [sum T_u, y_dim] float32 labels on the device, utterance u at rows frame_off[u] : frame_off[u + 1]; counts: T_u."""

    def __init__(self, X, Y, counts):
        self.X, self.Y = X, Y
        self.counts = [int(c) for c in counts]
        self.frame_off = R.prefix(self.counts)

    def __len__(self):
        return len(self.counts)

    def frames(self, u):
        """(X_u [T_u, 513], Y_u [T_u, y_dim]) device views: what utterance_to_frames returns for utterance u."""
        a, b = int(self.frame_off[u]), int(self.frame_off[u + 1])
        return self.X[a:b], self.Y[a:b]


_PACK_THREADS = 8


def _pack(buf, signals, x0, padded):
    """buf[x0[u] : x0[u] + padded[u]] = signal u followed by zeros.  The copy is bound by host memory bandwidth (a split of 5 s
    utterances is GBs), so it runs on a few threads (numpy releases the GIL for the copies)."""
    def part(us):
        for u in us:
            a, n = int(x0[u]), len(signals[u])
            buf[a:a + n] = signals[u]
            buf[a + n:a + int(padded[u])] = 0.0
    U = len(signals)
    k = min(_PACK_THREADS, U, 1 + int(np.sum(padded)) // (1 << 20))
    if k <= 1:
        return part(range(U))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(k) as ex:
        list(ex.map(part, [range(i, U, k) for i in range(k)]))


def utterances_to_frames(speeches, labels="vad_labels", fs=16000, wlen_sec=64e-3, hop_percent=0.25, vad_threshold=1.70, eps=1e-8,
                         ibm_threshold=50, device="cuda:0"):
    """utterance_to_frames of every utterance in a fixed handful of launches: the raw signals (float64 samples) and their end pads are
    packed on the host and copied to the device once, then peak normalisation, the power STFT, and the VAD on the same buffer or the
    complex STFT and the mask over its frames.  -> FrameBatch whose frames(u) are bit-identical to utterance_to_frames(speeches[u], ...).
    nfft 1024 / hop 256 only (what the batch STFT covers).  ValueError naming the utterance for one whose samples are all zero (the
    reference divides by zero there)."""
    if labels not in ("vad_labels", "ibm_labels"):
        raise ValueError(f"utterances_to_frames: unknown label kind {labels!r} (vad_labels or ibm_labels)")
    nfft, hop = H.sizes(fs, wlen_sec, hop_percent, "STFT")
    if not H.batch_covers(nfft, hop):
        raise ValueError(f"utterances_to_frames: nfft {nfft} / hop {hop}: the batch transform covers nfft 1024 / hop 256; use utterance_to_frames")
    sp = [np.asarray(s, dtype=np.float64) for s in speeches]
    if not sp:
        raise ValueError("utterances_to_frames: no utterances")
    for u, s in enumerate(sp):
        if s.ndim != 1:
            raise ValueError(f"utterances_to_frames: utterance {u} is not 1-D (shape {s.shape})")
    lengths = [len(s) for s in sp]
    plan = H.plan_stft_batch(lengths, fs, wlen_sec, hop_percent, center=False, pad_at_end=True)
    x0, padded, frames = plan["x0"], plan["padded"], plan["frames"]
    dev = torch.device(device)
    with torch.cuda.device(dev):
        host = torch.empty(int(padded.sum()), dtype=torch.float64, pin_memory=True)
        _pack(host.numpy(), sp, x0, padded)
        x = host.to(dev, non_blocking=True)
        peak = peak_normalise_batch(x, x0, lengths)
        X = H.stft_packed(x, frames, x0, padded, lengths, False, 1).frames
        if labels == "vad_labels":
            Y = vad_labels_batch(x, x0, padded, frames, nfft, hop, vad_threshold)[:, None]
        else:
            S = H.stft_packed(x, frames, x0, padded, lengths, False, 2).frames
            Y = ibm_labels_batch(S, plan["frame_off"][:-1] * S.shape[1], frames * S.shape[1], np.full(len(sp), S.shape[1]), eps, ibm_threshold)
        zero = np.flatnonzero(peak.cpu().numpy() == 0)
    if zero.size:
        raise ValueError(f"utterances_to_frames: utterance {int(zero[0])} is all zeros (peak normalisation divides by zero)"
                         + (f"; {zero.size - 1} more" if zero.size > 1 else ""))
    return FrameBatch(X, Y, frames)

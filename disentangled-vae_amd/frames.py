"""GPU-resident frame store: the MI355X-native replacement of the reference's training input pipeline.

The reference reads ONE 513-float column per __getitem__ from an lzf-compressed HDF5 file through 16
DataLoader workers (packages/data_handling.py:45-60, scripts/training_M2.py:77-89).  The fused train
step consumes >100 M frames/s; a whole training set of spectrogram frames (2 KB each) fits the 288 GB
of HBM many times over, so the set is loaded once, kept frames-major ([N][513], the layout the train
step reads), and every epoch is ONE row gather into a second buffer (a random permutation, what
DataLoader(shuffle=True) produces) after which batches are contiguous views: no per-step copy at all.
"""
import numpy as np
import torch

from . import native as N

F_BINS = 513


def _to_device_rows(a, device, chunk=1 << 18):
    """(F, n) host/device matrix, one frame per column (on-disk orientation) -> [n][F] float32 device rows."""
    lib = N.load()
    rows, n = a.shape
    out = torch.empty((n, rows), dtype=torch.float32, device=device)
    for c0 in range(0, n, chunk):               # bounded staging: the file may be larger than pinned host memory
        c1 = min(n, c0 + chunk)
        blk = a[:, c0:c1]
        blk = torch.from_numpy(np.ascontiguousarray(blk, dtype=np.float32)) if not torch.is_tensor(blk) else blk.to(torch.float32)
        blk = blk.to(device).contiguous()
        N.check(lib.dvae_transpose(N.ptr(blk), rows, c1 - c0, c1 - c0, N.ptr(out[c0:c1]), rows, N.stream()), "dvae_transpose")
    return out


def frame_stats(X, rows=None, bad=None):
    """Per-bin (mean, std) of the frames of X, float32 device tensors [513]: the X_train_mean / X_train_std of the reference's
    create_train_set.py, formed on the device in two launches (include/dvae.h: dvae_frame_stats -- the formula in double, the
    order of summation fixed, std 0 and not NaN for a constant bin).  X: float32 CUDA rows [N, >= 513 by stride] (DeviceFrames.x, a
    FrameBatch's X).  rows: an int64 CUDA index tensor (a train split of a larger store); an index outside the store is counted in
    `bad` (an int32 CUDA tensor of one element, optional) and left out.  Fewer than two frames: ValueError."""
    if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] >= F_BINS and X.shape[0] >= 1
            and X.stride(1) == 1 and (X.shape[0] == 1 or X.stride(0) >= F_BINS)):
        raise TypeError(f"frame_stats: X must be float32 CUDA rows [N, {F_BINS}] (row stride >= {F_BINS})")
    if rows is not None and not (torch.is_tensor(rows) and rows.device == X.device and rows.dtype == torch.int64 and rows.dim() == 1
                                 and rows.is_contiguous()):
        raise TypeError(f"frame_stats: rows must be a contiguous int64 tensor [n] on {X.device}")
    if bad is not None and not (torch.is_tensor(bad) and bad.device == X.device and bad.dtype == torch.int32 and bad.numel() == 1):
        raise TypeError(f"frame_stats: bad must be an int32 tensor of one element on {X.device}")
    n = X.shape[0] if rows is None else rows.numel()
    if n < 2:
        raise ValueError(f"frame_stats: {n} frames (the standard deviation divides by n - 1: at least 2)")
    lib = N.load()
    with torch.cuda.device(X.device):
        ws = torch.empty(lib.dvae_frame_stats_workspace_bytes(n) // 8, dtype=torch.float64, device=X.device)
        out = torch.empty((2, F_BINS), dtype=torch.float32, device=X.device)
        N.check(lib.dvae_frame_stats(N.ptr(X), N.ld(X), X.shape[0], N.ptr(rows), 0 if rows is None else n, N.ptr(out[0]), N.ptr(out[1]),
                                     N.ptr(bad), N.ptr(ws), N.stream()), "dvae_frame_stats")
    return out[0], out[1]


class DeviceFrames:
    """Frames X [N][513] and labels Y [N][y_dim] resident in HBM.

    X, Y: arrays / tensors / h5py datasets in the on-disk orientation (513, N), (y_dim, N); Y may be None (M1).
    """

    def __init__(self, X, Y=None, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceFrames needs the MI355X HIP path (no CPU fallback)")
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.x = _to_device_rows(X, self.device)
            self.y = _to_device_rows(Y, self.device) if Y is not None else None
        if self.y is not None and self.y.shape[0] != self.x.shape[0]:
            raise ValueError("X and Y hold different numbers of frames")
        self._xs = self._ys = None
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    @classmethod
    def from_rows(cls, X, Y=None):
        """Adopt frames already in the training layout: X [N][513], Y [N][y_dim] (or None) float32 device rows, e.g. a FrameBatch's
        (target.utterances_to_frames).  No transpose and no copy for contiguous rows."""
        for name, t in (("X", X), ("Y", Y)):
            if t is None:
                continue
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
                raise TypeError(f"DeviceFrames.from_rows: {name} must be a 2-D float32 CUDA tensor of rows")
        if X.shape[1] != F_BINS:
            raise ValueError(f"DeviceFrames.from_rows: X rows of {F_BINS} bins expected, got {X.shape[1]}")
        if Y is not None and (Y.shape[0] != X.shape[0] or Y.device != X.device):
            raise ValueError("X and Y hold different numbers of frames")
        self = cls.__new__(cls)
        self.device = X.device
        self.x = X.contiguous()
        self.y = Y.contiguous() if Y is not None else None
        self._xs = self._ys = None
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self

    @classmethod
    def from_hdf5(cls, path, split, device="cuda:0"):
        """The reference's training file (scripts/create_train_set.py:91-219): datasets X_<split>, Y_<split>."""
        import h5py
        with h5py.File(path, "r") as f:
            return cls(f["X_" + split], f["Y_" + split] if ("Y_" + split) in f else None, device)

    def __len__(self):
        return self.x.shape[0]

    def _gather(self, src, idx, dst):
        lib = N.load()
        N.check(lib.dvae_gather_rows(N.ptr(src), src.stride(0), src.shape[0], N.ptr(idx), idx.numel(), src.shape[1], N.ptr(dst),
                                     dst.stride(0), N.ptr(self._bad), N.stream()), "dvae_gather_rows")

    def stats(self, rows=None):
        """(mean, std) per bin over the store, or over its rows `rows` (int64 device indices: the train split), as frame_stats; an
        index outside the store goes to bad_row_count()."""
        return frame_stats(self.x, rows, self._bad)

    def bad_row_count(self):
        """Indices outside the store that stats() and the epoch gathers skipped since the last call (synchronises)."""
        n = int(self._bad.item())
        if n:
            self._bad.zero_()
        return n

    def shuffled(self, generator=None):
        """One epoch's order: returns (x, y) permuted copies (buffers are reused from epoch to epoch)."""
        n = len(self)
        with torch.cuda.device(self.device):
            perm = torch.randperm(n, device=self.device, generator=generator)
            if self._xs is None:
                self._xs = torch.empty_like(self.x)
                self._ys = torch.empty_like(self.y) if self.y is not None else None
            self._gather(self.x, perm, self._xs)
            if self.y is not None:
                self._gather(self.y, perm, self._ys)
        self.last_perm = perm
        return self._xs, self._ys

    def index_batches(self, batch, shuffle=True, drop_last=False, generator=None):
        """Yields int64 row-index tensors [b] for `Trainer.step(data.x, data.y, rows=idx)`: the rows kernel gathers the
        frames itself (2 KB contiguous per frame), so an epoch's shuffle costs one randperm instead of a copy of the set."""
        n = len(self)
        with torch.cuda.device(self.device):
            order = torch.randperm(n, device=self.device, generator=generator) if shuffle else torch.arange(n, device=self.device)
        self.last_perm = order
        for s in range(0, n, batch):
            e = min(n, s + batch)
            if e - s < batch and drop_last:
                return
            yield order[s:e]

    def batches(self, batch, shuffle=True, drop_last=False, generator=None):
        """Yields (x [b,513], y [b,y_dim] or None) contiguous device views, b == batch except possibly the last."""
        x, y = self.shuffled(generator) if shuffle else (self.x, self.y)
        n = len(self)
        for s in range(0, n, batch):
            e = min(n, s + batch)
            if e - s < batch and drop_last:
                return
            yield x[s:e], (y[s:e] if y is not None else None)

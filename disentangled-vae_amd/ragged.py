"""Host side of ragged batches: many utterances of different lengths packed end to end in one buffer, the layout of every batch op
here (stft.py, target.py, metrics.py, mix.py).  An op checks its per-utterance offset tables on the host and refuses, naming the
utterance; packs its inputs into one pinned buffer and uploads it once; and uploads a prefix table of work items from which each
wave finds its utterance (csrc/ragged.hpp).  What the ops share of that lives here; importing and testing it needs no GPU.
"""
import numpy as np
import torch

UTTERANCE = ("utterance", "utterances")        # what an op calls the members of a list, singular and plural, in its messages
ENTRY = ("entry", "entries")


class WaveBatch:
    """A ragged batch of waveforms on the device: y float32, utterance u is y[offsets[u] : offsets[u] + lengths[u]] (offsets are
    multiples of 64 samples; what lies between two utterances is unspecified)."""

    def __init__(self, y, offsets, lengths):
        self.y, self.offsets, self.lengths = y, [int(o) for o in offsets], [int(n) for n in lengths]

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, u):
        return self.y[self.offsets[u]:self.offsets[u] + self.lengths[u]]

    def numpy(self):
        h = self.y.cpu().numpy()
        return [h[o:o + n] for o, n in zip(self.offsets, self.lengths)]


# ---- tables ------------------------------------------------------------------------------------------------------------------------------

def prefix(counts):
    """int64 [len + 1]: 0 and the running sums of counts."""
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def item_prefix(extents, chunk):
    """The work-item prefix table [U + 1] that batch_item (csrc/ragged.hpp) searches: utterance u has ceil(extents[u] / chunk) items."""
    return prefix(-(-np.asarray(extents, np.int64) // chunk))


def monotone(name, a):
    a = np.asarray(a, np.int64)
    if a.size > 1 and np.any(np.diff(a) < 0):
        raise ValueError(f"{name} must be non-decreasing: {a.tolist()[:16]}")


def segments(what, start, extent, n_total):
    """start / extent: one int64 entry per utterance; refuses empty, overlapping or out-of-buffer segments."""
    start, extent = np.asarray(start, np.int64).reshape(-1), np.asarray(extent, np.int64).reshape(-1)
    if start.size == 0 or extent.size != start.size:
        raise ValueError(f"{what}: the tables need one entry per utterance (got {start.size} offsets, {extent.size} extents)")
    if np.any(extent < 1):
        raise ValueError(f"{what}: every utterance needs at least one element (extents {extent.tolist()[:16]})")
    monotone(f"{what}: offsets", start)
    if start[0] < 0 or np.any(start[:-1] + extent[:-1] > start[1:]) or start[-1] + extent[-1] > n_total:
        raise ValueError(f"{what}: utterances overlap or leave the packed buffer ({n_total} elements)")
    return start, extent


def paired_views(op, names, views, totals, trim):
    """The views of one set of utterances inside several packed buffers (names[k]: (offsets, lengths) in a buffer of totals[k]
    elements), with trim samples dropped at both ends of every utterance -> (the trimmed offsets per buffer, the trimmed lengths, U).
    ValueError naming the utterance for lengths that differ between the buffers, for an utterance not longer than 2 * trim and for
    one outside its buffer."""
    trim = int(trim)
    if trim < 0:
        raise ValueError(f"{op}: trim must not be negative (got {trim})")
    offs = [np.asarray(o, np.int64).reshape(-1) for o, _ in views]
    lens = [np.asarray(n, np.int64).reshape(-1) for _, n in views]
    U = offs[0].size
    if U == 0:
        raise ValueError(f"{op}: no utterances")
    for name, o, n in zip(names, offs, lens):
        if o.size != U or n.size != U:
            raise ValueError(f"{op}: {name} holds {max(o.size, n.size)} utterances, {names[0]} {U}")
    for name, n in zip(names[1:], lens[1:]):
        bad = np.flatnonzero(n != lens[0])
        if bad.size:
            u = int(bad[0])
            raise ValueError(f"{op}: utterance {u}: {names[0]} has {int(lens[0][u])} samples, {name} {int(n[u])}")
    short = np.flatnonzero(lens[0] <= 2 * trim)
    if short.size:
        u = int(short[0])
        raise ValueError(f"{op}: utterance {u} has {int(lens[0][u])} samples: "
                         + (f"not longer than 2 * trim = {2 * trim}" if trim else "at least one is needed"))
    for name, o, total in zip(names, offs, totals):
        bad = np.flatnonzero((o < 0) | (o + lens[0] > int(total)))
        if bad.size:
            u = int(bad[0])
            raise ValueError(f"{op}: utterance {u} of {name} ([{int(o[u])}, {int(o[u] + lens[0][u])})) leaves its buffer ({int(total)} elements)")
    return [o + trim for o in offs], lens[0] - 2 * trim, U


# ---- the device ---------------------------------------------------------------------------------------------------------------------------

def device():
    if not torch.cuda.is_available():
        raise RuntimeError("STFT/ISTFT run on the MI355X HIP path only: no GPU is visible (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def find_device(*groups):
    """The device of the first CUDA tensor among the groups (WaveBatches or lists), else the current one."""
    for g in groups:
        for a in ([g.y] if isinstance(g, WaveBatch) else g):
            if torch.is_tensor(a) and a.is_cuda:
                return a.device
    return device()


def upload(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def check_packed(op, named):
    """named: (name, buffer) pairs of one call.  Every buffer a contiguous 1-D float32 / float64 CUDA tensor, all on the first one's device."""
    first, dev = named[0][0], named[0][1].device
    for name, b in named:
        if not (torch.is_tensor(b) and b.is_cuda and b.dim() == 1 and b.dtype in (torch.float32, torch.float64) and b.is_contiguous()):
            raise TypeError(f"{op}: {name}: a contiguous 1-D float32 / float64 CUDA tensor is required")
        if b.device != dev:
            raise ValueError(f"{op}: {name} lives on {b.device}, {first} on {dev}")
    return dev


def f64_flag(b):
    """The `*_f64` argument of the C ABI for the buffer b (0 for an absent one)."""
    return 1 if b is not None and b.dtype == torch.float64 else 0


# ---- packing ------------------------------------------------------------------------------------------------------------------------------

def as_list(x, what, noun=UTTERANCE, empty="no utterances", floating=False):
    """A WaveBatch as it is; anything else as a list of 1-D arrays / tensors (one array or tensor: a list of one).  what: "<op>: <name>",
    the head of every message.  floating: refuse an entry that is not floating point here, before anything else is looked at."""
    if isinstance(x, WaveBatch):
        y = x.y
        if not (torch.is_tensor(y) and y.is_cuda and y.dim() == 1 and y.dtype in (torch.float32, torch.float64)):
            raise TypeError(f"{what}: a WaveBatch over a 1-D float32 / float64 CUDA tensor is required")
        return x
    x = [x] if torch.is_tensor(x) or isinstance(x, np.ndarray) else list(x)
    if not x:
        raise ValueError(f"{what}: {empty}")
    for u, a in enumerate(x):
        if getattr(a, "ndim", None) != 1:
            raise ValueError(f"{what}: {noun[0]} {u} is not a 1-D array or tensor")
        if floating and not (a.dtype.is_floating_point if torch.is_tensor(a) else np.issubdtype(a.dtype, np.floating)):
            raise TypeError(f"{what}: {noun[0]} {u} is not floating point ({a.dtype})")
    return x


def view(x, dedupe=False):
    """(offsets, lengths, element count) of the packed buffer that pack makes of x, offsets and lengths int64 arrays.  dedupe: an
    array given several times is packed once."""
    if isinstance(x, WaveBatch):
        return np.asarray(x.offsets, np.int64), np.asarray(x.lengths, np.int64), x.y.numel()
    seen, offs, total = {}, [], 0
    for u, a in enumerate(x):
        key = id(a) if dedupe else u
        if key not in seen:
            seen[key] = total
            total += int(a.shape[0])
        offs.append(seen[key])
    return np.asarray(offs, np.int64), np.asarray([int(a.shape[0]) for a in x], np.int64), total


def pack(x, what, dev, noun=UTTERANCE, dedupe=False):
    """The packed 1-D float32 / float64 CUDA tensor of x, in the order of view: a WaveBatch's own, one device tensor adopted as it is,
    several concatenated, host arrays packed into one pinned buffer and uploaded once."""
    if isinstance(x, WaveBatch):
        return x.y.contiguous()
    uniq = list({(id(a) if dedupe else u): a for u, a in enumerate(x)}.values())
    on_dev = [torch.is_tensor(a) and a.is_cuda for a in uniq]
    if all(on_dev):
        dt = torch.float32 if all(a.dtype == torch.float32 for a in uniq) else torch.float64
        if len(uniq) == 1 and uniq[0].dtype == dt:
            return uniq[0].contiguous()
        return torch.cat([a.to(dt) for a in uniq]).contiguous()
    if any(on_dev):
        raise TypeError(f"{what} mixes host and device {noun[1]}")
    xs = [a.detach().numpy() if torch.is_tensor(a) else np.asarray(a) for a in uniq]
    for u, a in enumerate(xs):
        if not np.issubdtype(a.dtype, np.floating):
            raise TypeError(f"{what}: {noun[0]} {u} is not floating point ({a.dtype})")
    # float32 samples convert to double exactly, and the kernels compute in double whatever they read: one buffer type serves all
    dt = torch.float32 if all(a.dtype == np.float32 for a in xs) else torch.float64
    host = torch.empty(sum(len(a) for a in xs), dtype=dt, pin_memory=True)
    h, o = host.numpy(), 0
    for a in xs:
        h[o:o + len(a)] = a
        o += len(a)
    return host.to(dev, non_blocking=True)

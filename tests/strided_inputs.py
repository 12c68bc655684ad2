"""Row-strided and offset views of a packed [n, w] float32 array, for the train steps' x and y (tests/test_strided_inputs_cpu.py shows
what each layout promises and which wrong read it exposes; tests/test_gpu_train_strided.py steps the four trainers on them).  torch and
numpy only, no GPU needed to import.

Every layout is a view with the packed array's values into a backing buffer that is NaN everywhere else, ends in one more NaN row, and
allocates every row to its full leading dimension -- so a read through the wrong stride or from the wrong base lands on a NaN or on
another element, never outside the allocation.

    packed    [n + 1, w][:n]                          ld w, offset 0: the control
    ld+7      [n + 1, w + 7][:n, :w]                  ld 520 for w 513: every row 16-byte aligned, ld != w
    odd       [n + 1, w + 6][:n, 3:3 + w]             offset 3, ld 519 for w 513: the rows run through all four alignments mod 16
    shifted   flat[1 + (n + 1) w] from element 1      ld == w, the base 4 bytes past a 16-byte boundary
    column    [n + 1, 513][:n, k:k + w]  (labels)     one label (k 7) or 3 / 17 labels (k 2) out of a 513-wide label store
"""
import numpy as np
import torch

X_LAYOUTS = ("ld+7", "odd", "shifted")              # the strided layouts of x, and of y at any width
COLUMN_WIDTHS = {1: 7, 3: 2, 17: 2}                  # label widths the `column` layout exists for -> first column k
STORE_WIDTH = 513                                    # the label store `column` slices
EXTRA_ROWS = 37                                      # a rows= store holds this many frames more than the batch gathers


def names(w, kind="x"):
    """The layouts of a width-w array: kind "x" or "y" (labels: `column` too where w is 1, 3 or 17)."""
    return ("packed",) + X_LAYOUTS + (("column",) if kind == "y" and w in COLUMN_WIDTHS else ())


def geometry(name, n, w):
    """(backing shape, row stride ld, storage offset) of a layout."""
    if name == "packed":
        return (n + 1, w), w, 0
    if name == "ld+7":
        return (n + 1, w + 7), w + 7, 0
    if name == "odd":
        return (n + 1, w + 6), w + 6, 3
    if name == "shifted":
        return (1 + (n + 1) * w,), w, 1
    if name == "column":
        return (n + 1, STORE_WIDTH), STORE_WIDTH, COLUMN_WIDTHS[w]
    raise ValueError(name)


def layout(a, name):
    """The view of layout `name` with a's values (a: packed float32 [n, w]); backing(view) is its whole buffer."""
    a = np.array(a, dtype=np.float32)                    # (a copy: the shared inputs of the cases modules are read-only)
    n, w = a.shape
    shape, ld, off = geometry(name, n, w)
    buf = torch.full(shape, float("nan"), dtype=torch.float32)
    view = buf.reshape(-1).as_strided((n, w), (ld, 1), off)
    view.copy_(torch.from_numpy(a))
    return view


def layouts(a, kind="x"):
    """{name: view} of every layout a [n, w] array of `kind` has."""
    return {name: layout(a, name) for name in names(np.shape(a)[1], kind)}


def backing(view):
    """The whole storage of a view as a flat tensor (the NaN padding included)."""
    return torch.as_strided(view, (view.untyped_storage().nbytes() // view.element_size(),), (1,), 0)


def on_device(view, device):
    """The backing buffer moved to `device` and viewed again: same shape, strides and storage offset."""
    return backing(view).to(device).as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def gather_rows(n, B, seed=3):
    """The fixed permutation of a rows= case: B distinct rows of a store of n, int64."""
    return np.random.default_rng(seed).permutation(n)[:B].astype(np.int64)


def gather_stores(pool, B, kind="x", seed=3):
    """({name: view of pool[:B + EXTRA_ROWS]}, rows): the rows= stores of a batch of B in every layout, and the permutation
    that gathers it."""
    n = B + EXTRA_ROWS
    assert pool.shape[0] >= n, (pool.shape, n)
    return layouts(pool[:n], kind), gather_rows(n, B, seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatements of a read site (tests/test_strided_inputs_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------

def read(flat, n, w, ld, off):
    """What a kernel loads for element (r, c): flat[off + r ld + c]."""
    r, c = np.arange(n)[:, None], np.arange(w)[None, :]
    return np.asarray(flat)[off + r * ld + c]


def read_right(view):
    return read(backing(view).numpy(), view.shape[0], view.shape[1], view.stride(0), view.storage_offset())


def read_width_for_stride(view):
    """One read site that uses the width in place of the leading dimension."""
    return read(backing(view).numpy(), view.shape[0], view.shape[1], view.shape[1], view.storage_offset())


def read_without_offset(view):
    """A reader handed the allocation's base instead of the view's first element."""
    return read(backing(view).numpy(), view.shape[0], view.shape[1], view.stride(0), 0)

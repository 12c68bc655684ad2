"""tests/strided_inputs.py on the CPU: what every layout promises (strides, storage offset, alignment of the first element, the packed
array's bits, NaN everywhere else, a spare NaN row) and which wrong read it exposes.

Sharpness.  Two numpy restatements of a faulty read site, on the very buffers the GPU tests hand to the trainers:
  width for stride   element (r, c) read at base + r w + c in place of base + r ld + c
  base for offset    element (r, c) read from the allocation's first element in place of the view's
Each non-packed layout returns a NaN or another element's value under at least one of them, at every n >= 2:
  ld+7     width for stride only  (its offset is 0)
  odd      both
  shifted  base for offset only   (ld == w: it is there for the alignment of the base, which no stride can show)
  column   both
and the right reader returns the packed array bit for bit on all of them.  At n == 1 no stride is ever used; there only the offset
shows (odd, shifted, column).
"""
import numpy as np
import pytest
import torch

import strided_inputs as S

SHAPES = [(1, 513), (2, 513), (50, 513), (87, 513), (50, 1), (50, 3), (50, 17), (50, 2), (2, 1), (1, 1)]
CATCHES = {"ld+7": (True, False), "odd": (True, True), "shifted": (False, True), "column": (True, True)}      # (width for stride, base for offset)


def _array(n, w):
    a = np.random.default_rng(100 * n + w).standard_normal((n, w)).astype(np.float32)
    a[0, 0] = -0.0                                                          # a sign bit a value comparison would miss
    return a


def _cases():
    return [(n, w, kind, name) for n, w in SHAPES for kind in ("x", "y") for name in S.names(w, kind)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n,w,kind,name", _cases())
def test_layout_keeps_its_promises(n, w, kind, name):
    a = _array(n, w)
    v = S.layouts(a, kind)[name]
    shape, ld, off = S.geometry(name, n, w)
    assert tuple(v.shape) == (n, w) and v.dtype == torch.float32
    assert v.stride() == (ld, 1) and v.storage_offset() == off
    buf = S.backing(v)
    assert buf.numel() == int(np.prod(shape)) and buf.data_ptr() % 16 == 0
    assert v.data_ptr() % 16 == (4 * off) % 16
    want = {"packed": (w, 0, 0), "ld+7": (w + 7, 0, 0), "odd": (w + 6, 3, 12), "shifted": (w, 1, 4),
            "column": (513, S.COLUMN_WIDTHS.get(w, 0), 4 * S.COLUMN_WIDTHS.get(w, 0) % 16)}[name]
    assert (v.stride(0), v.storage_offset(), v.data_ptr() % 16) == want
    if w == 513:
        assert (ld == 513 and v.data_ptr() % 16 == 0) == (name == "packed")          # only the control meets the whole-tile condition
    # the packed array bit for bit, NaN everywhere else, every row allocated to its ld, one spare row
    assert np.array_equal(_bits(v.numpy()), _bits(a))
    inside = np.zeros(buf.numel(), bool)
    inside[off + np.arange(n)[:, None] * ld + np.arange(w)[None, :]] = True
    flat = buf.numpy()
    assert np.all(np.isnan(flat[~inside])) and np.array_equal(_bits(flat[inside]), _bits(a).ravel())
    assert buf.numel() == (n + 1) * ld + (1 if name == "shifted" else 0)
    assert buf.numel() - (off + (n - 1) * ld + w) >= w                            # at least one more row's worth of NaN behind the last element
    # moved as a whole and viewed again: the same view
    moved = S.on_device(v, "cpu")
    assert moved.stride() == v.stride() and moved.storage_offset() == off and np.array_equal(_bits(moved.numpy()), _bits(a))
    assert np.array_equal(_bits(v.contiguous().numpy()), _bits(a))
    assert n == 1 or v.contiguous().stride() == (w, 1)                            # (one row is contiguous at any stride: no copy is made)


@pytest.mark.parametrize("n,w,kind,name", [c for c in _cases() if c[3] != "packed"])
def test_a_wrong_read_site_shows_on_every_strided_layout(n, w, kind, name):
    """The right reader returns the array; a reader with the width for the stride, or the base for the offset, does not -- in the
    combinations the module docstring lists.  `shifted` is ld == w: it catches the second variant only."""
    a = _array(n, w)
    v = S.layouts(a, kind)[name]
    assert np.array_equal(_bits(S.read_right(v)), _bits(a))
    by_width, by_base = S.read_width_for_stride(v), S.read_without_offset(v)
    wrong_rows = lambda got: int(np.sum(np.any(_bits(got) != _bits(a), axis=1)))
    catches_width, catches_base = CATCHES[name]
    if n >= 2:
        assert (wrong_rows(by_width) >= 1) == catches_width, (name, wrong_rows(by_width))
        if catches_width:
            assert wrong_rows(by_width) >= n - 1                                 # every row but the first
    else:
        assert wrong_rows(by_width) == 0                                         # one row: no stride is used
    assert (wrong_rows(by_base) >= 1) == catches_base, (name, wrong_rows(by_base))
    if n >= 2:
        assert catches_width or catches_base
    if name == "shifted":
        assert v.stride(0) == w and wrong_rows(by_width) == 0 and wrong_rows(by_base) == n


def test_the_packed_control_is_blind_to_both():
    a = _array(50, 513)
    v = S.layouts(a)["packed"]
    assert np.array_equal(_bits(S.read_width_for_stride(v)), _bits(a)) and np.array_equal(_bits(S.read_without_offset(v)), _bits(a))


def test_gather_stores():
    B = 50
    pool = _array(B + S.EXTRA_ROWS + 5, 513)
    stores, rows = S.gather_stores(pool, B)
    assert rows.dtype == np.int64 and rows.shape == (B,) and len(set(rows.tolist())) == B and rows.max() < B + S.EXTRA_ROWS
    assert np.array_equal(rows, S.gather_rows(B + S.EXTRA_ROWS, B)) and not np.array_equal(rows, np.arange(B))
    for name, v in stores.items():
        assert tuple(v.shape) == (B + S.EXTRA_ROWS, 513) and v.stride(0) == S.geometry(name, B + S.EXTRA_ROWS, 513)[1]
        assert np.array_equal(_bits(v[torch.from_numpy(rows)].numpy()), _bits(pool[rows]))
    labels, _ = S.gather_stores(_array(B + S.EXTRA_ROWS, 1), B, "y")
    assert set(labels) == {"packed", "ld+7", "odd", "shifted", "column"} and labels["column"].stride() == (513, 1)

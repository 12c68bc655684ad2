"""Float64 restatement of the reparametrisation noise the rows kernels draw themselves (csrc/rows_common.hpp:
philox_normal4 / frame_noise8, Trainer.noise()).  numpy only, no GPU.

Contract (the device code and this file state it once each):

  block    Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
  key      (seed lo, seed hi)                                   -- the trainer's 64-bit seed, see rank_seed()
  counter  (frame lo, frame hi, step lo, (step hi << 8) | draw) -- frame = position in the batch, step < 2^56, draw 0 .. 3
  uniform  u = (float32(w >> 8) + 0.5f) * 2^-24 IN FLOAT32      -- 24 bits per word; the sum rounds to even from 2^23 on, so
                                                                   u lies in [2^-25, 1] and w >> 8 = 2^24 - 1 gives exactly 1
  normals  r = sqrt(-2 ln u0), t = 2 pi u1 -> (r cos t, r sin t); the same from (u2, u3): four per block
  layout   draw 0 -> latent features 0 .. 3, draw 1 -> 8 .. 11, draw 2 -> 4 .. 7, draw 3 -> 12 .. 15
  steps    training step n (1-based) uses step = n; the k-th evaluate() without a noise tensor uses step = 2^40 + k
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)
EVAL_BASE = 1 << 40
RANK_STRIDE = 0x9E3779B97F4A7C15
# latent features of draw d (four consecutive ones)
DRAW_FEATURE0 = (0, 8, 4, 12)


def _u64(a):
    """Python ints up to 2^64 - 1 / integer arrays -> uint64 array."""
    if isinstance(a, np.ndarray):
        return a.astype(np.uint64)
    if isinstance(a, (list, tuple, range)):
        return np.array([int(v) for v in a], dtype=np.uint64)
    return np.array(int(a), dtype=np.uint64)


def philox4x32_10(counter4, key2):
    """counter4 = four, key2 = two uint64 arrays holding 32-bit words (broadcast against each other) -> four output words."""
    c0, c1, c2, c3 = [_u64(c) & M32 for c in counter4]
    k0, k1 = [_u64(k) & M32 for k in key2]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def eval_step(k):
    """Counter step of the k-th (1-based) evaluate() that draws its own noise: a range no training step reaches."""
    return EVAL_BASE + int(k)


def rank_seed(base, rank):
    """The key of rank `rank` of a data-parallel run started with the common seed `base` (trainer.py)."""
    return (int(base) + int(rank) * RANK_STRIDE) & 0xFFFFFFFFFFFFFFFF


def counter(frames, step, draw):
    """The four counter words of (frame, step, draw); each argument a Python int or an integer array."""
    f, s, d = _u64(frames), _u64(step), _u64(draw)
    return f & M32, f >> S32, s & M32, (((s >> S32) << np.uint64(8)) | d) & M32


def key(seed):
    s = _u64(seed)
    return s & M32, s >> S32


def words(seed, frames, step, draw):
    """Philox output words of (seed, frame, step, draw), stacked on a last axis of four."""
    return np.stack(np.broadcast_arrays(*philox4x32_10(counter(frames, step, draw), key(seed))), axis=-1)


def uniforms(w):
    """The kernel's input quantisation, in float32 arithmetic like the kernel's: 24 bits of the word, centred.  From w >> 8 = 2^23 on the
    sum is not representable and rounds to even, so the result lies in [2^-25, 1] -- 1.0 included (w >> 8 = 2^24 - 1)."""
    k = (_u64(w) >> np.uint64(8)).astype(np.float32)              # < 2^24: exact
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(u):
    """u [..., 4] float32 uniforms of one block -> [..., 4] float64 normals (r_a cos, r_a sin, r_b cos, r_b sin)."""
    u = np.asarray(u).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    ta, tb = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=-1)


def normals(seed, frames, step):
    """float64 [len(frames), 16]: the noise of the given batch positions at counter step `step` under key `seed`."""
    frames = _u64(frames).reshape(-1)
    out = np.empty((frames.shape[0], 16), np.float64)
    for draw in range(4):
        f0 = DRAW_FEATURE0[draw]
        out[:, f0:f0 + 4] = box_muller(uniforms(words(seed, frames, step, draw)))
    return out

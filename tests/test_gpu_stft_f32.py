"""The float32-arithmetic 1024 / 256 transforms on the MI355X, frame by frame against float64: dvae_stft_f32 ->
stft1024_walk_f32_kernel<POWER> and dvae_istft_f32 -> istft1024_walk_f32_kernel (both on Fft512F, csrc/fft_wave.hpp), held to the bounds
and the per-frame L2 bar derived in tests/stft_f32_ref.py (checked on the CPU in tests/test_stft_f32_bounds_cpu.py).  Every bound is
relative to the frame's (the sample's) OWN level, on signals whose level changes every hop over six decades.

Which case reaches which kernel form:

  forward  H.stft_device_f32, layout 2 -> <POWER = false>, layout 1 -> <POWER = true>.  A wave walks chunk = ceil(T / 3072) consecutive
           frames: 3072 = 1024 x STFT_F32_OCC wave slots (dvae_stft_f32, csrc/stft.hip; STFT_F32_OCC = 3 in csrc/stft_types.hpp).  The
           frame counts below are chosen for THAT chunk: they move if STFT_F32_OCC does.
    T = 1 .. 5              chunk 1: no ring step; idle waves in the only workgroup (T = 5: a second workgroup with one busy wave)
    T = 3072, 3073          chunk 1 / chunk 2: ring phase 1; 3073: the last wave holds one frame
    T = 6145                chunk 3: phases 0 .. 2
    T = 9217                chunk 4: all four phases
    T = 12290 .. 12294      chunk 5: the ring wraps (phase 0 again on slots loaded in phases 0 .. 3); the last wave holds
                            T - 5 floor((T - 1) / 5) = 5, 1, 2, 3, 4 frames: a last walk cut by te after every count the chunk allows
    T = 15361               chunk 6 (3.9 M samples)
    wrapper                 packages.processing.stft.stft_pytorch of a CUDA float32 signal, center=True (chunk 1)
  inverse  H.istft_device_f32.  A wave owns chunk = ceil(T / slots) frames, transforms the three halo frames in front of them too, and the
           last chunk flushes the three hops behind frame T - 1.  DVAE_ISTFT_SLOTS=64 (read per call) makes small T reach long chunks:
    T = 1 .. 5              chunk 1; no hop is covered by four frames (`inner` never true, T = 4, 5: hop 3 (and 4) only)
    T = 64 / 65             chunk 1 / chunk 2, the last chunk holds one frame
    T = 129, 193, 321       chunk 3, 4 (the halo shorter than the chunk), 6
    T = 2049, 4097          the default 2048 slots: chunk 2 and 3
    variants, every T       frame-major memory with ld 513 and ld 520 (read in place), bin-major memory (c64_transpose_kernel first; T = 1
                            always, a [513, 1] tensor has no frame-major form); start 0, 512 (the centre trim), 3 (odd: the scalar stores)
                            with out_len five past the signal, and start 0 with out_len five past the signal
    wrapper                 packages.processing.stft.istft_pytorch, center=True

Every test prints its worst figures before it asserts.  Every device allocation comes from a private pool that is emptied when the
module is done (see the fixture).

MEASURED on an MI355X (worst err / bound over all cases of the family; L2: the worst per-frame (per-hop) ratio against the restatement
alone, against host torch alone and against the larger of the two, and the largest median over a case of the ratio against the larger;
stft_f32_ref, PER-FRAME L2 BAR: the median is held to MARGIN = 1.25 in every case, the largest ratio in the `levels` cases).  Every case
inside every bound and bar, every exact zero exact: no kernel or host code needed a fix.
  family                      layout                err/bound          L2 / restatement   L2 / torch   L2 / larger: max   median
  forward levels              2 complex | 1 power   0.027 | 0.025      1.100              1.152        1.084 (held)       0.967
  forward tone_levels         2 complex | 1 power   0.071 | 0.070      1.719              1.484        1.416 (printed)    1.030
  forward impulses            2 complex | 1 power   0.135 | 0.128      silent frames: 0 non-zero values in either layout, every T
  forward wrapper             stft_pytorch          0.015 | 0.016      -                  -            1.016 (held)       0.946
  inverse levels, 64 slots    each of the three     0.0069             1.230              1.233        1.221 (printed)    1.007
  inverse levels, default     each of the three     0.0076             1.309              1.264        1.254 (printed)    0.924
  inverse single frames       each of the three     0.0075             uncovered samples: 0 non-zero values (up to 175 446 of them)
  inverse wrapper             istft_pytorch         0.0049             -                  -            1.075 (printed)    0.906
Over the thousands of frames of a long case the median stands at 0.92 .. 0.95: the kernels contract products into fma, which removes
roundings the restatement keeps.  The largest medians are those of the cases of one to five frames.
The three inverse layouts returned the same figures to the last digit, and so did start 0, 512 and 3.  The component bounds are wide
by construction (they add every rounding in line: a correct transform sits at 2 u32 of the frame's mass against G_F = 41.9); what they
and the exact zeros exclude is a wrong sample, in a quiet frame as in a loud one.  The largest single-frame ratios on tone_levels and
in the inverse are those of single frames in which the two correct CPU implementations differ from each other by as much
(tests/test_stft_f32_bounds_cpu.py prints 1.58 and 1.42).
"""
import gc
import importlib

import numpy as np
import pytest
import torch

import stft_f32_ref as R
from packages.processing import stft as ps

pytestmark = pytest.mark.gpu
H = importlib.import_module("disentangled-vae_amd.stft")

DEV = "cuda"
POISON = 1e30
# chunk = ceil(T / 3072) in dvae_stft_f32 (1024 x STFT_F32_OCC = 3): see the table above
FORWARD_T = [1, 2, 3, 4, 5, 3072, 3073, 6145, 9217, 12290, 12291, 12292, 12293, 12294, 15361]
INVERSE_T_SLOTS64 = [1, 2, 3, 4, 5, 64, 65, 129, 193, 321]
INVERSE_T_DEFAULT = [2049, 4097]
KW = dict(fs=16000, wlen_sec=64e-3, hop_percent=0.25)


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """As in test_gpu_stft_generic.py: every device allocation of this module comes from a private pool of the caching allocator,
    emptied when the module is done, so that the cached blocks of the default pool are exactly those the module found."""
    pool = torch.cuda.MemPool()
    cached = set(H._window_cache)
    with torch.cuda.use_mem_pool(pool):
        yield
        for key in set(H._window_cache) - cached:                                  # the float32 window was allocated in the pool
            del H._window_cache[key]
        gc.collect()
        torch.cuda.synchronize()
    del pool


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

def forward_case(T, name):
    """The signal, its float64 transform and the two yardsticks of the L2 bar."""
    x = {"levels": R.levels, "tone_levels": R.tone_levels}[name](T, T)
    ref, mass = R.forward_reference(x, T)
    rel_rest = R.rel_l2(R.stft_f32(x, T), ref)
    rel_torch = R.rel_l2(R.torch_stft(x, T), ref)
    return x, ref, mass, rel_rest, rel_torch


def check_forward(got2, got1, ref, mass, rel_rest, rel_torch, what):
    """got2: complex64 [T, 513] (layout 2), got1: float32 [T, 513] (layout 1) -> the figures, printed."""
    S = got2.cpu().numpy().T
    comp = R.forward_worst(S, ref, mass)
    rel = R.rel_l2(S, ref)
    l2, med = R.l2_ratio(rel, rel_rest, rel_torch), R.l2_median(rel, rel_rest, rel_torch)
    pw = R.power_worst(got1.cpu().numpy().T, ref, mass)
    print(f"[forward] {what}: component err/bound {comp:.4f}, power err/bound {pw:.4f}, per-frame L2 vs restatement {R.l2_ratio(rel, rel_rest):.3f}, "
          f"vs torch {R.l2_ratio(rel, rel_torch):.3f}, vs the larger: max {l2:.3f}, median {med:.3f} "
          f"(relative L2 {rel.min() / R.U32:.2f} .. {rel.max() / R.U32:.2f} u32)")
    return comp, pw, l2, med


@pytest.mark.parametrize("name", ["levels", "tone_levels"])
@pytest.mark.parametrize("T", FORWARD_T)
def test_forward_every_frame_at_its_own_level(T, name):
    x, ref, mass, rel_rest, rel_torch = forward_case(T, name)
    xd = torch.from_numpy(x).to(DEV)
    comp, pw, l2, med = check_forward(H.stft_device_f32(xd, 1024, 256, T, 2), H.stft_device_f32(xd, 1024, 256, T, 1), ref, mass, rel_rest, rel_torch,
                                      f"{name} T={T} chunk {-(-T // 3072)}")
    assert comp < 1 and pw < 1
    assert med <= R.MARGIN
    assert name != "levels" or l2 <= R.MARGIN                                      # the per-frame maximum: `levels` only (stft_f32_ref)


@pytest.mark.parametrize("T", FORWARD_T)
def test_forward_impulses(T):
    """Frames without an impulse are exactly zero in both layouts; a frame with one is w_i exp(-2 pi i f i / 1024) within the bound."""
    x, pos = R.impulses(T, T)
    ref, mass = R.impulse_reference(T, pos)
    xd = torch.from_numpy(x).to(DEV)
    S = H.stft_device_f32(xd, 1024, 256, T, 2).cpu().numpy().T
    P = H.stft_device_f32(xd, 1024, 256, T, 1).cpu().numpy().T
    silent = mass == 0
    comp, pw = R.forward_worst(S, ref, mass), R.power_worst(P, ref, mass)
    nz = int(np.count_nonzero(S[:, silent])) + int(np.count_nonzero(P[:, silent]))
    print(f"[forward] impulses T={T}: {int(silent.sum())} silent frames of {T}, non-zero values in them {nz}; component err/bound {comp:.4f}, power {pw:.4f}")
    assert T < 5 or (silent.any() and not silent.all())
    assert nz == 0
    assert comp < 1 and pw < 1


def test_wrapper_forward():
    """stft_pytorch of a CUDA float32 signal, center=True, against the float64 transform of the reflect-padded signal."""
    n = 256 * 41 + 57
    x = R.levels(n // 256 + 2, 77)[:n]
    x_ = np.pad(x, (0, 256)) if H.needs_end_pad(n, KW["fs"], KW["wlen_sec"], KW["hop_percent"]) else x
    x_ = np.pad(x_, 512, mode="reflect")
    T = H.frame_count(len(x_), 1024, 256)
    ref, mass = R.forward_reference(x_, T)
    rel_rest, rel_torch = R.rel_l2(R.stft_f32(x_, T), ref), R.rel_l2(R.torch_stft(x_, T), ref)
    out = ps.stft_pytorch(torch.from_numpy(x).to(DEV), center=True, **KW)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (513, T, 2)
    S = torch.view_as_complex(out.contiguous()).cpu().numpy()
    comp = R.forward_worst(S, ref, mass)
    rel = R.rel_l2(S, ref)
    l2, med = R.l2_ratio(rel, rel_rest, rel_torch), R.l2_median(rel, rel_rest, rel_torch)
    pw = R.power_worst((out[..., 0] ** 2 + out[..., 1] ** 2).cpu().numpy(), ref, mass)      # the caller's own power (data_handling.py)
    print(f"[forward] wrapper T={T}: component err/bound {comp:.4f}, power {pw:.4f}, per-frame L2 vs the larger: max {l2:.3f}, median {med:.3f}")
    assert comp < 1 and pw < 1
    assert med <= R.MARGIN and l2 <= R.MARGIN                                      # a `levels` signal


# ---- inverse ----------------------------------------------------------------------------------------------------------------------------

def inverse_case(T):
    S = R.spectrum_levels(T, T)
    ref, bound = R.inverse_reference(S)
    rel_rest = R.rel_l2(R.weighted_hops(R.istft_f32(S), T), R.weighted_hops(ref, T))
    return S, ref, bound, rel_rest, R.inverse_rel_torch(S, ref)


def layouts(S):
    """The spectrum on the device as [513, T] tensors: frame-major ld 513, frame-major ld 520 (padding poisoned), bin-major."""
    T = S.shape[1]
    rows = torch.from_numpy(np.ascontiguousarray(S.T)).to(DEV)
    wide = torch.full((T, 520), complex(POISON, -POISON), dtype=torch.complex64, device=DEV)
    wide[:, :513] = rows
    return {"frame-major ld 513": rows.T, "frame-major ld 520": wide[:, :513].T, "bin-major": torch.from_numpy(np.ascontiguousarray(S)).to(DEV)}


def check_inverse(S, ref, bound, what):
    """Every layout and cut within the per-sample bound, exact zeros behind the signal -> (worst err/bound, the whole signals)."""
    T, ntot = S.shape[1], len(ref)
    worst, whole = 0.0, {}
    for lname, Sd in layouts(S).items():
        for start, out_len in ((0, ntot), (512, ntot - 1024), (3, ntot - 3 + 5), (0, ntot + 5)):
            if out_len == 0:                                                       # T = 1: the centre trim leaves nothing
                continue
            y = H.istft_device_f32(Sd, 1024, 256, T, start, out_len).cpu().numpy()
            r = R.inverse_worst(y, ref, bound, start, out_len)
            behind = y[max(ntot - start, 0):]
            print(f"[inverse] {what} {lname} start={start} out_len={out_len}: err/bound {r:.4f}")
            assert not behind.any() and len(behind) == max(start + out_len - ntot, 0)
            worst = max(worst, r)
            if (start, out_len) == (0, ntot):
                whole[lname] = y
    return worst, whole


def run_inverse(T):
    S, ref, bound, rel_rest, rel_torch = inverse_case(T)
    worst, whole = check_inverse(S, ref, bound, f"T={T}")
    l2, med = 0.0, 0.0
    for lname, y in whole.items():
        rel = R.rel_l2(R.weighted_hops(y, T), R.weighted_hops(ref, T))
        l2, med = max(l2, R.l2_ratio(rel, rel_rest, rel_torch)), max(med, R.l2_median(rel, rel_rest, rel_torch))
        print(f"[inverse] T={T} {lname}: per-hop L2 vs restatement {R.l2_ratio(rel, rel_rest):.3f}, vs torch {R.l2_ratio(rel[2:T + 1], rel_torch[2:T + 1]):.3f}, "
              f"vs the larger: max {R.l2_ratio(rel, rel_rest, rel_torch):.3f}, median {R.l2_median(rel, rel_rest, rel_torch):.3f}")
    print(f"[inverse] T={T}: WORST err/bound {worst:.4f}, per-hop L2 vs the larger: max {l2:.3f}, median {med:.3f}")
    assert worst < 1
    assert med <= R.MARGIN


@pytest.mark.parametrize("T", INVERSE_T_SLOTS64)
def test_inverse_every_sample_at_its_own_level_64_slots(T, monkeypatch):
    monkeypatch.setenv("DVAE_ISTFT_SLOTS", "64")                                   # chunk = ceil(T / 64)
    run_inverse(T)


@pytest.mark.parametrize("T", INVERSE_T_DEFAULT)
def test_inverse_every_sample_at_its_own_level(T, monkeypatch):
    monkeypatch.delenv("DVAE_ISTFT_SLOTS", raising=False)                          # chunk = ceil(T / 2048)
    run_inverse(T)


@pytest.mark.parametrize("T,slots,offset", [(193, "64", 0), (193, "64", 3), (65, "64", 1), (2049, None, 0)])
def test_inverse_of_single_frames_is_zero_elsewhere(T, slots, offset, monkeypatch):
    """Non-zero frames six apart.  T = 193 at 64 slots (chunk 4): from frame 0 they sit first and third in their chunks (the third is
    a halo frame of the next chunk, the first lies in front of its halo), from frame 3 last and second (both halo frames of the next
    chunk); T = 65 (chunk 2: every frame is a halo frame of the next chunk) and the default dispatch (T = 2049, chunk 2) as well.
    Samples that no non-zero frame covers are exactly zero, the others within the bound."""
    if slots is None:
        monkeypatch.delenv("DVAE_ISTFT_SLOTS", raising=False)
    else:
        monkeypatch.setenv("DVAE_ISTFT_SLOTS", slots)
    frames = np.arange(offset, T, 6)
    S = R.sparse_spectrum(T, frames, T)
    ref, bound = R.inverse_reference(S)
    uncovered = bound == 0
    assert uncovered.sum() >= 2 * 256 * (len(frames) - 1)
    worst, whole = check_inverse(S, ref, bound, f"single frames T={T} from {offset}")
    nz = sum(int(np.count_nonzero(y[uncovered])) for y in whole.values())
    print(f"[inverse] single frames T={T} from {offset}: non-zero values among {int(uncovered.sum())} uncovered samples: {nz}; WORST err/bound {worst:.4f}")
    assert nz == 0 and worst < 1


def test_wrapper_inverse():
    """istft_pytorch of a CUDA complex64 spectrogram, center=True: samples [512, ntot - 512) of the untrimmed signal."""
    T = 43
    S, ref, bound, rel_rest, rel_torch = inverse_case(T)
    for lname, Sd in layouts(S).items():
        y = ps.istft_pytorch(Sd, center=True, **KW)
        assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (len(ref) - 1024,)
        y = y.cpu().numpy()
        r = R.inverse_worst(y, ref, bound, 512, len(y))
        rel = R.rel_l2(R.weighted_hops(y, T, 2), R.weighted_hops(ref[512:len(ref) - 512], T, 2))
        l2, med = R.l2_ratio(rel, rel_rest[2:T + 1], rel_torch[2:T + 1]), R.l2_median(rel, rel_rest[2:T + 1], rel_torch[2:T + 1])
        print(f"[inverse] wrapper T={T} {lname}: err/bound {r:.4f}, per-hop L2 vs the larger: max {l2:.3f}, median {med:.3f}")
        assert r < 1
        assert med <= R.MARGIN

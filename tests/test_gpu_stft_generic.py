"""The STFT / ISTFT kernels outside nfft 1024 / hop 256 on the MI355X against a float64 transform, within the bounds derived in
tests/stft_bounds.py (checked on the CPU in tests/test_stft_bounds_cpu.py).  Which case reaches which kernel (csrc/stft.hip):

  forward  pow2 (8/2, 16/4, 512/128, 2048/512)            stft_pow2_kernel<float | double>, layouts 0, 1, 2
           DFT (4/1, 12/3, 800/200, 800/240, 2046/512)    stft_dft_kernel<float | double>, layouts 0, 1, 2
           1024 with hop 128, 512, 1024, 341              stft1024_kernel<., 0> (layout 0), <., 1> and <., 2> (chunk 1; chunk 5 at 8199 frames)
  inverse  pow2                                           istft_frames_pow2_kernel + istft_ola_kernel
           DFT                                            istft_frames_dft_kernel + istft_ola_kernel
           1024 with generic hop                          istft1024_frames_kernel + istft_ola_kernel
  frame-major input of the three frames kernels: test_inverse_c_abi_strides (dvae_istft_frames; nothing in Python reaches it).
  The wrapper tests run packages.processing.stft.stft / istft at 800/200, 800/400, 512/128 and 2048/512.

Every test prints its worst error in units of the bound before it asserts.  No environment switch is set: the generic kernels need
none.  Every device allocation comes from a private pool that is emptied when the module is done (see the fixture).

Measured on an MI355X (worst err / bound over all cases of the family, the wrapper's and the grid-stride cases included; every case
inside its bound, so no kernel or host code needed a fix):
  family             forward complex   forward power   inverse   round trip
  pow2               0.995             0.763           0.561     0.157 (512/128)
  DFT                0.997             0.890           0.604     0.141 (800/200)
  1024, generic hop  0.998             0.974           0.892     -
The complex figures sit just below 1 by construction: the float32 rounding of a component is the bound's first term, and the double
term adds only 1e-13 of the frame's mass (a kernel with float32 twiddles stands at 1e4, tests/test_stft_bounds_cpu.py).  The power
figure of 0.974 is the 8199-frame case (4.2 million values) of stft1024_kernel's power form, whose magnitude comes from the 1-ulp
v_sqrt_f32 and not from hypotf: a worst case of 9 u32 held to the 7 u32 of the bound (tests/stft_bounds.py, POWER); the same
arithmetic with a correctly rounded root stands at 0.765 on the CPU.  The other power cases stay below 0.91.
"""
import gc
import importlib

import numpy as np
import pytest
import torch

import stft_bounds as B
from oracle import stft_oracle as so
from packages.processing import stft as ps

pytestmark = pytest.mark.gpu
H = importlib.import_module("disentangled-vae_amd.stft")
N = importlib.import_module("disentangled-vae_amd.native")

DEV = "cuda"
POISON = 1e30
SENTINEL = -7.5
_windows = {}


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """As in test_gpu_classify.py: every device allocation of this module comes from a private pool of the caching allocator, emptied
    when the module is done, so that the cached blocks of the default pool (which test_gpu_module_path.py's flat-memory check is
    sensitive to) are exactly those the module found."""
    pool = torch.cuda.MemPool()
    cached = set(H._window_cache)
    with torch.cuda.use_mem_pool(pool):
        yield
        _windows.clear()
        for key in set(H._window_cache) - cached:                                  # the wrapper's windows were allocated in the pool
            del H._window_cache[key]
        gc.collect()
        torch.cuda.synchronize()
    del pool


def win_dev(win, nfft):
    """The float64 window on the device (kept in this module's pool, not in the library's cache)."""
    if (win, nfft) not in _windows:
        _windows[win, nfft] = torch.from_numpy(B.window(win, nfft)).to(DEV)
    return _windows[win, nfft]


def frames_that_fit(n, nfft, hop):
    return 1 + (n - nfft) // hop


def stft_raw(x_dev, n, w, nfft, hop, T, layout, out=None):
    """dvae_stft with a free sample count n (<= the buffer's) -> (return code, output tensor)."""
    F = nfft // 2 + 1
    if out is None:
        out = torch.empty((F, T) if layout == 0 else (T, F), dtype=torch.float32 if layout == 1 else torch.complex64, device=DEV)
    rc = N.load().dvae_stft(N.ptr(x_dev), 1 if x_dev.dtype == torch.float64 else 0, n, N.ptr(w), nfft, hop, T, N.ptr(out), layout, N.stream())
    return rc, out


def bin_major(out, layout):
    """The kernel's output as a host array [F, T]."""
    a = out.cpu().numpy()
    return a if layout == 0 else a.T


def check_forward(x, dtype, nfft, hop, T, layouts=(0, 1, 2), n=None, tail=0, what=""):
    """x: float64 host signal.  Transforms the first n samples (default: all) of a device buffer with `tail` poisoned samples behind
    them, in every layout, and returns the worst err / bound against the float64 transform of what the kernel was given."""
    xin = np.asarray(x, dtype)
    n = len(xin) if n is None else n
    buf = np.full(n + tail, POISON, dtype)
    buf[:n] = xin[:n]
    xd = torch.from_numpy(buf).to(DEV)
    w = win_dev("hann", nfft)
    ref, mass = B.forward_reference(xin[:n].astype(np.float64), "hann", nfft, hop, T)
    worst = 0.0
    for layout in layouts:
        if tail == 0:
            out = H.stft_device(xd, w, nfft, hop, T, layout)
        else:
            rc, out = stft_raw(xd, n, w, nfft, hop, T, layout)
            assert rc == 0, N.load().dvae_last_error()
        got = bin_major(out, layout)
        assert got.shape == ref.shape
        r = B.power_worst(got, ref, mass, nfft) if layout == 1 else B.forward_worst(got, ref, mass, nfft)
        print(f"[{B.family(nfft, hop)} forward] {nfft}/{hop} {np.dtype(dtype).name} T={T} n={n}+{tail} layout {layout} {what}: err/bound {r:.3f}")
        worst = max(worst, r)
    return worst


def forward_signals(nfft, hop, T, extra=0):
    n = (T - 1) * hop + nfft + extra
    return {"tone": B.tone_noise(n, nfft, 11 * nfft + hop + T), "noise": np.random.default_rng(13 * nfft + hop + T).standard_normal(n)}


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_forward_within_the_bound(nfft, hop, dtype):
    """Every layout at 1, 2 and 7 frames, a tone between two bins plus weak noise and plain noise; the signal ends exactly with
    the last frame, one sample later, and inside a longer buffer whose tail is poisoned (nothing past n may be read)."""
    worst = 0.0
    for T in (1, 2, 7):
        for name, x in forward_signals(nfft, hop, T, extra=1).items():
            worst = max(worst, check_forward(x[:-1], dtype, nfft, hop, T, what=name))
            worst = max(worst, check_forward(x, dtype, nfft, hop, T, what=name + " one sample more"))
            assert frames_that_fit(len(x), nfft, hop) == T or hop == 1
        x = forward_signals(nfft, hop, T, extra=1)["tone"]
        worst = max(worst, check_forward(x, dtype, nfft, hop, T, n=len(x) - 1, tail=2 * nfft + 3, what="poisoned tail"))
        worst = max(worst, check_forward(x, dtype, nfft, hop, T, n=len(x), tail=2 * nfft + 3, what="poisoned tail, one sample more"))
    print(f"[{B.family(nfft, hop)} forward] {nfft}/{hop} {np.dtype(dtype).name}: WORST {worst:.3f}")
    assert worst < 1


@pytest.mark.parametrize("nfft,hop,T,layouts,dtype", [(16, 4, 2050, (0, 1, 2), np.float64), (12, 3, 2050, (0, 1, 2), np.float32),
                                                      (1024, 128, 2049 * 4 + 3, (1, 2), np.float32)])
def test_forward_grid_stride(nfft, hop, T, layouts, dtype):
    """More frames than the 2048 workgroups of the pow2 and DFT kernels; 1024/128: chunk = 5 frames per wave in stft1024_kernel's
    frame-major forms, the last workgroup ragged (19 of 20 frames)."""
    x = forward_signals(nfft, hop, T)["tone"]
    worst = check_forward(x, dtype, nfft, hop, T, layouts=layouts, what="grid stride")
    print(f"[{B.family(nfft, hop)} forward] {nfft}/{hop} T={T}: WORST {worst:.3f}")
    assert worst < 1


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("wlen,hp", [(50e-3, 0.25), (50e-3, 0.5), (32e-3, 0.25), (128e-3, 0.25)])
def test_wrapper_forward_within_the_bound(wlen, hp, center):
    """packages.processing.stft.stft against the oracle in complex128, lengths with and without the end pad, float64 and float32."""
    nfft, hop = so.stft_sizes(16000, wlen, hp)
    lengths = [20 * hop, 20 * hop + 57]
    assert [so.pad_decision(n, 16000, wlen, hp) for n in lengths] == [False, True]
    worst = 0.0
    for n in lengths:
        for dtype in (np.float64, np.float32):
            x = B.tone_noise(n, nfft, n).astype(dtype)
            kw = dict(fs=16000, wlen_sec=wlen, hop_percent=hp, center=center)
            got = ps.stft(x, **kw)
            ref = so.stft(x.astype(np.float64), dtype="complex128", **kw)
            mass = so.stft(np.abs(x.astype(np.float64)), dtype="complex128", **kw)[0].real     # sum_i w_i |x_i|: the window is not negative
            assert got.shape == ref.shape and got.dtype == np.complex64
            r = B.forward_worst(got, ref, mass, nfft)
            print(f"[{B.family(nfft, hop)} forward] wrapper {nfft}/{hop} center={center} n={n} {np.dtype(dtype).name}: err/bound {r:.3f}")
            worst = max(worst, r)
    assert worst < 1


# ---- inverse ----------------------------------------------------------------------------------------------------------------------------

def spectrum(nfft, T, seed):
    """complex64 noise; the imaginary parts of DC and Nyquist are set, and the kernel must ignore them."""
    rng = np.random.default_rng(seed)
    F = nfft // 2 + 1
    S = (rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))).astype(np.complex64)
    assert S[0].imag.all() and S[-1].imag.all()
    return S


def cuts(nfft, ntot):
    """(start, out_len): the whole signal, the centre trim, out_len past the end, one sample."""
    c = [(0, ntot), (0, ntot + 37), (ntot // 2, 1), (ntot - 1, 3)]
    if ntot - 2 * (nfft // 2) > 0:
        c.append((nfft // 2, ntot - 2 * (nfft // 2)))
    return c


def check_inverse(S, win, nfft, hop, what=""):
    T = S.shape[1]
    ref, M, wss = B.inverse_reference(S, win, nfft, hop)
    Sd = torch.from_numpy(S).to(DEV)
    w = win_dev(win, nfft)
    worst = 0.0
    for start, out_len in cuts(nfft, len(ref)):
        y = H.istft_device(Sd, w, nfft, hop, T, start, out_len).cpu().numpy()
        r = B.inverse_worst(y, ref, M, wss, nfft, hop, start, out_len)
        print(f"[{B.family(nfft, hop)} inverse] {nfft}/{hop} {win} T={T} start={start} out_len={out_len} {what}: err/bound {r:.3f}")
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("win", ["hann", "hamming"])
@pytest.mark.parametrize("nfft,hop", B.SHAPES)
def test_inverse_within_the_bound(nfft, hop, win):
    """Fewer frames than overlaps, exactly as many, one more; no sample excluded (a Hann window's sample 0 must be exactly 0, and
    every sample behind the signal)."""
    nov = B.n_ov(nfft, hop)
    worst = 0.0
    for T in sorted({1, 2, nov, nov + 1, 7}):
        worst = max(worst, check_inverse(spectrum(nfft, T, 3 * nfft + hop + T), win, nfft, hop))
    print(f"[{B.family(nfft, hop)} inverse] {nfft}/{hop} {win}: WORST {worst:.3f}")
    assert worst < 1


@pytest.mark.parametrize("nfft,hop", [(16, 4), (12, 3)])
def test_inverse_grid_stride(nfft, hop):
    """2050 frames: more than the 2048 workgroups of the two frames kernels, and the grid stride of istft_ola_kernel's callers."""
    worst = check_inverse(spectrum(nfft, 2050, nfft), "hann", nfft, hop, what="grid stride")
    print(f"[{B.family(nfft, hop)} inverse] {nfft}/{hop} T=2050: WORST {worst:.3f}")
    assert worst < 1


@pytest.mark.parametrize("nfft,hop", [(800, 200), (512, 128), (1024, 128)])
def test_inverse_c_abi_strides(nfft, hop):
    """dvae_istft on bin-major [F, T + 7] and dvae_istft_frames on frame-major [T, F + 5], the padding poisoned: the bits of the
    tightly packed bin-major call (itself within the bound)."""
    lib = N.load()
    T, F = 7, nfft // 2 + 1
    S = spectrum(nfft, T, nfft + 1)
    ref, M, wss = B.inverse_reference(S, "hann", nfft, hop)
    ntot = len(ref)
    w = win_dev("hann", nfft)
    tight = H.istft_device(torch.from_numpy(S).to(DEV), w, nfft, hop, T, 0, ntot)
    r = B.inverse_worst(tight.cpu().numpy(), ref, M, wss, nfft, hop)
    print(f"[{B.family(nfft, hop)} inverse] {nfft}/{hop} C ABI tight: err/bound {r:.3f}")
    assert r < 1
    ws = torch.empty(max(lib.dvae_istft_workspace_bytes_hop(T, nfft, hop), 16), dtype=torch.uint8, device=DEV)
    wide = torch.full((F, T + 7), complex(POISON, -POISON), dtype=torch.complex64, device=DEV)
    wide[:, :T] = torch.from_numpy(S).to(DEV)
    y = torch.full((ntot,), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(lib.dvae_istft(N.ptr(wide), T, T + 7, N.ptr(w), nfft, hop, 0, N.ptr(y), ntot, N.ptr(ws), N.stream()), "dvae_istft")
    assert torch.equal(tight.view(torch.int32), y.view(torch.int32))
    rows = torch.full((T, F + 5), complex(POISON, -POISON), dtype=torch.complex64, device=DEV)
    rows[:, :F] = torch.from_numpy(np.ascontiguousarray(S.T)).to(DEV)
    y = torch.full((ntot,), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(lib.dvae_istft_frames(N.ptr(rows), T, F + 5, N.ptr(w), nfft, hop, 0, N.ptr(y), ntot, N.ptr(ws), N.stream()), "dvae_istft_frames")
    assert torch.equal(tight.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("center", [False, True])
def test_wrapper_inverse_within_the_bound(center):
    """packages.processing.stft.istft at the reference's default window (50 ms: 800/200) against the oracle in float64: max_len
    None, the signal's length, shorter and longer."""
    nfft, hop, T = 800, 200, 9
    kw = dict(fs=16000, wlen_sec=50e-3, hop_percent=0.25, center=center)
    S = spectrum(nfft, T, 5)
    full = nfft + hop * (T - 1) - (2 * (nfft // 2) if center else 0)
    worst = 0.0
    for max_len in (None, full, full - 333, full + 123):
        ref = so.istft(S, dtype="float64", max_len=max_len, **kw)
        # the oracle's frame truncation, start and length, to place the bound's M and wss on the same samples
        n_frames = T if not max_len else min(T, int(np.ceil((max_len + nfft if center else max_len) / hop)))
        whole, M, wss = B.inverse_reference(S[:, :n_frames], "hann", nfft, hop)
        start = nfft // 2 if center else 0
        assert np.array_equal(B.cut(whole, start, len(ref)), ref)
        got = ps.istft(S, max_len=max_len, **kw)
        assert got.dtype == np.float32 and got.shape == ref.shape
        r = B.inverse_worst(got, whole, M, wss, nfft, hop, start, len(ref))
        print(f"[DFT inverse] wrapper 800/200 center={center} max_len={max_len}: err/bound {r:.3f}")
        worst = max(worst, r)
    assert worst < 1


@pytest.mark.parametrize("nfft,hop", [(800, 200), (512, 128)])
def test_round_trip_returns_the_signal(nfft, hop):
    """istft(stft(x)) = x wherever n_ov frames overlap, within the inverse bound plus the forward bound carried through the inverse."""
    T = 9
    x = np.random.default_rng(nfft).standard_normal((T - 1) * hop + nfft)
    w = win_dev("hann", nfft)
    Sd = H.stft_device(torch.from_numpy(x).to(DEV), w, nfft, hop, T, 0)
    y = H.istft_device(Sd, w, nfft, hop, T, 0, len(x)).cpu().numpy()
    ref, mass = B.forward_reference(x, "hann", nfft, hop, T)
    _, M, wss = B.inverse_reference(Sd.cpu().numpy(), "hann", nfft, hop)
    bound = B.inverse_bound(M, wss, nfft, hop) + B.carried_forward_bound(*B.forward_bound(ref, mass, nfft), "hann", nfft, hop, wss)
    lo, hi = (B.n_ov(nfft, hop) - 1) * hop, T * hop
    r = B.ratio(np.abs(y.astype(np.float64) - x)[lo:hi], bound[lo:hi])
    print(f"[{B.family(nfft, hop)} round trip] {nfft}/{hop}: err/bound {r:.3f} over samples [{lo}, {hi})")
    assert r < 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched():
    """Odd nfft, nfft above 2048 (2050: no power of two, 4096: one), hop 0, frames that do not fit, a leading dimension too small
    for the inverse: a non-zero code, the entry's name in dvae_last_error, and not one output element written."""
    lib = N.load()
    x = torch.ones(20000, dtype=torch.float32, device=DEV)
    w = torch.ones(4096, dtype=torch.float64, device=DEV)
    S = torch.ones((2049, 8), dtype=torch.complex64, device=DEV)
    ws = torch.empty(8 * 4096 * 8, dtype=torch.uint8, device=DEV)

    def refused(rc, name, out):
        torch.cuda.synchronize()
        msg = lib.dvae_last_error().decode()
        print(f"{name}: code {rc}: {msg}")
        assert rc != 0 and name in msg
        assert bool((out == SENTINEL).all())

    for nfft, hop, T in ((801, 200, 4), (7, 2, 4), (2050, 512, 4), (4096, 1024, 4), (800, 0, 4), (800, 200, 98), (512, 128, 154)):
        for layout in (0, 1, 2):
            out = torch.full((4096 * 4,), SENTINEL, dtype=torch.float32, device=DEV)
            assert T == 4 or (T - 1) * hop + nfft > x.numel()
            refused(lib.dvae_stft(N.ptr(x), 0, x.numel(), N.ptr(w), nfft, hop, T, N.ptr(out), layout, N.stream()), "stft", out)
    for entry in (lib.dvae_istft, lib.dvae_istft_frames):
        for nfft, hop in ((801, 200), (7, 2), (2050, 512), (4096, 1024), (800, 0)):
            y = torch.full((4096,), SENTINEL, dtype=torch.float32, device=DEV)
            refused(entry(N.ptr(S), 4, 2049, N.ptr(w), nfft, hop, 0, N.ptr(y), y.numel(), N.ptr(ws), N.stream()), "istft", y)
    y = torch.full((4096,), SENTINEL, dtype=torch.float32, device=DEV)
    refused(lib.dvae_istft(N.ptr(S), 4, 3, N.ptr(w), 800, 200, 0, N.ptr(y), y.numel(), N.ptr(ws), N.stream()), "istft", y)        # [F, ld]: ld < T
    refused(lib.dvae_istft_frames(N.ptr(S), 4, 400, N.ptr(w), 800, 200, 0, N.ptr(y), y.numel(), N.ptr(ws), N.stream()), "istft", y)   # [T, ld]: ld < F
    refused(lib.dvae_istft_frames(N.ptr(S), 4, 256, N.ptr(w), 512, 128, 0, N.ptr(y), y.numel(), N.ptr(ws), N.stream()), "istft", y)

// Forward STFT kernels and their launchers (the inverse: istft.hip; the host entries dvae_stft*, their argument checks and the choice
// between the kernels: stft.hip; the transform pieces the kernels share: fft_wave.hpp; constants and launcher declarations: stft_types.hpp).
//
// STFT / ISTFT for packages/processing/stft.py (librosa semantics restated in
// oracle/stft_oracle.py).  One workgroup walks frames; per frame the nfft real
// samples are windowed and packed into an nfft/2-point complex FFT that runs
// entirely in LDS (double precision: the reference transforms float64 audio
// and only then casts to complex64), followed by the real-FFT split step.
// Twiddles and the window are staged in LDS once per workgroup.
// ISTFT = inverse of the same split + FFT, windowed frames to a scratch
// buffer, then a gather overlap-add that replays librosa's float32
// frame-by-frame accumulation order exactly (deterministic, no atomics).
#include "fft_wave.hpp"
#include "ragged.hpp"
#include "stft_types.hpp"

namespace dvae {

__device__ __forceinline__ void store_bin(void* out, int layout, int64_t T, int F, int64_t t, int f, cd v) {
    float* o = (float*)out;
    const float re = (float)v.x, im = (float)v.y;
    if (layout == 0) {            // complex64 [F][T]  (column = frame)
        o[(f * T + t) * 2] = re;
        o[(f * T + t) * 2 + 1] = im;
    } else if (layout == 2) {     // complex64 [T][F]  (row = frame: the memory order of librosa's Fortran-ordered result)
        o[(t * F + f) * 2] = re;
        o[(t * F + f) * 2 + 1] = im;
    } else {                      // power [T][F] float32: np.abs(complex64)**2
        const float a = hypotf(re, im);
        o[t * F + f] = a * a;
    }
}

template <typename TIN>
__global__ __launch_bounds__(256) void stft_pow2_kernel(const TIN* __restrict__ x, int64_t n, const double* __restrict__ window,
                                                         int nfft, int logM, int hop, int64_t T, void* out, int layout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = nfft >> 1, F = M + 1;
    cd* z = (cd*)smem;
    cd* tw = z + M;
    double* win = (double*)(tw + M);
    stage_tables(tw, win, window, nfft);
    __syncthreads();
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        const int64_t base = t * hop;
        for (int i = threadIdx.x; i < M; i += blockDim.x) {
            const int64_t s0 = base + 2 * i;
            const double a = (s0 < n) ? (double)x[s0] * win[2 * i] : 0.0;
            const double b = (s0 + 1 < n) ? (double)x[s0 + 1] * win[2 * i + 1] : 0.0;
            z[__brev((unsigned)i) >> (32 - logM)] = cd{a, b};
        }
        __syncthreads();
        fft_lds(z, tw, logM, 0);
        // split: X[k] = E + W^k O, X[M-k] = conj(E - W^k O)
        for (int k = threadIdx.x; k <= (M >> 1); k += blockDim.x) {
            const cd zk = z[k], zc = cconj(z[(M - k) & (M - 1)]);
            const cd e = cd{0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y)};
            const cd d = csub(zk, zc);
            const cd o = cd{0.5 * d.y, -0.5 * d.x};          // -0.5 i (zk - zc)
            const cd wo = cmul(tw[k], o);
            store_bin(out, layout, T, F, t, k, cadd(e, wo));
            store_bin(out, layout, T, F, t, M - k, cconj(csub(e, wo)));
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// nfft = 1024 (every caller of the reference): ONE WAVE per frame.  The 512-point complex FFT is three radix-8
// Stockham passes with 8 points per lane in registers; lanes exchange data through a private LDS buffer between
// passes (no workgroup barrier anywhere: a wave's LDS accesses are ordered), the window and all twiddles live in
// registers for the whole launch.  Double precision throughout (the reference transforms float64 audio and only
// then casts to complex64).  Power frames ([T][513], the training layout) leave as 256-byte runs per wave; the
// complex [513][T] layout is staged through LDS 16 frames at a time so each bin's 16 frames leave as one 128-byte run.
template <typename TIN, int LAYOUT>
__global__ __launch_bounds__(256) void stft1024_kernel(const TIN* __restrict__ x, int64_t n, const double* __restrict__ window,
                                                        int hop, int64_t T, int chunk, void* out) {
    constexpr int M = 512, F = 513;
    __shared__ double lre[4][M + 64], lim[4][M + 64];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* stage = reinterpret_cast<float2*>(smem);              // LAYOUT 0: [F][STFT_FR + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* re = lre[wave];
    double* im = lim[wave];
    // per-lane constants
    double wa[8], wb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { wa[r] = window[2 * (lane + 64 * r)]; wb[r] = window[2 * (lane + 64 * r) + 1]; }
    Fft512 fft;
    fft.init(lane);
    double sr[5], si[5];                                                           // split twiddles exp(-2 pi i k / 1024), k = lane + 64 r; [4]: k = 256
#pragma unroll
    for (int r = 0; r < 4; ++r) sincospi(-2.0 * (double)(lane + 64 * r) / 1024.0, &si[r], &sr[r]);
    sr[4] = 0.0; si[4] = -1.0;

    // raw sample pairs of frame t (the zero end-pad is implied past n); requested one frame ahead of the transform
    struct TIN2 { TIN a, b; };
    auto fetch = [&](int64_t t, TIN2 (&raw)[8]) {
        const int64_t base = t * hop;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t s0 = base + 2 * (lane + 64 * r);
            if (s0 + 1 < n) raw[r] = *reinterpret_cast<const TIN2*>(x + s0);      // hop and the pair offset are even: aligned pair loads
            else { raw[r].a = s0 < n ? x[s0] : (TIN)0; raw[r].b = (TIN)0; }
        }
    };
    // consecutive frames overlap by nfft - hop samples: with hop = 256 (128 pairs = 2 slots of 64 lanes) pair slot r of
    // frame t+1 is slot r+2 of frame t IN THE SAME LANE, so a wave walking consecutive frames loads only slots 6 and 7
    auto advance = [&](int64_t tnext, const TIN2 (&prev)[8], TIN2 (&raw)[8]) {
#pragma unroll
        for (int r = 0; r < 6; ++r) raw[r] = prev[r + 2];
        const int64_t base = tnext * hop;
#pragma unroll
        for (int r = 6; r < 8; ++r) {
            const int64_t s0 = base + 2 * (lane + 64 * r);
            if (s0 + 1 < n) raw[r] = *reinterpret_cast<const TIN2*>(x + s0);
            else { raw[r].a = s0 < n ? x[s0] : (TIN)0; raw[r].b = (TIN)0; }
        }
    };
    auto one_frame = [&](int64_t t, const TIN2 (&raw)[8], auto&& emit) {
        cd v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = cd{(double)raw[r].a * wa[r], (double)raw[r].b * wb[r]};
        fft.run(v, re, im, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int i = padidx(lane + 64 * r); re[i] = v[r].x; im[i] = v[r].y; }
        __builtin_amdgcn_wave_barrier();
        // real-FFT split: X[k] = E + W^k O, X[M-k] = conj(E - W^k O), partner z[M-k] from LDS
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            const int pi = padidx((M - k) & (M - 1));
            const cd zk = v[r], zc = cd{re[pi], -im[pi]};
            const cd e = cd{0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y)};
            const cd d = csub(zk, zc);
            const cd wo = cmulc(cd{0.5 * d.y, -0.5 * d.x}, sr[r], si[r]);
            emit(k, cadd(e, wo));
            emit(M - k, cconj(csub(e, wo)));
        }
        if (lane == 0) {                                         // k = 256 (its own partner): X = E + (-i) O
            const cd zk = v[4];
            emit(256, cd{zk.x, -zk.y});
        }
        __builtin_amdgcn_wave_barrier();
    };

    TIN2 cur[8], nxt[8];
    if (LAYOUT == 2) {
        // complex frames, frame-major: the walk of the power layout, each bin leaving as its complex64 value (512-byte runs per wave)
        float2* o = (float2*)out;
        const int64_t tb = ((int64_t)blockIdx.x * 4 + wave) * chunk;
        const int64_t te = tb + chunk < T ? tb + chunk : T;
        if (tb < te) fetch(tb, cur);
        for (int64_t t = tb; t < te; ++t) {
            if (t + 1 < te) { if (hop == 256) advance(t + 1, cur, nxt); else fetch(t + 1, nxt); }
            one_frame(t, cur, [&](int f, cd X) { o[t * F + f] = float2{(float)X.x, (float)X.y}; });
#pragma unroll
            for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
        }
    } else if (LAYOUT == 1) {
        float* o = (float*)out;
        // each wave walks `chunk` consecutive frames (chunk chosen by the host so that the launch still fills the chip)
        const int64_t tb = ((int64_t)blockIdx.x * 4 + wave) * chunk;
        const int64_t te = tb + chunk < T ? tb + chunk : T;
        if (tb < te) fetch(tb, cur);
        for (int64_t t = tb; t < te; ++t) {
            if (t + 1 < te) { if (hop == 256) advance(t + 1, cur, nxt); else fetch(t + 1, nxt); }   // in flight under this frame's transform
            one_frame(t, cur, [&](int f, cd X) {
                // np.abs(complex64) ** 2: float32 magnitude, then its square.  The magnitudes here are far from
                // overflow, so the square root of re^2 + im^2 stands in for hypotf (30 instructions).  __fsqrt_rn is the
                // 1-ulp v_sqrt_f32 here (HIP's headers round it correctly only under OCML_BASIC_ROUNDED_OPERATIONS), on a sum
                // with two roundings: the magnitude is within 1.5 ulp, not hypotf's 1 (tests/stft_bounds.py, POWER)
                const float re32 = (float)X.x, im32 = (float)X.y;
                const float a = __fsqrt_rn(fmaf(re32, re32, im32 * im32));
                o[t * F + f] = a * a;
            });
#pragma unroll
            for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
        }
    } else {
        float2* o = (float2*)out;
        for (int64_t t0 = (int64_t)blockIdx.x * STFT_FR; t0 < T; t0 += (int64_t)gridDim.x * STFT_FR) {
            constexpr int PW = STFT_FR / 4;                           // consecutive frames per wave
            if (t0 + wave * PW < T) fetch(t0 + wave * PW, cur);
            for (int q = wave * PW; q < (wave + 1) * PW; ++q) {
                const int64_t t = t0 + q;
                if (q + 1 < (wave + 1) * PW && t + 1 < T) { if (hop == 256) advance(t + 1, cur, nxt); else fetch(t + 1, nxt); }
                if (t < T) one_frame(t, cur, [&](int f, cd X) { stage[f * (STFT_FR + 1) + q] = float2{(float)X.x, (float)X.y}; });
#pragma unroll
                for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
            }
            __syncthreads();
            const int nq = (int)(T - t0 < STFT_FR ? T - t0 : STFT_FR);
            for (int idx = threadIdx.x; idx < F * STFT_FR; idx += 256) {
                const int f = idx / STFT_FR, q = idx - f * STFT_FR;
                if (q < nq) o[(int64_t)f * T + t0 + q] = stage[f * (STFT_FR + 1) + q];
            }
            __syncthreads();
        }
    }
}

// hop = 256 (every caller of the reference), frame-major outputs: the walk of stft1024_kernel<., 1 / 2> with the per-frame VALU work that is
// not the transform taken out.  Round 3 measured the walk at ~100 % VALU issue (2 waves per SIMD, 520 VALU instructions per frame, 282 of them
// fp64 transform arithmetic); the rest was (a) 48 v_mov_b64 rotating the six carried sample pairs from one frame's slots into the next, (b) ~80
// instructions of 64-bit address arithmetic and end-of-signal compares around 10 loads and 9 stores, (c) the denormal-input scaling hipcc wraps
// around v_sqrt_f32 (5 of 10 instructions per bin).  Here: (a) the pairs live in a ring of 8 registers indexed by frame number mod 4 -- the loop
// is unrolled by four and nothing moves; (b) loads and stores go through buffer descriptors: one per-lane byte offset, the frame offset in an
// SGPR (the scalar offset is outside the descriptor's range check on gfx9: every access is in range by the host's own check that all T
// frames fit in n samples, dvae_stft: "(T - 1) hop + nfft <= n" -- the caller passes the end-padded signal); (c) the raw v_sqrt_f32 (1 ulp,
// not the correctly rounded sqrtf: its square is within ~2 ulp of np.abs(complex64) ** 2, inside the 4e-7 relative bound at which
// tests/test_gpu_stft.py pins the reference's HDF5 power frames; |X|^2 below 1.2e-38 -- where the reference's own result is a denormal
// or zero -- gives 0: parity for denormal magnitudes is unpinned by any reference fixture).
//
// BATCH (dvae_stft_batch): the same walk over a ragged batch.  A wave's work item is one utterance and a run of at most `chunk` of its
// frames; tab = [item prefix (U + 1) | first output frame (U + 1) | first signal sample (U)] (int64, see batch_item).  The buffer
// descriptors are built from the utterance's own base address, so the 32-bit byte-offset limit holds per utterance, not per batch.
template <typename TIN, bool POWER, bool OCC3, bool BATCH = false>
__global__ __launch_bounds__(256, OCC3 ? 3 : 2) void stft1024_walk_kernel(const TIN* __restrict__ x, int64_t n, const double* __restrict__ window, int64_t T, int chunk,
                                                             void* out, const int64_t* __restrict__ tab = nullptr, int U = 0) {
    static_assert(!(BATCH && OCC3), "the batch walk has the two-wave form only");
    constexpr int M = 512, F = 513;
    constexpr int ESZ = POWER ? 4 : 8;
    __shared__ double lre[4][M + 64], lim[4][M + 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform frame numbers: scalar buffer offsets)
    double* re = lre[wave];
    double* im = lim[wave];
    // OCC3 (diagnostic build, measured slower -- see the launcher): three waves per SIMD (<= 168 registers): the window (32 registers), the
    // pass-1 twiddles (28) and the split twiddles (16) are read from LDS tables every frame instead (19 ds_read_b128)
    __shared__ double2 lwin[OCC3 ? M : 1], lsp[OCC3 ? M / 2 : 1], lt1[OCC3 ? 64 : 1];
    double wa[OCC3 ? 1 : 8], wb[OCC3 ? 1 : 8], sr[OCC3 ? 1 : 4], si[OCC3 ? 1 : 4];
    typename std::conditional<OCC3, Fft512L, Fft512>::type fft;
    fft.init(lane);
    if constexpr (OCC3) {
        for (int k = threadIdx.x; k < M; k += 256) lwin[k] = double2{window[2 * k], window[2 * k + 1]};
        for (int k = threadIdx.x; k < M / 2; k += 256) { double sn, cs; sincospi(-2.0 * (double)k / 1024.0, &sn, &cs); lsp[k] = double2{cs, sn}; }
        if (threadIdx.x < 64) { double sn, cs; sincospi(-2.0 * (double)((threadIdx.x & 7) * (threadIdx.x >> 3)) / 64.0, &sn, &cs); lt1[threadIdx.x] = double2{cs, sn}; /* entry (k = tid >> 3, r = tid & 7) */ }
        __syncthreads();
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) { wa[r] = window[2 * (lane + 64 * r)]; wb[r] = window[2 * (lane + 64 * r) + 1]; }
#pragma unroll
        for (int r = 0; r < 4; ++r) sincospi(-2.0 * (double)(lane + 64 * r) / 1024.0, &si[r], &sr[r]);   // split twiddles exp(-2 pi i k / 1024), k = lane + 64 r
    }

    int64_t tb = ((int64_t)blockIdx.x * 4 + wave) * chunk;
    if constexpr (BATCH) {
        const BatchItem it = batch_item(tab, U, (int64_t)blockIdx.x * 4 + wave);
        if (it.u < 0) return;
        const int64_t f0 = uni64(tab[U + 1 + it.u]), Tu = uni64(tab[U + 2 + it.u]) - f0, s0 = uni64(tab[2 * U + 2 + it.u]);
        const int64_t nu = (Tu - 1) * 256 + 1024;                               // the samples the utterance's frames read
        // a table the host's checks would have refused: the wave leaves without touching memory
        if (Tu < 1 || f0 < 0 || f0 + Tu > T || s0 < 0 || s0 + nu > n || nu * (int64_t)sizeof(TIN) >= ((int64_t)1 << 31) ||
            Tu * F * ESZ >= ((int64_t)1 << 31) || it.local * chunk >= Tu) return;
        x += s0;
        n = nu;
        out = (char*)out + f0 * F * ESZ;
        T = Tu;
        tb = it.local * chunk;
    }
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<TIN*>(x), 0, (int)(n * (int64_t)sizeof(TIN)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(T * F * ESZ), 0x00020000);
    struct TIN2 { TIN a, b; };
    const int vx = lane * 2 * (int)sizeof(TIN);
    // pair slot r of frame t: samples 256 t + 128 r + 2 lane, + 1 (always inside n: the host checks that every frame fits)
    auto ldpair = [&](int64_t t, int r) __attribute__((always_inline)) {
        const int so = (int)((t * 256 + 128 * r) * (int64_t)sizeof(TIN));
        if constexpr (sizeof(TIN) == 8) {
            typedef unsigned u4 __attribute__((ext_vector_type(4)));
            const u4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, vx, so, 0);
            return __builtin_bit_cast(TIN2, v);
        } else {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            const u2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_x, vx, so, 0);
            return __builtin_bit_cast(TIN2, v);
        }
    };
    const int vk = lane * ESZ, vm = (M - 192 - lane) * ESZ;                        // bins lane + 64 r / 512 - lane - 64 r: + 64 r ESZ / + 64 (3 - r) ESZ
    auto put = [&](int voff, int so, cd X) __attribute__((always_inline)) {
        const float re32 = (float)X.x, im32 = (float)X.y;
        if constexpr (POWER) {
            // np.abs(complex64) ** 2: float32 magnitude (v_sqrt_f32 of re^2 + im^2, 1 ulp, stands in for hypotf: far from overflow), squared
            const float a = __builtin_amdgcn_sqrtf(fmaf(re32, re32, im32 * im32));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, a * a), rs_o, voff, so, 0);
        } else {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(u2{__builtin_bit_cast(unsigned, re32), __builtin_bit_cast(unsigned, im32)}, rs_o, voff, so, 0);
        }
    };

    const int64_t te = tb + chunk < T ? tb + chunk : T;
    TIN2 buf[8];                                                                   // ring: slot r of a frame with t - tb = p (mod 4) is buf[(r + 2 p) & 7]
    if (tb < te) {
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[r] = ldpair(tb, r);
    }
    auto frame = [&](auto phc, int64_t t) __attribute__((always_inline)) {
        constexpr int PH = decltype(phc)::value;
        cd v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const TIN2 q = buf[(r + 2 * PH) & 7];
            if constexpr (OCC3) { const double2 w = lwin[lane + 64 * r]; v[r] = cd{(double)q.a * w.x, (double)q.b * w.y}; }
            else v[r] = cd{(double)q.a * wa[r], (double)q.b * wb[r]};
        }
        if (t + 1 < te) {                                                          // slots 6, 7 of the next frame take the places of this frame's slots 0, 1
            buf[(2 * PH) & 7] = ldpair(t + 1, 6);
            buf[(2 * PH + 1) & 7] = ldpair(t + 1, 7);
        }
        if constexpr (OCC3) fft.run(v, re, im, lane, lt1); else fft.run(v, re, im, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int i = padidx(lane + 64 * r); re[i] = v[r].x; im[i] = v[r].y; }
        __builtin_amdgcn_wave_barrier();
        const int so = (int)(t * F * ESZ);
        // real-FFT split: X[k] = E + W^k O, X[M-k] = conj(E - W^k O), partner z[M-k] from LDS
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            const int pi = padidx((M - k) & (M - 1));
            const cd zk = v[r], zc = cd{re[pi], -im[pi]};
            const cd e = cd{0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y)};
            const cd d = csub(zk, zc);
            double swr, swi;
            if constexpr (OCC3) { const double2 w = lsp[k]; swr = w.x; swi = w.y; } else { swr = sr[r]; swi = si[r]; }
            const cd wo = cmulc(cd{0.5 * d.y, -0.5 * d.x}, swr, swi);
            put(vk + 64 * r * ESZ, so, cadd(e, wo));
            put(vm + 64 * (3 - r) * ESZ, so, cconj(csub(e, wo)));
        }
        if (lane == 0) put(256 * ESZ, so, cd{v[4].x, -v[4].y});                    // k = 256 (its own partner): X = E + (-i) O
        __builtin_amdgcn_wave_barrier();
    };
    for (int64_t t = tb; t < te; t += 4) {
        frame(std::integral_constant<int, 0>{}, t);
        if (t + 1 < te) frame(std::integral_constant<int, 1>{}, t + 1);
        if (t + 2 < te) frame(std::integral_constant<int, 2>{}, t + 2);
        if (t + 3 < te) frame(std::integral_constant<int, 3>{}, t + 3);
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 ARITHMETIC, nfft = 1024 / hop = 256: the transform of stft_pytorch (packages/processing/stft.py:123-152 = torch.stft on an fp32
// tensor with torch.hann_window(1024): window product, FFT and output all in float32; the caller squares and adds in float32 as well,
// packages/data_handling.py:136).  The float64 walk above stays the transform of stft() (librosa multiplies by a float64 window, so its
// FFT runs in double whatever the audio's type) and of every bit-level pin.  Same walk -- one wave per frame, three radix-8 Stockham
// passes, 8 points per lane, six of the eight sample pairs carried over in a register ring -- with what the narrower type buys: a point
// is ONE 8-byte LDS slot (re, im) instead of two 8-byte doubles (half the exchange instructions, half the bytes), no fp64 VALU (half
// rate on gfx950), and under 128 registers, i.e. four waves per SIMD instead of two.
template <bool POWER>
__global__ __launch_bounds__(256, STFT_F32_OCC) void stft1024_walk_f32_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ window, int64_t T,
                                                                              int chunk, void* out) {
    constexpr int M = 512, F = 513;
    constexpr int ESZ = POWER ? 4 : 8;
    __shared__ __attribute__((aligned(8))) cf lz[4][M + 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* z = lz[wave];
    float wa[8], wb[8], sr[4], si[4];
    Fft512F fft;
    fft.init(lane);
#pragma unroll
    for (int r = 0; r < 8; ++r) { wa[r] = window[2 * (lane + 64 * r)]; wb[r] = window[2 * (lane + 64 * r) + 1]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) { double sn, cs; sincospi(-2.0 * (double)(lane + 64 * r) / 1024.0, &sn, &cs); sr[r] = (float)cs; si[r] = (float)sn; }

    // every access in range by the host's check that all T frames fit in n samples (the scalar offset is not range-checked)
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)(n * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(T * F * ESZ), 0x00020000);
    const int vx = lane * 8;
    auto ldpair = [&](int64_t t, int r) __attribute__((always_inline)) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        const u2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_x, vx, (int)((t * 256 + 128 * r) * 4), 0);
        return __builtin_bit_cast(cf, v);                                          // (samples 2 lane, 2 lane + 1 of the slot)
    };
    const int vk = lane * ESZ, vm = (M - 192 - lane) * ESZ;
    auto put = [&](int voff, int so, cf X) __attribute__((always_inline)) {
        if constexpr (POWER) {
            // x_tf[..., 0] ** 2 + x_tf[..., 1] ** 2 (packages/data_handling.py:136): two rounded squares, one rounded sum
            // (contraction switched off for the expression: __fmul_rn / __fadd_rn are plain operators in HIP's headers and would fuse)
            float pw;
            {
#pragma clang fp contract(off)
                const float a2 = X.x * X.x, b2 = X.y * X.y;
                pw = a2 + b2;
            }
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pw), rs_o, voff, so, 0);
        } else {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, X), rs_o, voff, so, 0);
        }
    };
    const int64_t tb = ((int64_t)blockIdx.x * 4 + wave) * chunk;
    const int64_t te = tb + chunk < T ? tb + chunk : T;
    cf buf[8];                                                                     // ring: slot r of a frame with t - tb = p (mod 4) is buf[(r + 2 p) & 7]
    if (tb < te) {
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[r] = ldpair(tb, r);
    }
    auto frame = [&](auto phc, int64_t t) __attribute__((always_inline)) {
        constexpr int PH = decltype(phc)::value;
        cf v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { const cf q = buf[(r + 2 * PH) & 7]; v[r] = cf{q.x * wa[r], q.y * wb[r]}; }
        if (t + 1 < te) {
            buf[(2 * PH) & 7] = ldpair(t + 1, 6);
            buf[(2 * PH + 1) & 7] = ldpair(t + 1, 7);
        }
        fft.run(v, z, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) z[padidx(lane + 64 * r)] = v[r];
        __builtin_amdgcn_wave_barrier();
        const int so = (int)(t * F * ESZ);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            const cf zk = v[r], zc = cconj(z[padidx((M - k) & (M - 1))]);
            const cf e = cf{0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y)};
            const cf d = csub(zk, zc);
            const cf wo = cmulc(cf{0.5f * d.y, -0.5f * d.x}, sr[r], si[r]);
            put(vk + 64 * r * ESZ, so, cadd(e, wo));
            put(vm + 64 * (3 - r) * ESZ, so, cconj(csub(e, wo)));
        }
        if (lane == 0) put(256 * ESZ, so, cf{v[4].x, -v[4].y});
        __builtin_amdgcn_wave_barrier();
    };
    for (int64_t t = tb; t < te; t += 4) {
        frame(std::integral_constant<int, 0>{}, t);
        if (t + 1 < te) frame(std::integral_constant<int, 1>{}, t + 1);
        if (t + 2 < te) frame(std::integral_constant<int, 2>{}, t + 2);
        if (t + 3 < te) frame(std::integral_constant<int, 3>{}, t + 3);
    }
}

// generic O(N^2) DFT for non power-of-two window lengths (e.g. the wrapper's never-used
// default 50 ms = 800 samples): API completeness only.
template <typename TIN>
__global__ __launch_bounds__(256) void stft_dft_kernel(const TIN* __restrict__ x, int64_t n, const double* __restrict__ window,
                                                        int nfft, int hop, int64_t T, void* out, int layout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cd* tw = (cd*)smem;                 // nfft entries exp(-2 pi i k / nfft)
    double* fr = (double*)(tw + nfft);  // windowed frame
    const int F = nfft / 2 + 1;
    for (int k = threadIdx.x; k < nfft; k += blockDim.x) {
        double s, c;
        sincospi(-2.0 * (double)k / (double)nfft, &s, &c);
        tw[k] = cd{c, s};
    }
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        __syncthreads();
        for (int i = threadIdx.x; i < nfft; i += blockDim.x) {
            const int64_t s0 = t * hop + i;
            fr[i] = (s0 < n) ? (double)x[s0] * window[i] : 0.0;
        }
        __syncthreads();
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            double re = 0.0, im = 0.0;
            int idx = 0;
            for (int i = 0; i < nfft; ++i) {
                re += fr[i] * tw[idx].x;
                im += fr[i] * tw[idx].y;
                idx += f; if (idx >= nfft) idx -= nfft;
            }
            store_bin(out, layout, T, F, t, f, cd{re, im});
        }
    }
}

// ---- launchers (declared in stft_types.hpp)

// the in_f64 x layout ladder of the double walk, once for its three forms (product, OCC3, batch)
template <bool OCC3, bool BATCH>
static void stft1024_walk_launch(const void* x, int in_f64, int64_t n, const double* window, int64_t T, int chunk, void* out, int layout,
                                 const int64_t* tab, int U, dim3 grid, hipStream_t s) {
    if (layout == 1) {
        if (in_f64) hipLaunchKernelGGL((stft1024_walk_kernel<double, true, OCC3, BATCH>), grid, dim3(256), 0, s, (const double*)x, n, window, T, chunk, out, tab, U);
        else hipLaunchKernelGGL((stft1024_walk_kernel<float, true, OCC3, BATCH>), grid, dim3(256), 0, s, (const float*)x, n, window, T, chunk, out, tab, U);
    } else {
        if (in_f64) hipLaunchKernelGGL((stft1024_walk_kernel<double, false, OCC3, BATCH>), grid, dim3(256), 0, s, (const double*)x, n, window, T, chunk, out, tab, U);
        else hipLaunchKernelGGL((stft1024_walk_kernel<float, false, OCC3, BATCH>), grid, dim3(256), 0, s, (const float*)x, n, window, T, chunk, out, tab, U);
    }
}

int launch_stft1024_walk(const void* x, int in_f64, int64_t n, const double* window, int64_t T, int chunk, void* out, int layout, bool occ3,
                         const int64_t* tab, int U, int64_t n_items, hipStream_t s) {
    if (tab) stft1024_walk_launch<false, true>(x, in_f64, n, window, T, chunk, out, layout, tab, U, dim3((unsigned)cdiv(n_items, 4)), s);
    else if (occ3) {
        if constexpr (kDiagBuild) stft1024_walk_launch<true, false>(x, in_f64, n, window, T, chunk, out, layout, nullptr, 0, dim3((int)cdiv(T, (int64_t)4 * chunk)), s);
    } else stft1024_walk_launch<false, false>(x, in_f64, n, window, T, chunk, out, layout, nullptr, 0, dim3((int)cdiv(T, (int64_t)4 * chunk)), s);
    DVAE_LAUNCH_OK(tab ? "stft1024_walk_kernel (batch)" : "stft");
    return 0;
}

int launch_stft1024(const void* x, int in_f64, int64_t n, const double* window, int hop, int64_t T, int chunk, void* out, int layout, hipStream_t s) {
    if (layout != 0) {
        const int wb = (int)cdiv(T, (int64_t)4 * chunk);
        if (layout == 1) {
            if (in_f64) hipLaunchKernelGGL((stft1024_kernel<double, 1>), dim3(wb), dim3(256), 0, s, (const double*)x, n, window, hop, T, chunk, out);
            else hipLaunchKernelGGL((stft1024_kernel<float, 1>), dim3(wb), dim3(256), 0, s, (const float*)x, n, window, hop, T, chunk, out);
        } else {
            if (in_f64) hipLaunchKernelGGL((stft1024_kernel<double, 2>), dim3(wb), dim3(256), 0, s, (const double*)x, n, window, hop, T, chunk, out);
            else hipLaunchKernelGGL((stft1024_kernel<float, 2>), dim3(wb), dim3(256), 0, s, (const float*)x, n, window, hop, T, chunk, out);
        }
    } else {
        const int wb = (int)(cdiv(T, STFT_FR) < 2048 ? cdiv(T, STFT_FR) : 2048);
        const size_t lds = (size_t)513 * (STFT_FR + 1) * sizeof(float2);
        static bool attr_done = false;
        if (!attr_done) {
            DVAE_HIP(hipFuncSetAttribute((const void*)stft1024_kernel<double, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            DVAE_HIP(hipFuncSetAttribute((const void*)stft1024_kernel<float, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_done = true;
        }
        if (in_f64) hipLaunchKernelGGL((stft1024_kernel<double, 0>), dim3(wb), dim3(256), lds, s, (const double*)x, n, window, hop, T, 1, out);
        else hipLaunchKernelGGL((stft1024_kernel<float, 0>), dim3(wb), dim3(256), lds, s, (const float*)x, n, window, hop, T, 1, out);
    }
    DVAE_LAUNCH_OK("stft");
    return 0;
}

int launch_stft_pow2(const void* x, int in_f64, int64_t n, const double* window, int nfft, int logM, int hop, int64_t T, void* out, int layout, hipStream_t s) {
    const int blocks = (int)(T < 2048 ? T : 2048);
    const size_t lds = (size_t)(nfft / 2) * 2 * sizeof(cd) + (size_t)nfft * sizeof(double);
    if (in_f64)
        hipLaunchKernelGGL((stft_pow2_kernel<double>), dim3(blocks), dim3(256), lds, s, (const double*)x, n, window, nfft, logM, hop, T, out, layout);
    else
        hipLaunchKernelGGL((stft_pow2_kernel<float>), dim3(blocks), dim3(256), lds, s, (const float*)x, n, window, nfft, logM, hop, T, out, layout);
    DVAE_LAUNCH_OK("stft");
    return 0;
}

int launch_stft_dft(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop, int64_t T, void* out, int layout, hipStream_t s) {
    const int blocks = (int)(T < 2048 ? T : 2048);
    const size_t lds = (size_t)nfft * sizeof(cd) + (size_t)nfft * sizeof(double);
    if (in_f64)
        hipLaunchKernelGGL((stft_dft_kernel<double>), dim3(blocks), dim3(256), lds, s, (const double*)x, n, window, nfft, hop, T, out, layout);
    else
        hipLaunchKernelGGL((stft_dft_kernel<float>), dim3(blocks), dim3(256), lds, s, (const float*)x, n, window, nfft, hop, T, out, layout);
    DVAE_LAUNCH_OK("stft");
    return 0;
}

int launch_stft1024_walk_f32(const float* x, int64_t n, const float* window, int64_t T, int chunk, void* out, int layout, hipStream_t s) {
    const int wb = (int)cdiv(T, (int64_t)4 * chunk);
    if (layout == 1) hipLaunchKernelGGL((stft1024_walk_f32_kernel<true>), dim3(wb), dim3(256), 0, s, x, n, window, T, chunk, out);
    else hipLaunchKernelGGL((stft1024_walk_f32_kernel<false>), dim3(wb), dim3(256), 0, s, x, n, window, T, chunk, out);
    DVAE_LAUNCH_OK("stft1024_walk_f32_kernel");
    return 0;
}

}  // namespace dvae

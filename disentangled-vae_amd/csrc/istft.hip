// Inverse STFT kernels and their launchers (the forward kernels, with the description of the transform itself: stft_fwd.hip; the host
// entries dvae_istft*, their argument checks and the choice between the kernels: stft.hip; the transform pieces: fft_wave.hpp; IstftBatch,
// constants and launcher declarations: stft_types.hpp).
// ISTFT = inverse of the real-FFT split + FFT, windowed frames, then an overlap-add that replays librosa's float32 frame-by-frame
// accumulation order exactly (deterministic, no atomics): to a scratch buffer and a gather (istft*_frames*_kernel + istft_ola_kernel), or
// in one kernel for nfft = 1024 / hop = 256 (istft1024_fused_kernel, istft1024_walk_kernel).
#include <float.h>
#include "fft_wave.hpp"
#include "ragged.hpp"
#include "stft_types.hpp"

namespace dvae {

// nfft = 1024: frames[t][m] = window[m] * irfft(S[:, t])[m] with ONE WAVE per frame (same FFT core, run on the
// conjugate: ifft(Z) = conj(fft(conj Z)) / M).  S is [bin][T]: a workgroup stages 16 consecutive frames through LDS
// (one 128-byte run per bin) and its four waves take four frames each.
__global__ __launch_bounds__(256) void istft1024_frames_kernel(const float2* __restrict__ S, int64_t T, int64_t sf, int64_t st,
                                                               const double* __restrict__ window, double* __restrict__ frames) {
    constexpr int M = 512, F = 513, PW = ISTFT_FR / 4;
    __shared__ double lre[4][M + 64], lim[4][M + 64];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* stage = reinterpret_cast<float2*>(smem);              // [F][ISTFT_FR + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* re = lre[wave];
    double* im = lim[wave];
    double wa[8], wb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { wa[r] = window[2 * (lane + 64 * r)] * (1.0 / M); wb[r] = window[2 * (lane + 64 * r) + 1] * (1.0 / M); }
    Fft512 fft;
    fft.init(lane);
    double sr[8], si[8];                                          // exp(+2 pi i k / 1024), k = lane + 64 r
#pragma unroll
    for (int r = 0; r < 8; ++r) sincospi(2.0 * (double)(lane + 64 * r) / 1024.0, &si[r], &sr[r]);
    for (int64_t t0 = (int64_t)blockIdx.x * ISTFT_FR; t0 < T; t0 += (int64_t)gridDim.x * ISTFT_FR) {
        const int nq = (int)(T - t0 < ISTFT_FR ? T - t0 : ISTFT_FR);
        __syncthreads();                                          // the previous block's readers are done with `stage`
        for (int idx = threadIdx.x; idx < F * ISTFT_FR; idx += 256) {
            const int f = idx / ISTFT_FR, q = idx - f * ISTFT_FR;
            if (q < nq) stage[f * (ISTFT_FR + 1) + q] = S[(int64_t)f * sf + (t0 + q) * st];
        }
        __syncthreads();
        for (int q = wave * PW; q < (wave + 1) * PW && q < nq; ++q) {
            cd v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int k = lane + 64 * r;
                const float2 a = stage[k * (ISTFT_FR + 1) + q], b = stage[(M - k) * (ISTFT_FR + 1) + q];
                cd xk = cd{(double)a.x, (double)a.y}, xc = cd{(double)b.x, -(double)b.y};   // X[k], conj(X[M-k])
                if (k == 0) { xk.y = 0.0; xc.y = 0.0; }                                      // C2R ignores imag of DC / Nyquist
                const cd e = cd{0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y)};
                const cd o = cmulc(cd{0.5 * (xk.x - xc.x), 0.5 * (xk.y - xc.y)}, sr[r], si[r]);
                v[r] = cd{e.x - o.y, -(e.y + o.x)};               // conj(E + i O)
            }
            fft.run(v, re, im, lane);
            double* dst = frames + (t0 + q) * 1024;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int i = lane + 64 * r;
                reinterpret_cast<double2*>(dst)[i] = double2{wa[r] * v[r].x, -wb[r] * v[r].y};   // conj, 1/M folded into the window
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// nfft = 1024, hop = 256 (every caller of the reference): inverse FFT AND overlap-add in one kernel, no frame scratch.
// The two-kernel form above writes every windowed frame to HBM in double (8 KB per frame: 307 MB for ten minutes of audio) and
// gathers it back; here a workgroup owns a chunk of IF_K consecutive frames and the IF_K * 256 output samples they complete.
// It computes the chunk's frames plus the three frames in front of it (whose tails reach into the chunk: 10 % more FFTs, no
// exchange between workgroups), one wave per frame, four consecutive frames per round; after each round the four frames sit in
// LDS and all 256 threads add them into the chunk's float output image IN FRAME ORDER with one float rounding per addition --
// exactly the arithmetic of librosa's in-place `y[...] += ytmp` and of istft_ola_kernel (the results are bit-identical).
// Chunk sizes: NPASS staging passes of IF_FR frames (one 8 * IF_FR-byte run per bin), three of the frames halo; short
// utterances take small chunks so that the launch still covers the CUs.  The next pass's S values are requested into registers
// before the current pass's FFT rounds and committed to LDS after them.
constexpr int IF_H = 3;
template <int IF_FR, int NPASS> struct IstftFusedLds {
    static constexpr int R = NPASS * IF_FR, K = R - IF_H;   // frames computed / owned per chunk
    static constexpr int ACC = R * 256 + 768;                  // floats of the output image: frame R - 1 ends at (R - 1) * 256 + 1023
    double ex[4][1152];                                        // per wave: FFT exchange buffers (re: 576, im: 576), then its windowed frame (1024)
    float2 stage[513 * (IF_FR + 1)];                        // IF_FR frames of S: [bin][IF_FR + 1] (S bin-major, one (8 * IF_FR)-byte run per bin)
                                                               // or [frame][516] (S frame-major: whole 4104-byte frames, conflict-free readers)
    float acc[ACC];
    float wss4[256];                                           // window sum of squares of a sample covered by four frames, by src mod hop
};
template <int IF_FR, int NPASS, bool TF>
__global__ __launch_bounds__(256) void istft1024_fused_kernel(const float2* __restrict__ S, int64_t T, int64_t ld,
                                                              const double* __restrict__ window, int64_t start,
                                                              float* __restrict__ y, int64_t out_len) {
    typedef IstftFusedLds<IF_FR, NPASS> LT;
    constexpr int M = 512, F = 513, HOP = 256, NF = 1024, IF_K = LT::K, IF_ACC = LT::ACC;
    constexpr int NPRE = (F * IF_FR + 255) / 256;              // staged values per thread and pass
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LT& L = *reinterpret_cast<LT*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* re = L.ex[wave];
    double* im = L.ex[wave] + 576;
    double wa[8], wb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { wa[r] = window[2 * (lane + 64 * r)] * (1.0 / M); wb[r] = window[2 * (lane + 64 * r) + 1] * (1.0 / M); }
    Fft512 fft;
    fft.init(lane);
    double sr[8], si[8];                                          // exp(+2 pi i k / 1024), k = lane + 64 r
#pragma unroll
    for (int r = 0; r < 8; ++r) sincospi(2.0 * (double)(lane + 64 * r) / 1024.0, &si[r], &sr[r]);
    const int64_t ntot = (int64_t)NF + (int64_t)HOP * (T - 1);
    const int64_t nchunks = (T + IF_K - 1) / IF_K;
    {   // frames in ascending order: window positions m0 + 768, + 512, + 256, + 0; float rounding after every addition (as the generic loop)
        float w4 = 0.f;
#pragma unroll
        for (int f = 3; f >= 0; --f) { const double w = window[tid + f * HOP]; w4 = (float)((double)w4 + w * w); }
        L.wss4[tid] = w4;
    }
    float2 pre[NPRE];
    // staged value idx of a pass -> (bin, frame of the pass): consecutive threads take consecutive frames of a bin when S is
    // [bin][ld] and consecutive bins of a frame when S is [frame][ld]; `slot`: where (bin, frame) lives in L.stage
    auto split = [&](int idx, int& f, int& q) __attribute__((always_inline)) {
        if (TF) { q = idx / F; f = idx - q * F; } else { f = idx / IF_FR; q = idx - f * IF_FR; }
    };
    auto slot = [&](int f, int q) __attribute__((always_inline)) { return TF ? q * 516 + f : f * (IF_FR + 1) + q; };
    auto request = [&](int64_t ts) __attribute__((always_inline)) {   // IF_FR frames starting at ts (frames outside [0, T): zeros)
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int idx = tid + 256 * u;
            int f, q;
            split(idx, f, q);
            const int64_t t = ts + q;
            pre[u] = (idx < F * IF_FR && t >= 0 && t < T) ? (TF ? S[t * ld + f] : S[(int64_t)f * ld + t]) : float2{0.f, 0.f};
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int idx = tid + 256 * u;
            int f, q;
            split(idx, f, q);
            if (idx < F * IF_FR) L.stage[slot(f, q)] = pre[u];
        }
    };
    if ((int64_t)blockIdx.x < nchunks) request((int64_t)blockIdx.x * IF_K - IF_H);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t t0 = c * IF_K, tb = t0 - IF_H;              // first own frame, first computed frame (may be < 0)
        __syncthreads();                                          // the previous chunk's output pass is done with acc
        for (int i = tid; i < IF_ACC; i += 256) L.acc[i] = 0.f;
        for (int pass = 0; pass < NPASS; ++pass) {
            const int64_t ts = tb + (int64_t)pass * IF_FR;     // first frame of this staging pass
            commit();                                             // every reader of `stage` passed the barrier that closed the last round
            __syncthreads();
            // next pass (of this chunk or of this workgroup's next chunk): in flight during the FFT rounds
            if (pass + 1 < NPASS) request(ts + IF_FR);
            else if (c + gridDim.x < nchunks) request((c + gridDim.x) * IF_K - IF_H);
            for (int rr = 0; rr < IF_FR / 4; ++rr) {
                const int q = 4 * rr + wave;
                const int64_t t = ts + q;
                const bool valid = t >= 0 && t < T;               // wave-uniform
                if (valid) {
                    cd v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int k = lane + 64 * r;
                        const float2 a = L.stage[slot(k, q)], b = L.stage[slot(M - k, q)];
                        cd xk = cd{(double)a.x, (double)a.y}, xc = cd{(double)b.x, -(double)b.y};   // X[k], conj(X[M-k])
                        if (k == 0) { xk.y = 0.0; xc.y = 0.0; }                                      // C2R ignores imag of DC / Nyquist
                        const cd e = cd{0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y)};
                        const cd o = cmulc(cd{0.5 * (xk.x - xc.x), 0.5 * (xk.y - xc.y)}, sr[r], si[r]);
                        v[r] = cd{e.x - o.y, -(e.y + o.x)};       // conj(E + i O)
                    }
                    fft.run(v, re, im, lane);
                    __builtin_amdgcn_wave_barrier();              // every lane has read its pass-2 inputs: the buffer becomes the frame
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int i = lane + 64 * r;
                        reinterpret_cast<double2*>(L.ex[wave])[i] = double2{wa[r] * v[r].x, -wb[r] * v[r].y};   // conj, 1/M folded into the window
                    }
                }
                __syncthreads();                                  // the round's four frames are in LDS
                // overlap-add of frames ts + 4 rr .. + 3, in frame order, one float rounding per addition
                const int j0 = pass * IF_FR + 4 * rr;          // index of the round's first frame in the chunk
#pragma unroll
                for (int sidx0 = 0; sidx0 < 3 * HOP + NF; sidx0 += 256) {     // seven independent chains per thread (the float <-> double conversions are slow and dependent)
                    const int sidx = sidx0 + tid;
                    float a = L.acc[j0 * HOP + sidx];
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        const int m = sidx - f * HOP;
                        const int64_t tf = ts + 4 * rr + f;
                        if (m >= 0 && m < NF && tf >= 0 && tf < T) a = (float)((double)a + L.ex[f][m]);
                    }
                    L.acc[j0 * HOP + sidx] = a;
                }
                __syncthreads();                                  // before the next round reuses the exchange buffers (and `stage`, after the last round)
            }
        }
        // output: the samples this chunk completes (the last chunk also owns everything behind its frames)
        const int64_t s_lo = t0 * HOP;
        const bool last = c == nchunks - 1;
        const int64_t s_hi = last ? start + out_len : (t0 + IF_K) * HOP;
        for (int64_t src = s_lo + tid; src < s_hi; src += 256) {
            const int64_t i = src - start;
            if (i < 0 || i >= out_len) continue;
            float a = 0.f, wss = 0.f;
            if (src < ntot) {
                a = L.acc[src - tb * HOP];
                if (src >= NF - HOP && src / HOP <= T - 1) wss = L.wss4[src & (HOP - 1)];   // covered by four frames: the window sum depends on src mod hop only
                else {
                    int64_t tlo = (src - NF + HOP) / HOP;
                    if (src < NF) tlo = 0;
                    int64_t thi = src / HOP;
                    if (thi > T - 1) thi = T - 1;
                    for (int64_t t = tlo; t <= thi; ++t) {
                        const int m = (int)(src - t * HOP);
                        wss = (float)((double)wss + window[m] * window[m]);
                    }
                }
                if (wss > FLT_MIN) a = a / wss;
            }
            y[i] = a;
        }
    }
}

// nfft = 1024, hop = 256, S FRAME-major ([T][ld], row t = frame t): the mirror image of the forward kernel's walk.  A frame is one
// contiguous 4104-byte row, so a wave reads its frame straight into registers (two 512-byte runs per instruction: bins
// lane + 64 r ascending and 512 - lane - 64 r descending) -- no staging through LDS, no workgroup barrier.  Each wave walks
// `chunk` consecutive frames plus the three in front of them and keeps the overlap-add IN REGISTERS: after the inverse FFT lane l
// holds samples 2 l + 128 r + {0, 1} of the frame (r = 0..7), the running float image of the next 1024 output samples lives in
// the same lanes, and advancing one hop (256 samples) is a shift by two registers.  After frame t has been added, samples
// [256 t, 256 t + 256) have received all their frames in frame order with one float rounding per addition -- the arithmetic of
// librosa's `y[...] += ytmp`, of istft_ola_kernel and of the fused kernel above (bit-identical results) -- and leave as 512-byte runs.
// LDS: the FFT exchange buffers only (9 KB per wave).
//
// BATCH (dvae_istft_batch): the walk over a ragged batch of frame-major spectrograms packed row after row; a wave's work item is one
// utterance and a run of at most `chunk` of its frames (its three halo frames are the utterance's own).  GAIN: every bin is scaled by a
// real gain before the transform, re = g xr and im = g xi in float32 (numpy's `WF * X` of a float32 gain and a complex64 spectrogram);
// blockIdx.y selects the gain plane and the output (two Wiener estimates in one launch).
template <bool BATCH = false, bool GAIN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void istft1024_walk_kernel(const float2* __restrict__ S, int64_t T, int64_t ld,
                                                             const double* __restrict__ window, int64_t start,
                                                             float* __restrict__ y, int64_t out_len, int chunk, IstftBatch bt = IstftBatch{}) {
    static_assert(BATCH || !GAIN, "the fused gain exists in the batch walk only");
    constexpr int M = 512, HOP = 256, NF = 1024;
    __shared__ double lre[4][M + 64], lim[4][M + 64];
    // per-bin constants of the whole workgroup in LDS (two waves per SIMD need the kernel under 256 registers):
    // tw[k] = exp(+2 pi i k / 1024); wn[k] = (window[2 k], -window[2 k + 1]) / M  (conj and 1/M folded into the window)
    __shared__ double2 tw[M], wn[M];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform chunk and frame numbers: scalar loop control and addresses
    double* re = lre[wave];
    double* im = lim[wave];
    for (int k = threadIdx.x; k < M; k += 256) {
        double sn, cs;
        sincospi(2.0 * (double)k / 1024.0, &sn, &cs);
        tw[k] = double2{cs, sn};
        wn[k] = double2{window[2 * k] * (1.0 / M), -(window[2 * k + 1] * (1.0 / M))};
    }
    __syncthreads();                                              // the only workgroup barrier
    int64_t c = (int64_t)blockIdx.x * 4 + wave;
    const float* __restrict__ gp = nullptr;
    if constexpr (BATCH) {
        const BatchItem it = batch_item(bt.tab, bt.U, c);
        if (it.u < 0) return;
        const int U = bt.U, u = it.u;
        const int64_t f0 = uni64(bt.tab[U + 1 + u]), Tu = uni64(bt.tab[2 * U + 1 + u]), o0 = uni64(bt.tab[3 * U + 1 + u]);
        const int64_t lu = uni64(bt.tab[4 * U + 1 + u]), gc = uni64(bt.tab[5 * U + 1 + u]);
        // a table the host's checks would have refused: the wave leaves without touching memory (odd output offsets too: the
        // paired stores below are 8-byte aligned)
        if (Tu < 1 || f0 < 0 || f0 + Tu > bt.T_total || o0 < 0 || (o0 & 1) || lu < 0 || o0 + lu > bt.y_total || it.local * chunk >= Tu) return;
        if constexpr (GAIN) {
            if (gc < 0 || gc + Tu > bt.ldg) return;
            gp = (blockIdx.y ? bt.g[1] : bt.g[0]) + gc;
        }
        S += f0 * ld;
        T = Tu;
        y = (GAIN && blockIdx.y ? bt.y1 : y) + o0;
        out_len = lu;
        c = it.local;
    }
    const int64_t nchunks = (T + chunk - 1) / chunk;
    if (c >= nchunks) return;
    Fft512 fft;
    fft.init(lane);
    // window sum of squares of a sample covered by four frames, at the positions this lane emits (p = 2 lane + 128 j + e within the
    // hop): frames in ascending order see window positions p + 768, + 512, + 256, + 0; float rounding after every addition
    float w4[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float w = 0.f;
#pragma unroll
            for (int f = 3; f >= 0; --f) { const double ww = window[2 * lane + 128 * j + e + f * HOP]; w = (float)((double)w + ww * ww); }
            w4[j][e] = w;
        }
    const int64_t ntot = (int64_t)NF + (int64_t)HOP * (T - 1);
    const int64_t t0 = c * chunk;
    const int64_t te = t0 + chunk < T ? t0 + chunk : T;
    const bool last = c == nchunks - 1;
    const int64_t t_emit_end = last ? T + 3 : te;                 // the last chunk also flushes the three hops behind frame T - 1
    float2 ra[8], rb[8], na[8], nb[8];                            // X[k] and X[512 - k] of the current / the next frame
    float ga[GAIN ? 8 : 1], gb[GAIN ? 8 : 1];                     // the gains of X[k], X[512 - k] of the frame in flight
    // the utterance's gain columns through a buffer descriptor (the host keeps a gain plane below 2 GB)
    const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gp), 0, GAIN ? (int)(513 * bt.ldg * 4) : 0, 0x00020000);
    const int vga = GAIN ? (int)(lane * bt.ldg * 4) : 0, vgb = GAIN ? (int)((64 - lane) * bt.ldg * 4) : 0;
    auto fetch = [&](int64_t t, float2 (&a)[8], float2 (&b)[8]) __attribute__((always_inline)) {
        const float2* row = S + t * ld;
#pragma unroll
        for (int r = 0; r < 8; ++r) { a[r] = row[lane + 64 * r]; b[r] = row[M - lane - 64 * r]; }
    };
    auto fetch_gain = [&](int64_t t) __attribute__((always_inline)) {
        if constexpr (GAIN) {
            // bins lane + 64 r and (64 - lane) + 64 (7 - r) = 512 - lane - 64 r: a per-lane byte offset and a wave-uniform one
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                ga[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_g, vga, (int)((64 * r * bt.ldg + t) * 4), 0));
                gb[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_g, vgb, (int)((64 * (7 - r) * bt.ldg + t) * 4), 0));
            }
        }
    };
    // re = g xr, im = g xi in float32 (numpy's product of a float32 gain and a complex64 bin, up to the sign of a zero)
    auto apply_gain = [&](float2 (&a)[8], float2 (&b)[8]) __attribute__((always_inline)) {
        if constexpr (GAIN) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                a[r] = float2{__fmul_rn(ga[r], a[r].x), __fmul_rn(ga[r], a[r].y)};
                b[r] = float2{__fmul_rn(gb[r], b[r].x), __fmul_rn(gb[r], b[r].y)};
            }
        }
    };
    float acc[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) { acc[r][0] = 0.f; acc[r][1] = 0.f; }
    int64_t t = t0 - 3 < 0 ? 0 : t0 - 3;                          // frames in front of the signal do not exist (nothing to add, nothing to emit)
    if (t < T) { fetch(t, ra, rb); fetch_gain(t); apply_gain(ra, rb); }
    for (; t < t_emit_end; ++t) {
        if (t < T) {
            if (t + 1 < te) fetch(t + 1, na, nb);                 // in flight under this frame's transform
            cd v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int k = lane + 64 * r;
                cd xk = cd{(double)ra[r].x, (double)ra[r].y}, xc = cd{(double)rb[r].x, -(double)rb[r].y};   // X[k], conj(X[M-k])
                if (k == 0) { xk.y = 0.0; xc.y = 0.0; }                                                      // C2R ignores imag of DC / Nyquist
                const cd e = cd{0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y)};
                const double2 w = tw[k];
                const cd o = cmulc(cd{0.5 * (xk.x - xc.x), 0.5 * (xk.y - xc.y)}, w.x, w.y);
                v[r] = cd{e.x - o.y, -(e.y + o.x)};               // conj(E + i O)
            }
            fft.run(v, re, im, lane);
            if (t + 1 < te) fetch_gain(t + 1);                    // (after the transform: not live across it)
            __builtin_amdgcn_wave_barrier();                      // the next frame's first exchange writes come after every lane's last reads
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                // windowed frame values (conj, 1/M folded into the window) as the doubles the other kernels store, then one
                // float rounding per addition; __dmul_rn / __dadd_rn: never contracted into an fma
                const double2 w = wn[lane + 64 * r];
                acc[r][0] = (float)__dadd_rn((double)acc[r][0], __dmul_rn(w.x, v[r].x));
                acc[r][1] = (float)__dadd_rn((double)acc[r][1], __dmul_rn(w.y, v[r].y));
            }
            if (t + 1 < te) apply_gain(na, nb);
#pragma unroll
            for (int r = 0; r < 8; ++r) { ra[r] = na[r]; rb[r] = nb[r]; }
        }
        if (t >= t0) {
            // samples [256 t, 256 t + 256) are complete
            const bool inner = t >= 3 && t <= T - 1;              // covered by four frames: the window sum depends on the position in the hop only
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float o[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t src = t * HOP + 2 * lane + 128 * j + e;
                    float a = acc[j][e], wss = 0.f;
                    if (inner) wss = w4[j][e];
                    else {
                        int64_t tlo = (src - NF + HOP) / HOP;
                        if (src < NF) tlo = 0;
                        int64_t thi = src / HOP;
                        if (thi > T - 1) thi = T - 1;
                        for (int64_t tt = tlo; tt <= thi; ++tt) {
                            const int m = (int)(src - tt * HOP);
                            wss = (float)((double)wss + window[m] * window[m]);
                        }
                    }
                    if (wss > FLT_MIN) a = a / wss;
                    o[e] = a;
                }
                const int64_t i = t * HOP + 2 * lane + 128 * j - start;
                if (i >= 0 && i + 1 < out_len && ((start & 1) == 0)) *reinterpret_cast<float2*>(y + i) = float2{o[0], o[1]};
                else {
                    if (i >= 0 && i < out_len) y[i] = o[0];
                    if (i + 1 >= 0 && i + 1 < out_len) y[i + 1] = o[1];
                }
            }
        }
        // advance one hop: two registers down, zeros in behind
#pragma unroll
        for (int r = 0; r < 6; ++r) { acc[r][0] = acc[r + 2][0]; acc[r][1] = acc[r + 2][1]; }
        acc[6][0] = acc[6][1] = acc[7][0] = acc[7][1] = 0.f;
    }
    if (last)                                                      // behind the signal: zeros up to out_len
        for (int64_t src = ntot + lane; src < start + out_len; src += 64)
            if (src >= start) y[src - start] = 0.f;
}

// The same walk in the arithmetic of istft_pytorch (packages/processing/stft.py:154-190: torch.istft of a complex64 tensor with
// torch.hann_window): inverse FFT, window product, overlap-add and the division by the window envelope in float32 (the kernel above
// computes in double whatever the input: the arithmetic of istft(), where librosa transforms with numpy's double FFT).  What the narrower
// type buys: a point is ONE 8-byte LDS slot, packed float32 VALU instead of fp64 (ten minutes of audio: 73 -> 57-61 us; two waves
// per SIMD: stft_types.hpp, ISTFT_F32_OCC).
__global__ __launch_bounds__(256, ISTFT_F32_OCC) void istft1024_walk_f32_kernel(const float2* __restrict__ S, int64_t T, int64_t ld,
                                                                                const float* __restrict__ window, int64_t start,
                                                                                float* __restrict__ y, int64_t out_len, int chunk) {
    constexpr int M = 512, HOP = 256, NF = 1024;
    __shared__ __attribute__((aligned(8))) cf lz[4][M + 64];
    // tw[k] = exp(+2 pi i k / 1024); wn[k] = (window[2 k], -window[2 k + 1]) / M  (conj and 1/M folded into the window: exact scalings)
    __shared__ float2 tw[M], wn[M];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* z = lz[wave];
    for (int k = threadIdx.x; k < M; k += 256) {
        double sn, cs;
        sincospi(2.0 * (double)k / 1024.0, &sn, &cs);
        tw[k] = float2{(float)cs, (float)sn};
        wn[k] = float2{window[2 * k] * (1.0f / M), -(window[2 * k + 1] * (1.0f / M))};
    }
    __syncthreads();                                              // the only workgroup barrier
    const int64_t nchunks = (T + chunk - 1) / chunk;
    const int64_t c = (int64_t)blockIdx.x * 4 + wave;
    if (c >= nchunks) return;
    Fft512F fft;
    fft.init(lane);
    // window envelope of a sample covered by four frames, at the positions this lane emits (frames in ascending order)
    float w4[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float w = 0.f;
#pragma unroll
            for (int f = 3; f >= 0; --f) { const float ww = window[2 * lane + 128 * j + e + f * HOP]; w = fmaf(ww, ww, w); }
            w4[j][e] = w;
        }
    const int64_t ntot = (int64_t)NF + (int64_t)HOP * (T - 1);
    const int64_t t0 = c * chunk;
    const int64_t te = t0 + chunk < T ? t0 + chunk : T;
    const bool last = c == nchunks - 1;
    const int64_t t_emit_end = last ? T + 3 : te;                 // the last chunk also flushes the three hops behind frame T - 1
    float2 ra[8], rb[8], na[8], nb[8];                            // X[k] and X[512 - k] of the current / the next frame
    // one descriptor, two per-lane offsets, the frame's row as the scalar offset, the bin group as the instruction offset (sixteen 64-bit
    // addresses per frame cost 32 registers); the launcher checks T * ld * 8 < 2^31
    const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(S), 0, (int)(T * ld * 8), 0x00020000);
    const int va = lane * 8, vb = (64 - lane) * 8;
    auto fetch = [&](int64_t t, float2 (&a)[8], float2 (&b)[8]) __attribute__((always_inline)) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        const int so = (int)(t * ld * 8);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            a[r] = __builtin_bit_cast(float2, (u2)__builtin_amdgcn_raw_buffer_load_b64(rs_s, va + 512 * r, so, 0));
            b[r] = __builtin_bit_cast(float2, (u2)__builtin_amdgcn_raw_buffer_load_b64(rs_s, vb + 512 * (7 - r), so, 0));
        }
    };
    float acc[8][2];
#pragma unroll
    for (int r = 0; r < 8; ++r) { acc[r][0] = 0.f; acc[r][1] = 0.f; }
    int64_t t = t0 - 3 < 0 ? 0 : t0 - 3;
    if (t < T) fetch(t, ra, rb);
    for (; t < t_emit_end; ++t) {
        if (t < T) {
            if (t + 1 < te) fetch(t + 1, na, nb);                 // in flight under this frame's transform
            cf v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int k = lane + 64 * r;
                cf xk = cf{ra[r].x, ra[r].y}, xc = cf{rb[r].x, -rb[r].y};                        // X[k], conj(X[M-k])
                if (k == 0) { xk.y = 0.f; xc.y = 0.f; }                                           // C2R ignores imag of DC / Nyquist
                const cf e = cf{0.5f * (xk.x + xc.x), 0.5f * (xk.y + xc.y)};
                const float2 w = tw[k];
                const cf o = cmulc(cf{0.5f * (xk.x - xc.x), 0.5f * (xk.y - xc.y)}, w.x, w.y);
                v[r] = cf{e.x - o.y, -(e.y + o.x)};               // conj(E + i O)
            }
            fft.run(v, z, lane);
            __builtin_amdgcn_wave_barrier();                      // the next frame's first exchange writes come after every lane's last reads
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float2 w = wn[lane + 64 * r];
                acc[r][0] = fmaf(w.x, v[r].x, acc[r][0]);
                acc[r][1] = fmaf(w.y, v[r].y, acc[r][1]);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) { ra[r] = na[r]; rb[r] = nb[r]; }
        }
        if (t >= t0) {
            // samples [256 t, 256 t + 256) are complete
            const bool inner = t >= 3 && t <= T - 1;              // covered by four frames: the envelope depends on the position in the hop only
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float o[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t src = t * HOP + 2 * lane + 128 * j + e;
                    float a = acc[j][e], wss = 0.f;
                    if (inner) wss = w4[j][e];
                    else {
                        int64_t tlo = (src - NF + HOP) / HOP;
                        if (src < NF) tlo = 0;
                        int64_t thi = src / HOP;
                        if (thi > T - 1) thi = T - 1;
                        for (int64_t tt = tlo; tt <= thi; ++tt) {
                            const float ww = window[(int)(src - tt * HOP)];
                            wss = fmaf(ww, ww, wss);
                        }
                    }
                    if (wss > 1e-11f) a = a / wss;                // torch.istft: window_envelop.abs() > 1e-11 is asserted over the kept range
                    o[e] = a;
                }
                const int64_t i = t * HOP + 2 * lane + 128 * j - start;
                if (i >= 0 && i + 1 < out_len && ((start & 1) == 0)) *reinterpret_cast<float2*>(y + i) = float2{o[0], o[1]};
                else {
                    if (i >= 0 && i < out_len) y[i] = o[0];
                    if (i + 1 >= 0 && i + 1 < out_len) y[i + 1] = o[1];
                }
            }
        }
        // advance one hop: two registers down, zeros in behind
#pragma unroll
        for (int r = 0; r < 6; ++r) { acc[r][0] = acc[r + 2][0]; acc[r][1] = acc[r + 2][1]; }
        acc[6][0] = acc[6][1] = acc[7][0] = acc[7][1] = 0.f;
    }
    if (last)                                                      // behind the signal: zeros up to out_len
        for (int64_t src = ntot + lane; src < start + out_len; src += 64)
            if (src >= start) y[src - start] = 0.f;
}

// [513][ld] (bin-major rows, the legacy layout) -> [T][513] frame rows for the walk kernel: 64 x 64 tiles through LDS, 512-byte runs both ways
__global__ __launch_bounds__(256) void c64_transpose_kernel(const float2* __restrict__ S, int64_t T, int64_t ld, float2* __restrict__ out) {
    __shared__ float2 tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * 64;
    const int b0 = blockIdx.y * 64;
#pragma unroll 4
    for (int p = 0; p < 16; ++p) {
        const int b = b0 + ty + 4 * p;
        if (b < 513 && t0 + tx < T) tile[ty + 4 * p][tx] = S[(int64_t)b * ld + t0 + tx];
    }
    __syncthreads();
#pragma unroll 4
    for (int p = 0; p < 16; ++p) {
        const int64_t t = t0 + ty + 4 * p;
        if (t < T && b0 + tx < 513) out[t * 513 + b0 + tx] = tile[tx][ty + 4 * p];
    }
}

// frames[t][m] = window[m] * irfft(S[:, t])[m]   (double scratch)
__global__ __launch_bounds__(256) void istft_frames_pow2_kernel(const float* __restrict__ S, int64_t T, int64_t sf, int64_t st,
                                                                 const double* __restrict__ window, int nfft, int logM,
                                                                 double* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = nfft >> 1;
    cd* z = (cd*)smem;
    cd* tw = z + M;
    double* win = (double*)(tw + M);
    stage_tables(tw, win, window, nfft);
    __syncthreads();
    const double scale = 1.0 / (double)M;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        for (int k = threadIdx.x; k <= (M >> 1); k += blockDim.x) {
            cd xk = cd{(double)S[(k * sf + t * st) * 2], (double)S[(k * sf + t * st) * 2 + 1]};
            cd xm = cd{(double)S[((int64_t)(M - k) * sf + t * st) * 2], (double)S[((int64_t)(M - k) * sf + t * st) * 2 + 1]};
            if (k == 0) { xk.y = 0.0; xm.y = 0.0; }              // C2R ignores imag of DC / Nyquist
            const cd xc = cconj(xm);
            const cd e = cd{0.5 * (xk.x + xc.x), 0.5 * (xk.y + xc.y)};
            const cd d = csub(xk, xc);
            const cd o = cmul(cconj(tw[k]), cd{0.5 * d.x, 0.5 * d.y});
            const cd zk = cd{e.x - o.y, e.y + o.x};              // E + i O
            const cd zm = cd{e.x + o.y, -e.y + o.x};             // conj(E) + i conj(O)
            z[__brev((unsigned)k) >> (32 - logM)] = zk;
            if (k != 0 && k != (M >> 1)) z[__brev((unsigned)(M - k)) >> (32 - logM)] = zm;
        }
        __syncthreads();
        fft_lds(z, tw, logM, 1);
        for (int i = threadIdx.x; i < M; i += blockDim.x) {
            const cd v = z[i];
            frames[t * nfft + 2 * i] = win[2 * i] * (v.x * scale);
            frames[t * nfft + 2 * i + 1] = win[2 * i + 1] * (v.y * scale);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void istft_frames_dft_kernel(const float* __restrict__ S, int64_t T, int64_t sf, int64_t st,
                                                                const double* __restrict__ window, int nfft,
                                                                double* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cd* tw = (cd*)smem;                  // exp(+2 pi i k / nfft)
    cd* X = tw + nfft;                   // half spectrum of this frame
    const int F = nfft / 2 + 1;
    for (int k = threadIdx.x; k < nfft; k += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)k / (double)nfft, &s, &c);
        tw[k] = cd{c, s};
    }
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        __syncthreads();
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            cd v = cd{(double)S[(f * sf + t * st) * 2], (double)S[(f * sf + t * st) * 2 + 1]};
            if (f == 0 || (2 * f == nfft)) v.y = 0.0;
            X[f] = v;
        }
        __syncthreads();
        for (int m = threadIdx.x; m < nfft; m += blockDim.x) {
            double acc = X[0].x;
            int idx = 0;
            for (int f = 1; f < F; ++f) {
                idx += m; if (idx >= nfft) idx -= nfft;
                const double term = X[f].x * tw[idx].x - X[f].y * tw[idx].y;
                acc += (2 * f == nfft) ? term : 2.0 * term;
            }
            frames[t * nfft + m] = window[m] * (acc / (double)nfft);
        }
    }
}

// y[i] = sum over frames (float32 accumulation in frame order, as librosa's in-place +=) / wss
__global__ __launch_bounds__(256) void istft_ola_kernel(const double* __restrict__ frames, const double* __restrict__ window,
                                                         int64_t T, int nfft, int hop, int64_t start, float* __restrict__ y, int64_t out_len) {
    const int64_t ntot = (int64_t)nfft + (int64_t)hop * (T - 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < out_len; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = i + start;
        float acc = 0.f, wss = 0.f;
        if (src < ntot) {
            int64_t tlo = (src - nfft + hop) / hop;     // ceil((src - nfft + 1) / hop) for src >= nfft - 1
            if (src < nfft) tlo = 0;
            int64_t thi = src / hop;
            if (thi > T - 1) thi = T - 1;
            for (int64_t t = tlo; t <= thi; ++t) {
                const int m = (int)(src - t * hop);
                acc = (float)((double)acc + frames[t * nfft + m]);
                wss = (float)((double)wss + window[m] * window[m]);
            }
            if (wss > FLT_MIN) acc = acc / wss;
        }
        y[i] = acc;
    }
}

// ---- launchers (declared in stft_types.hpp)

template <int IF_FR, int NPASS, bool TF>
static int launch_istft_fused(const float2* S, int64_t T, int64_t ld, const double* window, int64_t start, float* y, int64_t out_len, hipStream_t s) {
    typedef IstftFusedLds<IF_FR, NPASS> LT;
    static bool attr_done[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (!attr_done[dev]) {
        DVAE_HIP(hipFuncSetAttribute((const void*)(istft1024_fused_kernel<IF_FR, NPASS, TF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LT)));
        attr_done[dev] = true;
    }
    const int64_t nchunks = cdiv(T, LT::K);
    const int per_cu = sizeof(LT) <= 80 * 1024 ? 2 : 1;           // workgroups resident per CU (LDS)
    const int wb = (int)(nchunks < 256 * per_cu ? nchunks : 256 * per_cu);
    hipLaunchKernelGGL((istft1024_fused_kernel<IF_FR, NPASS, TF>), dim3(wb), dim3(256), sizeof(LT), s, S, T, ld, window, start, y, out_len);
    DVAE_LAUNCH_OK("istft1024_fused_kernel");
    return 0;
}

// chunk size by length: enough chunks to cover the CUs first, then wider runs per bin and less halo work (3 of 8 / 16 / 32 frames)
template <bool TF>
static int istft_fused_by_length(const float2* S, int64_t T, int64_t ld, const double* window, int64_t start, float* y, int64_t out_len, hipStream_t s) {
    if (T <= 5 * 512) return launch_istft_fused<8, 1, TF>(S, T, ld, window, start, y, out_len, s);
    if (T <= 13 * 512) return launch_istft_fused<16, 1, TF>(S, T, ld, window, start, y, out_len, s);
    return launch_istft_fused<16, 2, TF>(S, T, ld, window, start, y, out_len, s);
}

int launch_istft1024_fused(const float2* S, int64_t T, int64_t ld, bool tf, const double* window, int64_t start, float* y, int64_t out_len, hipStream_t s) {
    if (tf) {                                                                    // frame-major input through the staged kernel: diagnostic builds (DVAE_ISTFT_STAGED)
#ifdef DVAE_DIAG
        return istft_fused_by_length<true>(S, T, ld, window, start, y, out_len, s);
#else
        set_error("istft: DVAE_ISTFT_STAGED on frame-major input exists in the diagnostic build only (build.py --diag)");
        return DVAE_E_UNSUPPORTED;
#endif
    }
    return istft_fused_by_length<false>(S, T, ld, window, start, y, out_len, s);
}

int launch_istft1024_walk(const float2* S, int64_t T, int64_t ld, const double* window, int64_t start, float* y, int64_t out_len, int chunk, hipStream_t s) {
    const int wb = (int)cdiv(cdiv(T, chunk), 4);
    hipLaunchKernelGGL((istft1024_walk_kernel<false, false>), dim3(wb), dim3(256), 0, s, S, T, ld, window, start, y, out_len, chunk);
    DVAE_LAUNCH_OK("istft1024_walk_kernel");
    return 0;
}

int launch_istft1024_walk_batch(const float2* S, const double* window, int64_t start, float* y, int chunk, int64_t n_items, const IstftBatch& bt, hipStream_t s) {
    if (bt.g[0]) {
        const dim3 grid((unsigned)cdiv(n_items, 4), bt.g[1] ? 2 : 1);
        hipLaunchKernelGGL((istft1024_walk_kernel<true, true>), grid, dim3(256), 0, s, S, bt.T_total, (int64_t)513, window, start, y, bt.y_total, chunk, bt);
    } else {
        hipLaunchKernelGGL((istft1024_walk_kernel<true, false>), dim3((unsigned)cdiv(n_items, 4)), dim3(256), 0, s, S, bt.T_total, (int64_t)513, window,
                           start, y, bt.y_total, chunk, bt);
    }
    DVAE_LAUNCH_OK("istft1024_walk_kernel (batch)");
    return 0;
}

int launch_istft1024_walk_f32(const float2* S, int64_t T, int64_t ld, const float* window, int64_t start, float* y, int64_t out_len, int chunk, hipStream_t s) {
    const int wb = (int)cdiv(cdiv(T, chunk), 4);
    hipLaunchKernelGGL(istft1024_walk_f32_kernel, dim3(wb), dim3(256), 0, s, S, T, ld, window, start, y, out_len, chunk);
    DVAE_LAUNCH_OK("istft1024_walk_f32_kernel");
    return 0;
}

int launch_c64_transpose(const float2* S, int64_t T, int64_t ld, float2* out, hipStream_t s) {
    hipLaunchKernelGGL(c64_transpose_kernel, dim3((unsigned)cdiv(T, 64), 9), dim3(256), 0, s, S, T, ld, out);
    DVAE_LAUNCH_OK("c64_transpose_kernel");
    return 0;
}

// the three forms of frames-to-scratch (the two-pass inverse): one launch check string
int launch_istft1024_frames(const float2* S, int64_t T, int64_t sf, int64_t st, const double* window, double* frames, hipStream_t s) {
    const size_t lds = (size_t)513 * (ISTFT_FR + 1) * sizeof(float2);
    static bool attr_done = false;
    if (!attr_done) {
        DVAE_HIP(hipFuncSetAttribute((const void*)istft1024_frames_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done = true;
    }
    const int wb = (int)(cdiv(T, ISTFT_FR) < 4096 ? cdiv(T, ISTFT_FR) : 4096);
    hipLaunchKernelGGL(istft1024_frames_kernel, dim3(wb), dim3(256), lds, s, S, T, sf, st, window, frames);
    DVAE_LAUNCH_OK("istft_frames");
    return 0;
}

int launch_istft_frames_pow2(const float* S, int64_t T, int64_t sf, int64_t st, const double* window, int nfft, int logM, double* frames, hipStream_t s) {
    const int blocks = (int)(T < 2048 ? T : 2048);
    const size_t lds = (size_t)(nfft / 2) * 2 * sizeof(cd) + (size_t)nfft * sizeof(double);
    hipLaunchKernelGGL(istft_frames_pow2_kernel, dim3(blocks), dim3(256), lds, s, S, T, sf, st, window, nfft, logM, frames);
    DVAE_LAUNCH_OK("istft_frames");
    return 0;
}

int launch_istft_frames_dft(const float* S, int64_t T, int64_t sf, int64_t st, const double* window, int nfft, double* frames, hipStream_t s) {
    const int blocks = (int)(T < 2048 ? T : 2048);
    const size_t lds = (size_t)nfft * sizeof(cd) + (size_t)(nfft / 2 + 1) * sizeof(cd);
    hipLaunchKernelGGL(istft_frames_dft_kernel, dim3(blocks), dim3(256), lds, s, S, T, sf, st, window, nfft, frames);
    DVAE_LAUNCH_OK("istft_frames");
    return 0;
}

int launch_istft_ola(const double* frames, const double* window, int64_t T, int nfft, int hop, int64_t start, float* y, int64_t out_len, hipStream_t s) {
    const int ob = (int)(cdiv(out_len, 256) < 2048 ? cdiv(out_len, 256) : 2048);
    hipLaunchKernelGGL(istft_ola_kernel, dim3(ob), dim3(256), 0, s, frames, window, T, nfft, hop, start, y, out_len);
    DVAE_LAUNCH_OK("istft_ola");
    return 0;
}

}  // namespace dvae

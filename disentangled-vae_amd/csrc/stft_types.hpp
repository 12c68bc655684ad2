// What the host side of the STFT / ISTFT (stft.hip: entries, argument checks, dispatch) shares with the device files (stft_fwd.hip,
// istft.hip: kernels and launchers): the constants the dispatch and the kernels both read, the batch argument block, and the launchers
// the host calls.  No device code here.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace dvae {

constexpr int STFT_FR = 16;        // frames staged per workgroup pass of the complex layout
constexpr int ISTFT_FR = 8;       // frames staged per workgroup pass: 37 KB + 37 KB of exchange buffers = two workgroups per CU
constexpr int64_t ISTFT_TR_MIN_T = 1024;      // shorter spectrograms go through the staged kernel directly (a second launch costs more than it saves)

// waves per SIMD of stft1024_walk_f32_kernel (stft_fwd.hip): 3 (168 registers).  Same box, alternating, ten minutes of float32 audio: complex frames 45.8 / 38.3 / 39.5 us and power
// frames 39.0 / 37.0 / 39.2 us at 4 / 3 / 2 (at 4 the complex form spills 8 registers)
#ifndef STFT_F32_OCC
#define STFT_F32_OCC 3
#endif

// waves per SIMD of istft1024_walk_f32_kernel (istft.hip): two, as the double walk: a round of 2048 waves is two per SIMD whatever the kernel allows, more and shorter chunks transform more halo
// frames and measured slower at every occupancy (profiles/r05_istft_f32_ab.txt; at three waves per SIMD the kernel spills: 72 us; the next
// row by LDS-direct loads instead of 32 registers, spill-free at three and four: 63-75 us at every occupancy -- the walk is bound by its
// VALU / LDS work per transform, not by latency).
#ifndef ISTFT_F32_OCC
#define ISTFT_F32_OCC 2
#endif

// the ragged batch of istft1024_walk_kernel<true, .> (dvae_istft_batch)
struct IstftBatch {
    const int64_t* tab;      // [item prefix (U + 1) | first frame (U) | frames (U) | first output sample (U) | output length (U) | gain column (U)]
    int U;
    int64_t T_total, y_total;
    const float* g[2];       // gain planes, bin-major [513][ldg]: bin k of the utterance's frame t at g[k * ldg + column + t]
    int64_t ldg;
    float* y1;               // the output of gain plane 1
};

// ---- launchers.  Each selects the instantiation, launches and returns 0 or an error code with set_error() called; the launch check
// strings are those of the host entries the launches came from.

// stft_fwd.hip.  x: float64 (in_f64) or float32 samples; layout: 0 complex [F][T], 1 power [T][F], 2 complex [T][F]
// stft1024_walk_kernel, a wave per `chunk` frames: one signal (tab == nullptr; occ3: the three-wave form of the diagnostic build) or the
// ragged batch of n_items work items described by tab (T = frames of the whole batch)
int launch_stft1024_walk(const void* x, int in_f64, int64_t n, const double* window, int64_t T, int chunk, void* out, int layout, bool occ3,
                         const int64_t* tab, int U, int64_t n_items, hipStream_t s);
// stft1024_kernel: layouts 1 / 2 a wave per `chunk` frames, layout 0 staged STFT_FR frames at a time (chunk unused)
int launch_stft1024(const void* x, int in_f64, int64_t n, const double* window, int hop, int64_t T, int chunk, void* out, int layout, hipStream_t s);
// stft_pow2_kernel (nfft = 2 << logM) / stft_dft_kernel (any even nfft): a workgroup per frame
int launch_stft_pow2(const void* x, int in_f64, int64_t n, const double* window, int nfft, int logM, int hop, int64_t T, void* out, int layout, hipStream_t s);
int launch_stft_dft(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop, int64_t T, void* out, int layout, hipStream_t s);
// stft1024_walk_f32_kernel, layouts 1 / 2
int launch_stft1024_walk_f32(const float* x, int64_t n, const float* window, int64_t T, int chunk, void* out, int layout, hipStream_t s);

// istft.hip
// istft1024_fused_kernel, its chunk size chosen by T; tf (S frame-major): diagnostic build only, DVAE_E_UNSUPPORTED in the product build
int launch_istft1024_fused(const float2* S, int64_t T, int64_t ld, bool tf, const double* window, int64_t start, float* y, int64_t out_len, hipStream_t s);
// istft1024_walk_kernel over one frame-major signal / over a ragged batch (gain planes as bt.g says; bt.T_total, bt.y_total: the extents)
int launch_istft1024_walk(const float2* S, int64_t T, int64_t ld, const double* window, int64_t start, float* y, int64_t out_len, int chunk, hipStream_t s);
int launch_istft1024_walk_batch(const float2* S, const double* window, int64_t start, float* y, int chunk, int64_t n_items, const IstftBatch& bt, hipStream_t s);
int launch_istft1024_walk_f32(const float2* S, int64_t T, int64_t ld, const float* window, int64_t start, float* y, int64_t out_len, int chunk, hipStream_t s);
// [513][ld] -> [T][513]
int launch_c64_transpose(const float2* S, int64_t T, int64_t ld, float2* out, hipStream_t s);
// windowed frames to the double scratch (S(bin f, frame t) = S[f * sf + t * st]), then the gather overlap-add
int launch_istft1024_frames(const float2* S, int64_t T, int64_t sf, int64_t st, const double* window, double* frames, hipStream_t s);
int launch_istft_frames_pow2(const float* S, int64_t T, int64_t sf, int64_t st, const double* window, int nfft, int logM, double* frames, hipStream_t s);
int launch_istft_frames_dft(const float* S, int64_t T, int64_t sf, int64_t st, const double* window, int nfft, double* frames, hipStream_t s);
int launch_istft_ola(const double* frames, const double* window, int64_t T, int nfft, int hop, int64_t start, float* y, int64_t out_len, hipStream_t s);

}  // namespace dvae

// Label makers of the training-set builders on the GPU (reference packages/processing/target.py:5-70):
// time-domain VAD (frame energy against the quietest frame) and the ideal binary mask (bins within
// `ibm_threshold` dB of the loudest bin).  Outputs are 0/1 labels and must match the reference bit for bit,
// so every float32 operation of the numpy code is reproduced as "exact value rounded once to float32"
// (double arithmetic, then one rounding): that is what a correctly rounded float32 libm returns.
#include <math.h>
#include "ragged.hpp"

namespace dvae {

// energy[t] = sum_{i < nfft} y[t*hop + i]^2 in double (samples past n count as the zero end-pad)
template <typename T>
__global__ __launch_bounds__(256) void frame_energy_kernel(const T* __restrict__ y, int64_t n, int nfft, int hop, int64_t frames,
                                                           double* __restrict__ energy) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= frames) return;
    const int64_t s0 = t * hop;
    double a = 0.0;
    for (int i = lane; i < nfft; i += 64) {
        const int64_t s = s0 + i;
        const double v = s < n ? (double)y[s] : 0.0;
        a = fma(v, v, a);
    }
    a = wave_sum(a);
    if (lane == 0) energy[t] = a;
}

// one workgroup: min over frames, then vad[t] = energy[t] > factor * min   (target.py:52-54)
__global__ __launch_bounds__(1024) void vad_threshold_kernel(const double* __restrict__ energy, int64_t frames, double factor, float* __restrict__ vad) {
    __shared__ double red[16];
    __shared__ double mn_s;
    double mn = INFINITY;
    for (int64_t t = threadIdx.x; t < frames; t += 1024) mn = fmin(mn, energy[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0];
        for (int w = 1; w < 16; ++w) m = fmin(m, red[w]);
        mn_s = m;
    }
    __syncthreads();
    const double thr = factor * mn_s;
    for (int64_t t = threadIdx.x; t < frames; t += 1024) vad[t] = energy[t] > thr ? 1.f : 0.f;
}

// float32 |S| as numpy computes it (npy_cabsf = hypotf, correctly rounded in current glibc)
__device__ __forceinline__ float mag_f32(float re, float im) {
    return (float)sqrt((double)re * (double)re + (double)im * (double)im);
}
// float32 20 * log10(mag + eps): float32 add, correctly rounded float32 log10, float32 multiply
__device__ __forceinline__ float db_f32(float mag, float eps) {
    const float t = mag + eps;
    return 20.f * (float)log10((double)t);
}

__global__ __launch_bounds__(256) void ibm_max_kernel(const float2* __restrict__ S, int64_t count, float* __restrict__ partial) {
    __shared__ float red[4];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float2 v = S[i];
        m = fmaxf(m, mag_f32(v.x, v.y));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// mask = 20 log10(|S| + eps) > max_db - threshold  (target.py:65-68); log10 is monotone, so max_db comes from the max magnitude
__global__ __launch_bounds__(256) void ibm_mask_kernel(const float2* __restrict__ S, int64_t count, const float* __restrict__ partial, int nparts,
                                                       float eps, float threshold, const float* __restrict__ gate, int64_t gate_cols,
                                                       float* __restrict__ mask) {
    float m = 0.f;
    for (int i = 0; i < nparts; ++i) m = fmaxf(m, partial[i]);       // nparts <= 1024, cached
    const float thr = db_f32(m, eps) - threshold;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float2 v = S[i];
        float o = db_f32(mag_f32(v.x, v.y), eps) > thr ? 1.f : 0.f;
        if (gate) o *= gate[i % gate_cols];                            // noise_robust_clean_speech_IBM: ibm * vad (target.py:103)
        mask[i] = o;
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_vad_workspace_bytes(int64_t frames) { return (size_t)frames * sizeof(double) + 256; }

extern "C" int dvae_vad_labels(const void* y, int in_f64, int64_t n, int nfft, int hop, int64_t frames, double vad_threshold,
                               float* vad, void* workspace, void* stream) {
    DVAE_CHECK_ARG(y && vad && workspace, "vad_labels: null argument");
    DVAE_CHECK_ARG(n > 0 && nfft > 0 && hop > 0 && frames > 0, "vad_labels: bad sizes");
    DVAE_CHECK_ARG((frames - 1) * hop + nfft <= n + hop, "vad_labels: %lld frames need more samples than n + hop = %lld",
                   (long long)frames, (long long)(n + hop));
    hipStream_t s = (hipStream_t)stream;
    double* energy = (double*)workspace;
    const unsigned blocks = (unsigned)cdiv(frames, 4);
    if (in_f64) hipLaunchKernelGGL(frame_energy_kernel<double>, dim3(blocks), dim3(256), 0, s, (const double*)y, n, nfft, hop, frames, energy);
    else hipLaunchKernelGGL(frame_energy_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)y, n, nfft, hop, frames, energy);
    DVAE_LAUNCH_OK("frame_energy_kernel");
    hipLaunchKernelGGL(vad_threshold_kernel, dim3(1), dim3(1024), 0, s, energy, frames, pow(10.0, vad_threshold), vad);
    DVAE_LAUNCH_OK("vad_threshold_kernel");
    return 0;
}

extern "C" size_t dvae_ibm_workspace_bytes(void) { return 1024 * sizeof(float); }

extern "C" int dvae_ibm_labels(const void* S, int64_t rows, int64_t cols, float eps, float ibm_threshold, const float* vad_gate,
                               float* mask, void* workspace, void* stream) {
    DVAE_CHECK_ARG(S && mask && workspace, "ibm_labels: null argument");
    DVAE_CHECK_ARG(rows > 0 && cols > 0, "ibm_labels: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int64_t count = rows * cols;
    const int nparts = (int)(cdiv(count, 256) < 1024 ? cdiv(count, 256) : 1024);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(ibm_max_kernel, dim3(nparts), dim3(256), 0, s, (const float2*)S, count, partial);
    DVAE_LAUNCH_OK("ibm_max_kernel");
    const unsigned blocks = (unsigned)(cdiv(count, 256) < 65536 ? cdiv(count, 256) : 65536);
    hipLaunchKernelGGL(ibm_mask_kernel, dim3(blocks), dim3(256), 0, s, (const float2*)S, count, partial, nparts, eps, ibm_threshold, vad_gate, cols, mask);
    DVAE_LAUNCH_OK("ibm_mask_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Ragged batches (dvae_peak_normalise_batch, dvae_vad_labels_batch, dvae_ibm_labels_batch): U utterances packed end to end, each
// kernel one wave per work item (one utterance and a run of at most `chunk` of its samples / frames / bins, found by batch_item).
// Every reduction is a max or a min, exact in any order, so "partials per item, then each wave combines its utterance's partials"
// gives the single-signal kernels' extrema without atomics; the per-element arithmetic is theirs, operation for operation.  Every
// table entry is checked against the scalar extents before memory is touched: a bad entry drops that utterance's work.

namespace dvae {

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_fmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// tab = [items (U + 1) | x0 (U) | len (U)]: utterance u is x[x0[u] : x0[u] + len[u]]
__device__ __forceinline__ ItemRange peak_item(const int64_t* __restrict__ tab, int U, int64_t n, int64_t n_items, int chunk, int64_t& x0) {
    const int64_t item = wave_item();
    const BatchItem it = batch_item(tab, U, item);
    if (it.u < 0) return ItemRange{-1, 0, 0, 0, 0, false};
    x0 = uni64(tab[U + 1 + it.u]);
    const int64_t len = uni64(tab[2 * U + 1 + it.u]);
    ItemRange r = item_range(tab, U, n_items, item, len, chunk, it);
    r.ok = r.ok && x0 >= 0 && len <= n - x0;
    return r;
}

// pass 1: partial[item] = max |x| over the item's samples
__global__ __launch_bounds__(256) void peak_partial_kernel(const double* __restrict__ x, int64_t n, int U, const int64_t* __restrict__ tab,
                                                           int64_t n_items, int chunk, double* __restrict__ partial) {
    int64_t x0 = 0;
    const ItemRange r = peak_item(tab, U, n, n_items, chunk, x0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double m = 0.0;
#pragma unroll 4
    for (int64_t s = r.lo + lane; s < r.hi; s += 64) m = max_nan(m, fabs(x[x0 + s]));
    m = wave_max_nan(m);
    if (lane == 0) partial[(int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = m;
}

// pass 2: peak = max of the utterance's partials (written once per utterance), x /= peak in IEEE double division: numpy's
// `speech / np.max(np.abs(speech))` bit for bit
__global__ __launch_bounds__(256) void peak_divide_kernel(double* __restrict__ x, int64_t n, int U, const int64_t* __restrict__ tab,
                                                          int64_t n_items, int chunk, const double* __restrict__ partial, double* __restrict__ peak) {
    int64_t x0 = 0;
    const ItemRange r = peak_item(tab, U, n, n_items, chunk, x0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double m = 0.0;
    for (int64_t p = r.p0 + lane; p < r.p1; p += 64) m = max_nan(m, partial[p]);
    m = wave_max_nan(m);
    if (r.lo == 0 && lane == 0) peak[r.u] = m;
#pragma unroll 4
    for (int64_t s = r.lo + lane; s < r.hi; s += 64) x[x0 + s] = x[x0 + s] / m;
}

// tab = [items (U + 1) | x0 (U) | n (U) | frame_off (U + 1)]: utterance u's samples are y[x0[u] : x0[u] + n[u]] (zero past n[u], as
// frame_energy_kernel), its frames are vad[frame_off[u] : frame_off[u + 1]]
__device__ __forceinline__ ItemRange vad_item(const int64_t* __restrict__ tab, int U, int64_t n, int nfft, int hop, int64_t n_items, int chunk,
                                              int64_t T_total, int64_t& x0, int64_t& nu, int64_t& f0) {
    const int64_t item = wave_item();
    const BatchItem it = batch_item(tab, U, item);
    if (it.u < 0) return ItemRange{-1, 0, 0, 0, 0, false};
    x0 = uni64(tab[U + 1 + it.u]);
    nu = uni64(tab[2 * U + 1 + it.u]);
    f0 = uni64(tab[3 * U + 1 + it.u]);
    const int64_t Tu = uni64(tab[3 * U + 2 + it.u]) - f0;
    ItemRange r = item_range(tab, U, n_items, item, Tu, chunk, it);
    r.ok = r.ok && x0 >= 0 && nu >= 1 && nu <= n - x0 && f0 >= 0 && Tu <= T_total - f0 && (Tu - 1) * hop + nfft <= nu + hop;
    return r;
}

// pass 1: energy[t] of each frame in frame_energy_kernel's summation order (lane-strided fma, then wave_sum); partial[item] = min
template <typename T>
__global__ __launch_bounds__(256) void vad_energy_batch_kernel(const T* __restrict__ y, int64_t n, int nfft, int hop, int U,
                                                               const int64_t* __restrict__ tab, int64_t n_items, int chunk, int64_t T_total,
                                                               double* __restrict__ energy, double* __restrict__ partial) {
    int64_t x0 = 0, nu = 0, f0 = 0;
    const ItemRange r = vad_item(tab, U, n, nfft, hop, n_items, chunk, T_total, x0, nu, f0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    const T* yu = y + x0;
    double mn = INFINITY;
    for (int64_t t = r.lo; t < r.hi; ++t) {
        const int64_t s0 = t * hop;
        double a = 0.0;
        for (int i = lane; i < nfft; i += 64) {
            const int64_t s = s0 + i;
            const double v = s < nu ? (double)yu[s] : 0.0;
            a = fma(v, v, a);
        }
        a = wave_sum(a);
        if (lane == 0) energy[f0 + t] = a;
        mn = fmin(mn, a);
    }
    if (lane == 0) partial[(int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = mn;
}

// pass 2: vad[t] = energy[t] > factor * (min over the utterance), as vad_threshold_kernel
__global__ __launch_bounds__(256) void vad_threshold_batch_kernel(const double* __restrict__ energy, int64_t n, int nfft, int hop, int U,
                                                                  const int64_t* __restrict__ tab, int64_t n_items, int chunk, int64_t T_total,
                                                                  double factor, const double* __restrict__ partial, float* __restrict__ vad) {
    int64_t x0 = 0, nu = 0, f0 = 0;
    const ItemRange r = vad_item(tab, U, n, nfft, hop, n_items, chunk, T_total, x0, nu, f0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double mn = INFINITY;
    for (int64_t p = r.p0 + lane; p < r.p1; p += 64) mn = fmin(mn, partial[p]);
    const double thr = factor * wave_min(mn);
    for (int64_t t = r.lo + lane; t < r.hi; t += 64) vad[f0 + t] = energy[f0 + t] > thr ? 1.f : 0.f;
}

// tab = [items (U + 1) | e0 (U) | count (U) | cols (U) | g0 (U)]: utterance u is S[e0[u] : e0[u] + count[u]], a row-major (count / cols,
// cols) matrix; with a gate, element i of it is multiplied by gate[g0[u] + i % cols[u]]
__device__ __forceinline__ ItemRange ibm_item(const int64_t* __restrict__ tab, int U, int64_t n, int64_t n_items, int chunk, bool gated,
                                              int64_t n_gate, int64_t& e0, int64_t& cols, int64_t& g0) {
    const int64_t item = wave_item();
    const BatchItem it = batch_item(tab, U, item);
    if (it.u < 0) return ItemRange{-1, 0, 0, 0, 0, false};
    e0 = uni64(tab[U + 1 + it.u]);
    const int64_t count = uni64(tab[2 * U + 1 + it.u]);
    cols = uni64(tab[3 * U + 1 + it.u]);
    g0 = uni64(tab[4 * U + 1 + it.u]);
    ItemRange r = item_range(tab, U, n_items, item, count, chunk, it);
    r.ok = r.ok && e0 >= 0 && count <= n - e0 && cols >= 1 && count % cols == 0 && (!gated || (g0 >= 0 && cols <= n_gate - g0));
    return r;
}

// pass 1: partial[item] = max mag_f32 over the item's bins (ibm_max_kernel's)
__global__ __launch_bounds__(256) void ibm_max_batch_kernel(const float2* __restrict__ S, int64_t n, int U, const int64_t* __restrict__ tab,
                                                            int64_t n_items, int chunk, int64_t n_gate, const float* __restrict__ gate,
                                                            float* __restrict__ partial) {
    int64_t e0 = 0, cols = 1, g0 = 0;
    const ItemRange r = ibm_item(tab, U, n, n_items, chunk, gate != nullptr, n_gate, e0, cols, g0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    float m = 0.f;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
        const float2 v = S[e0 + i];
        m = fmaxf(m, mag_f32(v.x, v.y));
    }
    m = wave_fmax(m);
    if (lane == 0) partial[(int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = m;
}

// pass 2: the mask of ibm_mask_kernel against the utterance's own maximum
__global__ __launch_bounds__(256) void ibm_mask_batch_kernel(const float2* __restrict__ S, int64_t n, int U, const int64_t* __restrict__ tab,
                                                             int64_t n_items, int chunk, const float* __restrict__ partial, float eps, float threshold,
                                                             const float* __restrict__ gate, int64_t n_gate, float* __restrict__ mask) {
    int64_t e0 = 0, cols = 1, g0 = 0;
    const ItemRange r = ibm_item(tab, U, n, n_items, chunk, gate != nullptr, n_gate, e0, cols, g0);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    float m = 0.f;
    for (int64_t p = r.p0 + lane; p < r.p1; p += 64) m = fmaxf(m, partial[p]);
    const float thr = db_f32(wave_fmax(m), eps) - threshold;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
        const float2 v = S[e0 + i];
        float o = db_f32(mag_f32(v.x, v.y), eps) > thr ? 1.f : 0.f;
        if (gate) o *= gate[g0 + i % cols];
        mask[e0 + i] = o;
    }
}

}  // namespace dvae

extern "C" size_t dvae_peak_normalise_workspace_bytes(int64_t n_items) { return (size_t)(n_items > 0 ? n_items : 1) * sizeof(double); }

extern "C" int dvae_peak_normalise_batch(double* x, int64_t n, int U, const int64_t* tables, int64_t n_items, int chunk, double* peak,
                                         void* workspace, void* stream) {
    DVAE_CHECK_ARG(x && peak && workspace && n > 0, "peak_normalise_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && chunk > 0, "peak_normalise_batch: bad table (U %d, %lld items, chunk %d)", U,
                   (long long)n_items, chunk);
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const dim3 grid((unsigned)cdiv(n_items, 4));
    hipLaunchKernelGGL(peak_partial_kernel, grid, dim3(256), 0, s, (const double*)x, n, U, tables, n_items, chunk, partial);
    DVAE_LAUNCH_OK("peak_partial_kernel");
    hipLaunchKernelGGL(peak_divide_kernel, grid, dim3(256), 0, s, x, n, U, tables, n_items, chunk, (const double*)partial, peak);
    DVAE_LAUNCH_OK("peak_divide_kernel");
    return 0;
}

extern "C" size_t dvae_vad_batch_workspace_bytes(int64_t T_total, int64_t n_items) {
    return (size_t)((T_total > 0 ? T_total : 1) + (n_items > 0 ? n_items : 1)) * sizeof(double);
}

extern "C" int dvae_vad_labels_batch(const void* y, int in_f64, int64_t n, int nfft, int hop, double vad_threshold, int U, const int64_t* tables,
                                     int64_t n_items, int chunk, int64_t T_total, float* vad, void* workspace, void* stream) {
    DVAE_CHECK_ARG(y && vad && workspace && n > 0 && nfft > 0 && hop > 0 && T_total > 0, "vad_labels_batch: bad argument");
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && chunk > 0 && n_items <= T_total, "vad_labels_batch: bad table (U %d, %lld items, chunk %d)", U,
                   (long long)n_items, chunk);
    hipStream_t s = (hipStream_t)stream;
    double* energy = (double*)workspace;
    double* partial = energy + T_total;
    const dim3 grid((unsigned)cdiv(n_items, 4));
    if (in_f64) hipLaunchKernelGGL(vad_energy_batch_kernel<double>, grid, dim3(256), 0, s, (const double*)y, n, nfft, hop, U, tables, n_items, chunk,
                                   T_total, energy, partial);
    else hipLaunchKernelGGL(vad_energy_batch_kernel<float>, grid, dim3(256), 0, s, (const float*)y, n, nfft, hop, U, tables, n_items, chunk, T_total,
                            energy, partial);
    DVAE_LAUNCH_OK("vad_energy_batch_kernel");
    hipLaunchKernelGGL(vad_threshold_batch_kernel, grid, dim3(256), 0, s, (const double*)energy, n, nfft, hop, U, tables, n_items, chunk, T_total,
                       pow(10.0, vad_threshold), (const double*)partial, vad);
    DVAE_LAUNCH_OK("vad_threshold_batch_kernel");
    return 0;
}

extern "C" size_t dvae_ibm_batch_workspace_bytes(int64_t n_items) { return (size_t)(n_items > 0 ? n_items : 1) * sizeof(float); }

extern "C" int dvae_ibm_labels_batch(const void* S, int64_t n, float eps, float ibm_threshold, int U, const int64_t* tables, int64_t n_items, int chunk,
                                     const float* vad_gate, int64_t n_gate, float* mask, void* workspace, void* stream) {
    DVAE_CHECK_ARG(S && mask && workspace && n > 0, "ibm_labels_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(!vad_gate || n_gate > 0, "ibm_labels_batch: a gate needs its extent");
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && chunk > 0, "ibm_labels_batch: bad table (U %d, %lld items, chunk %d)", U, (long long)n_items, chunk);
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const dim3 grid((unsigned)cdiv(n_items, 4));
    hipLaunchKernelGGL(ibm_max_batch_kernel, grid, dim3(256), 0, s, (const float2*)S, n, U, tables, n_items, chunk, n_gate, vad_gate, partial);
    DVAE_LAUNCH_OK("ibm_max_batch_kernel");
    hipLaunchKernelGGL(ibm_mask_batch_kernel, grid, dim3(256), 0, s, (const float2*)S, n, U, tables, n_items, chunk, (const float*)partial, eps,
                       ibm_threshold, vad_gate, n_gate, mask);
    DVAE_LAUNCH_OK("ibm_mask_batch_kernel");
    return 0;
}

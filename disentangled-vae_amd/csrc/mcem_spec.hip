// McemBatch's |X|^2 from a packed batch of spectrograms on the device (disentangled-vae_amd/mcem.py: McemBatch.init_parameters, the
// reference's `np.abs(X) ** 2`, packages/models/mcem.py:200, 364).  The input is what dvae_stft_batch writes in layout 2: frame-major
// complex64 rows [sum T_u][513], utterance after utterance; the output is McemBatch's bin-major X2 [513][ntot], utterance u in the
// columns from col[u].  A 64 x 64 tile (frames x bins) is squared on the way in and leaves transposed through LDS: 256-byte runs both ways.
//
// The magnitude is numpy's for complex64, squared in float32 (spec_power.hpp, shared with classify.hip): bit-identical to
// `(np.abs(X) ** 2).astype(np.float32)`.
//
// Beside it the start of the NMF factors for the same layout (dvae_mcem_nmf_start, below): clamps and Vb = W H for all utterances.
#include "common.hpp"
#include "spec_power.hpp"
#include "../../include/dvae_mcem.h"

namespace dvae {

// tab = [frame prefix (U + 1) | first column (U)], int64
__global__ __launch_bounds__(256) void mcem_spec_init_kernel(const float2* __restrict__ S, int64_t T_total, int U, const int64_t* __restrict__ tab,
                                                             float* __restrict__ X2, int64_t ntot) {
    constexpr int F = 513;
    __shared__ float tile[64][65];
    __shared__ int64_t col[64];
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int b0 = blockIdx.y * 64;
    if (threadIdx.x < 64) {
        const int64_t r = r0 + threadIdx.x;
        int64_t c = -1;
        if (r < T_total && U > 0 && tab[0] <= r && r < tab[U]) {
            int lo = 0, hi = U;                                    // tab[lo] <= r < tab[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tab[mid] <= r) lo = mid; else hi = mid;
            }
            const int64_t f0 = tab[lo], f1 = tab[lo + 1], c0 = tab[U + 1 + lo];
            // a table the host's checks would have refused: the frame is dropped, nothing is written for it
            if (f1 <= T_total && c0 >= 0 && c0 + (f1 - f0) <= ntot) c = c0 + (r - f0);
        }
        col[threadIdx.x] = c;
    }
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int rr = i >> 6, bb = i & 63;
        const int64_t r = r0 + rr;
        const int b = b0 + bb;
        float p = 0.f;
        if (r < T_total && b < F) {
            const float2 v = S[r * F + b];
            const float a = np_abs_c64(v.x, v.y);
            p = __fmul_rn(a, a);
        }
        tile[rr][bb] = p;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int bb = i >> 6, rr = i & 63;
        const int b = b0 + bb;
        const int64_t c = col[rr];
        if (b < F && c >= 0) X2[(int64_t)b * ntot + c] = tile[rr][bb];
    }
}

// The NMF factors' start for all utterances in one launch (McemBatch.init_parameters(fused_start=True); the reference's mcem.py:42-52).
// On entry W [U][513][K] and the real columns of H [K][ntot] hold uniform draws; on exit W = max(W, eps), real columns of H = max(H,
// eps), Vb[f][n] = sum_k W[u(n)][f][k] H[k][n] as ONE fma chain from 0 with k ascending, and the pad columns (in no utterance's range)
// of H and Vb are 1.  tab as above.  A workgroup is 64 columns x 64 bins, thread -> column (tid & 63), bins (tid >> 6) + 4 i.  Every
// reader of a draw clamps it itself, so the thread that stores the clamped value back (W: the utterance's first column; H: the first
// bin tile) can do so while others still read: they see the draw or its clamp, and take the same maximum.  The utterance index comes
// from a search that stays inside the table's entries, so whatever the table holds, nothing outside W, H and Vb is touched.
constexpr int NMF_KMAX = 16;

__global__ __launch_bounds__(256) void mcem_nmf_start_kernel(float* __restrict__ W, float* __restrict__ H, float* __restrict__ Vb, int64_t ntot, int K, int U,
                                                             const int64_t* __restrict__ tab, float eps) {
    constexpr int F = 513;
    const int q = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (n >= ntot) return;
    int a = 0, b = U;                                              // col[a] <= n < col[b]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (tab[U + 1 + mid] <= n) a = mid; else b = mid;
    }
    const int64_t d = n - tab[U + 1 + a], cnt = tab[a + 1] - tab[a];
    const bool real = d >= 0 && d < cnt;
    float hk[NMF_KMAX];
#pragma unroll
    for (int k = 0; k < NMF_KMAX; ++k) hk[k] = (k < K && real) ? fmaxf(H[(int64_t)k * ntot + n], eps) : 1.f;
    if (blockIdx.y == 0) {
#pragma unroll
        for (int k = 0; k < NMF_KMAX; ++k)
            if (k < K && (k & 3) == q) H[(int64_t)k * ntot + n] = hk[k];
    }
    for (int i = 0; i < 16; ++i) {
        const int f = blockIdx.y * 64 + q + 4 * i;
        if (f >= F) break;
        float s = 1.f;
        if (real) {
            float* w = W + ((int64_t)a * F + f) * K;
            s = 0.f;
#pragma unroll
            for (int k = 0; k < NMF_KMAX; ++k) {
                if (k < K) {
                    const float wk = fmaxf(w[k], eps);
                    s = __fmaf_rn(wk, hk[k], s);
                    if (d == 0) w[k] = wk;
                }
            }
        }
        Vb[(int64_t)f * ntot + n] = s;
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" int dvae_mcem_spec_init(const void* S, int64_t T_total, int U, const int64_t* tables, float* X2, int64_t ntot, void* stream) {
    DVAE_CHECK_ARG(S && tables && X2 && T_total > 0 && U > 0 && ntot > 0, "mcem_spec_init: bad argument");
    DVAE_CHECK_ARG(T_total <= ntot, "mcem_spec_init: %lld frames do not fit in %lld columns", (long long)T_total, (long long)ntot);
    DVAE_CHECK_ARG(cdiv(T_total, 64) < ((int64_t)1 << 31), "mcem_spec_init: %lld frames", (long long)T_total);
    hipLaunchKernelGGL(mcem_spec_init_kernel, dim3((unsigned)cdiv(T_total, 64), 9), dim3(256), 0, (hipStream_t)stream, (const float2*)S, T_total, U,
                       tables, X2, ntot);
    DVAE_LAUNCH_OK("mcem_spec_init_kernel");
    return 0;
}

extern "C" int dvae_mcem_nmf_start(float* W, float* H, float* Vb, int64_t ntot, int K, int U, const int64_t* tables, float eps, void* stream) {
    DVAE_CHECK_ARG(W && H && Vb && tables, "mcem_nmf_start: null pointer");
    DVAE_CHECK_ARG(ntot > 0 && U > 0 && K > 0 && K <= NMF_KMAX, "mcem_nmf_start: need ntot > 0, U > 0, 0 < K <= %d", NMF_KMAX);
    DVAE_CHECK_ARG(cdiv(ntot, 64) < ((int64_t)1 << 31), "mcem_nmf_start: %lld columns", (long long)ntot);
    hipLaunchKernelGGL(mcem_nmf_start_kernel, dim3((unsigned)cdiv(ntot, 64), 9), dim3(256), 0, (hipStream_t)stream, W, H, Vb, ntot, K, U, tables, eps);
    DVAE_LAUNCH_OK("mcem_nmf_start_kernel");
    return 0;
}

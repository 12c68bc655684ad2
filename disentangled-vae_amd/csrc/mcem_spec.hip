// McemBatch's |X|^2 from a packed batch of spectrograms on the device (disentangled-vae_amd/mcem.py: McemBatch.init_parameters, the
// reference's `np.abs(X) ** 2`, packages/models/mcem.py:200, 364).  The input is what dvae_stft_batch writes in layout 2: frame-major
// complex64 rows [sum T_u][513], utterance after utterance; the output is McemBatch's bin-major X2 [513][ntot], utterance u in the
// columns from col[u].  A 64 x 64 tile (frames x bins) is squared on the way in and leaves transposed through LDS: 256-byte runs both ways.
//
// The magnitude is numpy's for complex64, squared in float32 (spec_power.hpp, shared with classify.hip): bit-identical to
// `(np.abs(X) ** 2).astype(np.float32)`.
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

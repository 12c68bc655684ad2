// Per-bin mean and standard deviation of a frame store on the device (include/dvae.h: dvae_frame_stats; disentangled-vae_amd/frames.py:
// frame_stats, DeviceFrames.stats): the X_train_mean / X_train_std of scripts/create_train_set.py:123-219, for the std_norm switch of the
// train scripts.  One pass over the frames, HBM-bound.
//
//   * partial kernel: workgroup c owns chunk c = frames [c C, (c + 1) C) of the store or of the index table, C = DVAE_FRAME_STATS_CHUNK
//     whatever the grid.  Wave w takes the chunk's frames w, w + 4, ... ascending; lane l holds bins l, l + 64, ..., l + 448 and lane 0
//     bin 512 too, so every load instruction of a wave reads 256 contiguous bytes of one frame.  Four frames (36 loads) are requested
//     before the first addition.  Every bin has its own double accumulators s += x and q += x x (the square of a float32 is exact in
//     double), added in frame order; then the four waves in wave order through LDS.  No atomics on floating-point data: the same (X, rows)
//     give the same partials, and an index table gives the partials of the gathered copy.
//   * finalising kernel: one thread a bin adds the partials in chunk order and forms mean and std in double.
// An index outside [0, n_store) is never dereferenced: it is counted in *bad_count (an integer atomic) and left out of both sums and of n.
#include <math.h>
#include "common.hpp"

namespace dvae {

constexpr int FS_C = DVAE_FRAME_STATS_CHUNK;
constexpr int FS_BINS = 513, FS_G = 8;            // 8 groups of 64 bins and bin 512
constexpr int FS_U = 4;                           // frames of a wave in flight

struct FrameStatsArgs {
    const float* X; int64_t ld, n_store;
    const int64_t* rows; int64_t n;               // n: frames of the store (rows null) or entries of the index table
    double* partials;                             // [chunks][2][513]
    long long* counts;                            // [chunks] frames that entered the sums
    int* bad;
};

__global__ __launch_bounds__(256) void frame_stats_partial_kernel(const FrameStatsArgs g) {
    __shared__ double red[3][2][FS_BINS];         // waves 1..3
    __shared__ int wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * FS_C;
    const int cnt = (int)(g.n - f0 < FS_C ? g.n - f0 : FS_C);
    double s[FS_G + 1], q[FS_G + 1];
#pragma unroll
    for (int b = 0; b <= FS_G; ++b) s[b] = q[b] = 0.0;
    int valid = 0;
    for (int i = wave; i < cnt; i += 4 * FS_U) {
        // every load is issued, whatever the frame: one past the chunk or refused reads row 0 (always there) and its values are
        // dropped, so no load waits behind a branch and all 36 are in flight before the first addition
        bool ok[FS_U];
        const float* p[FS_U];
        int64_t ri[FS_U];
#pragma unroll
        for (int u = 0; u < FS_U; ++u) {
            const int fi = i + 4 * u;
            ok[u] = fi < cnt;                     // (wave-uniform)
            ri[u] = f0 + (ok[u] ? fi : 0);
        }
        if (g.rows) {
#pragma unroll
            for (int u = 0; u < FS_U; ++u) ri[u] = g.rows[ri[u]];
        }
#pragma unroll
        for (int u = 0; u < FS_U; ++u) {
            int64_t r = ri[u];
            if (r < 0 || r >= g.n_store) {        // (only under a table)
                if (ok[u] && lane == 0 && g.bad) atomicAdd(g.bad, 1);
                ok[u] = false;
                r = 0;
            }
            p[u] = g.X + r * g.ld;
        }
        float v[FS_U][FS_G + 1];
#pragma unroll
        for (int u = 0; u < FS_U; ++u) {
#pragma unroll
            for (int b = 0; b < FS_G; ++b) v[u][b] = p[u][64 * b + lane];
            v[u][FS_G] = p[u][512];
        }
#pragma unroll
        for (int u = 0; u < FS_U; ++u) {          // frame order; a frame left out adds +0
            if (ok[u]) ++valid;
#pragma unroll
            for (int b = 0; b <= FS_G; ++b) {
                const double x = (ok[u] && (b < FS_G || lane == 0)) ? (double)v[u][b] : 0.0;
                s[b] += x;
                q[b] = fma(x, x, q[b]);           // x x is exact in double: one rounding, that of the sum
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int b = 0; b < FS_G; ++b) { red[wave - 1][0][64 * b + lane] = s[b]; red[wave - 1][1][64 * b + lane] = q[b]; }
        if (lane == 0) { red[wave - 1][0][512] = s[FS_G]; red[wave - 1][1][512] = q[FS_G]; }
    }
    if (lane == 0) wcount[wave] = valid;
    __syncthreads();
    if (wave == 0) {
        double* ps = g.partials + (int64_t)blockIdx.x * 2 * FS_BINS;
        double* pq = ps + FS_BINS;
#pragma unroll
        for (int b = 0; b <= FS_G; ++b) {
            const int bin = 64 * b + lane;
            if (b == FS_G && lane != 0) continue;
            ps[bin] = ((s[b] + red[0][0][bin]) + red[1][0][bin]) + red[2][0][bin];       // waves in order
            pq[bin] = ((q[b] + red[0][1][bin]) + red[1][1][bin]) + red[2][1][bin];
        }
        if (lane == 0) g.counts[blockIdx.x] = (long long)wcount[0] + wcount[1] + wcount[2] + wcount[3];
    }
}

// mean = s / n; std = sqrt((q - n mean^2) / (n - 1)), every operation a rounded double operation of its own (no contraction); a difference
// that rounding made negative gives 0.  Fewer than two valid frames (possible only under an index table): NaN for both.
__global__ __launch_bounds__(64) void frame_stats_final_kernel(const double* __restrict__ partials, const long long* __restrict__ counts,
                                                               int64_t chunks, float* __restrict__ mean, float* __restrict__ std) {
    const int bin = blockIdx.x * 64 + threadIdx.x;
    if (bin >= FS_BINS) return;
    double s = 0.0, q = 0.0;
    long long n = 0;
    for (int64_t c0 = 0; c0 < chunks; c0 += 8) {  // chunk order; eight chunks requested before their additions (past the end: the last one again, dropped)
        double ps[8], pq[8];
        long long pn[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t c = c0 + j < chunks ? c0 + j : chunks - 1;
            ps[j] = partials[c * 2 * FS_BINS + bin];
            pq[j] = partials[c * 2 * FS_BINS + FS_BINS + bin];
            pn[j] = counts[c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < chunks) { s += ps[j]; q += pq[j]; n += pn[j]; }
    }
    if (n < 2) {
        mean[bin] = std[bin] = __builtin_nanf("");
        return;
    }
    const double nd = (double)n;
    const double m = __ddiv_rn(s, nd);
    const double d = __dsub_rn(q, __dmul_rn(nd, __dmul_rn(m, m)));
    const double var = __ddiv_rn(d, nd - 1.0);
    mean[bin] = (float)m;
    std[bin] = (float)(var < 0.0 ? 0.0 : __dsqrt_rn(var));
}

static int64_t fs_chunks(int64_t n) { return (n + FS_C - 1) / FS_C; }

}  // namespace dvae

using namespace dvae;

extern "C" int dvae_frame_stats_chunk(void) { return FS_C; }

extern "C" size_t dvae_frame_stats_workspace_bytes(int64_t n) {
    if (n < 1 || n >= ((int64_t)1 << 40)) return 0;
    return (size_t)fs_chunks(n) * (2 * FS_BINS * sizeof(double) + sizeof(long long));
}

extern "C" int dvae_frame_stats(const float* X, int64_t ld, int64_t n_store, const int64_t* rows, int64_t n_rows, float* mean, float* std,
                                int* bad_count, void* workspace, void* stream) {
    DVAE_CHECK_ARG(X && mean && std && workspace, "frame_stats: null pointer");
    DVAE_CHECK_ARG(ld >= FS_BINS && ld < ((int64_t)1 << 20), "frame_stats: leading dimension %lld (rows of at least 513 floats)", (long long)ld);
    DVAE_CHECK_ARG(n_store >= 1 && n_store < ((int64_t)1 << 40), "frame_stats: a store of %lld frames", (long long)n_store);
    const int64_t n = rows ? n_rows : n_store;
    DVAE_CHECK_ARG(n >= 2 && n < ((int64_t)1 << 40), "frame_stats: %lld frames (the standard deviation divides by n - 1: at least 2)", (long long)n);
    DVAE_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "frame_stats: the workspace must be 8-byte aligned");
    const int64_t chunks = fs_chunks(n);
    DVAE_CHECK_ARG(chunks < ((int64_t)1 << 31), "frame_stats: %lld chunks", (long long)chunks);
    FrameStatsArgs g;
    g.X = X; g.ld = ld; g.n_store = n_store; g.rows = rows; g.n = n;
    g.partials = (double*)workspace;
    g.counts = (long long*)(g.partials + chunks * 2 * FS_BINS);
    g.bad = bad_count;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_stats_partial_kernel, dim3((unsigned)chunks), dim3(256), 0, s, g);
    DVAE_LAUNCH_OK("frame_stats_partial_kernel");
    hipLaunchKernelGGL(frame_stats_final_kernel, dim3((FS_BINS + 63) / 64), dim3(64), 0, s, (const double*)g.partials,
                       (const long long*)g.counts, chunks, mean, std);
    DVAE_LAUNCH_OK("frame_stats_final_kernel");
    return 0;
}

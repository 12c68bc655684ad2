// Rational polyphase resampling of a ragged batch of signals (dvae_resample_batch): what the reference's
// packages/dataset/qut_database.py:63-83 asks of librosa per recording -- 48 kHz or 44.1 kHz noise down to 16 kHz -- for U signals in
// one launch.  The arithmetic is that of es_resample_kernel (estoi.hip), written out in include/dvae.h: output k = p sum_t h[j0 + t p]
// x[src0 + t], j0 = (L - k q) mod p, src0 = (k q + j0 - L) / p, the sum in double from 0.0 with t ascending, one fma per tap, times
// (double)p at the end.  The order is fixed, so the tiling below changes no bit.
//
// A work item is one signal and a FIXED run of its outputs (rs_plan: a function of p, q and L alone), found by batch_item; one wave
// per item, four per workgroup.  The wave copies the input span of its run, ceil((run - 1) q / p) + 1 + nt samples (nt = 2 L / p + 1
// taps per output at most), zero outside the signal, once into its own quarter of the workgroup's LDS as doubles, and every tap then
// reads LDS: global memory is read once per input sample plus the halo of nt per run, not once per tap.  No workgroup barrier: a
// wave's LDS traffic is in order, and no wave reads another's quarter.
//
// The taps arrive phase-major, [p][nt]: row j0 holds h[j0], h[j0 + p], ... (zeros past the row's own count).  Two ways to walk them:
//   uniform   p <= 16 and a span of 64 p outputs fits the tile: the run is a multiple of 64 p, and the wave takes one phase at a
//             time, lane l the outputs k0 + (64 s + l) p + phase.  The row is the same in every lane (scalar loads); the lanes read
//             LDS at a stride of q samples.
//   per lane  any other p (44.1 kHz -> 16 kHz: p = 160, 31 947 taps): one phase at a time would need 64 q input samples per pass.
//             Lane l takes output k0 + 64 s + l, whatever its phase, and walks its own row of the table (vector loads, 250 KB that
//             every wave shares: L2); the lanes read LDS at a stride of q / p samples.
// The LDS image is padded by one double per 32 when q is even: at a stride of q doubles the 32 lanes of a half wave would otherwise
// share 32 / gcd(q, 32) of the 32 eight-byte bank pairs (q = 8: 8-way), with the pad every lane has its own; an odd q is conflict-free
// as it is.  1280 doubles per wave = 40 KiB per workgroup: four workgroups, 16 waves, per CU.
//
// Every table entry is rechecked against the scalar extents before memory is touched; a bad entry drops that signal's work.
#include "ragged.hpp"

namespace dvae {

constexpr int kRsSpan = DVAE_RESAMPLE_SPAN;          // samples of a run's input span that the tile holds
constexpr int kRsLds = 1280;                         // doubles per wave: kRsSpan and its padding
constexpr int kRsMaxRun = DVAE_RESAMPLE_MAX_RUN;
constexpr int kRsUniformP = 16;
constexpr int64_t kRsMaxLen = (int64_t)1 << 31;
static_assert(kRsSpan - 1 + ((kRsSpan - 1) >> 5) < kRsLds, "the padded span must fit the wave's LDS");

struct RsArgs {
    int64_t n_x, n_y, stride;
    int x_f64, y_f64;
    int U;
    const int64_t* tab;                              // [items (U + 1) | x0 (U) | len (U) | y0 (U)]
    int64_t n_items;
    int p, q, L, nt, run;                            // nt: the row length of the phase-major taps [p][nt]
};

// The run of outputs per work item and the way the taps are walked, from the ratio and the filter alone.  run = 0: the span of 64
// outputs and their taps does not fit the tile.
struct RsPlan { int run; bool uniform; };
static inline RsPlan rs_plan(int p, int q, int L) {
    const int64_t nt = 2 * (int64_t)L / p + 1, room = kRsSpan - nt - 1;
    if (room < 1) return RsPlan{0, false};
    const int64_t rmax = room * p / q + 1;           // the longest run with ceil((run - 1) q / p) + 1 + nt <= kRsSpan
    const bool uniform = p <= kRsUniformP && 64 * (int64_t)p <= rmax;
    const int64_t unit = uniform ? 64 * p : 64;
    if (rmax < unit) return RsPlan{0, false};
    const int64_t most = rmax < kRsMaxRun ? rmax : kRsMaxRun;
    return RsPlan{(int)(unit * (most / unit > 1 ? most / unit : 1)), uniform};
}

// acc += sum_{t < nt} row[t] xs[li + t], t ascending, one fma per tap: eight taps and eight samples are fetched before their eight
// fmas, so that the loads of a block are in flight together
__device__ __forceinline__ double rs_dot(const double* __restrict__ row, const double* xs, int li, int nt, int padmask) {
    double acc = 0.0;
    int t = 0;
    for (; t + 8 <= nt; t += 8) {
        double h[8], v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = row[t + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = li + t + j;
            v[j] = xs[i + ((i >> 5) & padmask)];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fma(h[j], v[j], acc);
    }
    for (; t < nt; ++t) {
        const int i = li + t;
        acc = fma(row[t], xs[i + ((i >> 5) & padmask)], acc);
    }
    return acc;
}

template <bool Uniform>
__global__ __launch_bounds__(256) void rs_resample_kernel(RsArgs a, const void* __restrict__ x, const double* __restrict__ taps,
                                                          void* __restrict__ y) {
    __shared__ double lds[4][kRsLds];
    const int64_t item = wave_item();
    if (item >= a.n_items) return;
    const BatchItem it = batch_item(a.tab, a.U, item);
    if (it.u < 0) return;
    const int U = a.U, p = a.p, q = a.q, L = a.L;
    const int64_t x0 = uni64(a.tab[U + 1 + it.u]), len = uni64(a.tab[2 * U + 1 + it.u]), y0 = uni64(a.tab[3 * U + 1 + it.u]);
    if (len < 1 || len > kRsMaxLen) return;
    const int64_t nout = (len * p + q - 1) / q;
    const ItemRange r = item_range(a.tab, U, a.n_items, item, nout, a.run, it);
    if (!r.ok) return;
    if (x0 < 0 || x0 >= a.n_x || len - 1 > (a.n_x - 1 - x0) / a.stride) return;       // the last sample is x0 + (len - 1) stride
    if (y0 < 0 || nout > a.n_y - y0) return;
    // the span: samples [span0, span0 + spanlen) cover every tap of outputs [r.lo, r.hi)
    const int64_t k0 = r.lo, num = k0 * q - L;
    const int64_t span0 = num >= 0 ? (num + p - 1) / p : -((-num) / p);               // ceil((k0 q - L) / p) = src0 of output k0
    const int spanlen = (int)(((r.hi - 1 - k0) * q + p - 1) / p) + 1 + a.nt;
    if (spanlen > kRsSpan) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double* xs = lds[wave];
    const int padmask = (q & 1) ? 0 : -1;
    for (int i = lane; i < spanlen; i += 64) {
        const int64_t g = span0 + i;
        xs[i + ((i >> 5) & padmask)] = g >= 0 && g < len ? load_f64(x, a.x_f64, x0 + g * a.stride) : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    // A lane whose output lies past r.hi (in the item's last 64 only) computes and stores nothing it keeps: its LDS indices stay
    // inside the span of the whole run, which fits the tile, whatever was staged there.
    const double scale = (double)p;
    if (Uniform) {
        for (int ph = 0; ph < p; ++ph) {
            // k0 is a multiple of p (the run is one of 64 p), so every k below is = ph (mod p): one phase, one row in every lane
            const int j0 = (int)((((int64_t)L - (int64_t)ph * q) % p + p) % p);
            const int nt = j0 <= 2 * L ? (2 * L - j0) / p + 1 : 0;
            const double* __restrict__ row = taps + (int64_t)j0 * a.nt;
            // src0 of output k0 + ph, less span0 (exact: the numerator is a multiple of p); p outputs on, src0 is q samples on
            int li = (int)(((k0 + ph) * q + j0 - L) / p - span0) + lane * q;
            for (int64_t k = k0 + ph + (int64_t)lane * p; k - (int64_t)lane * p < r.hi; k += (int64_t)64 * p, li += 64 * q) {
                const double acc = rs_dot(row, xs, li, nt, padmask);
                if (k < r.hi) store_f64(y, a.y_f64, y0 + k, scale * acc);
            }
        }
    } else {
        // lane l takes outputs k0 + l, k0 + l + 64, ...: 64 outputs on, j0 falls by 64 q mod p (plus p when it wraps) and src0 rises
        // by (64 q + j0' - j0) / p, which is floor(64 q / p), one more on a wrap
        const int step = (64 * q) / p, fall = (64 * q) % p;
        int64_t k = k0 + lane;
        int j0 = (int)((((int64_t)L - k * q) % p + p) % p);
        int li = (int)((k * q + j0 - L) / p - span0);
        for (; k - lane < r.hi; k += 64) {
            const int nt = j0 <= 2 * L ? (2 * L - j0) / p + 1 : 0;
            const double acc = rs_dot(taps + (int64_t)j0 * a.nt, xs, li, nt, padmask);
            if (k < r.hi) store_f64(y, a.y_f64, y0 + k, scale * acc);
            j0 -= fall;
            li += step;
            if (j0 < 0) {
                j0 += p;
                li += 1;
            }
        }
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" int dvae_resample_run(int p, int q, int L) {
    if (p < 1 || q < 1 || p == q || L < 1 || p > (1 << 15) || q > (1 << 15) || L > (1 << 24)) return 0;
    return rs_plan(p, q, L).run;
}

extern "C" int dvae_resample_batch(const void* x, int64_t n_x, int x_f64, int64_t stride, void* y, int64_t n_y, int y_f64, int U,
                                   const int64_t* tables, int64_t n_items, const double* taps, int p, int q, int L, void* stream) {
    DVAE_CHECK_ARG(x && y && taps && n_x > 0 && n_y > 0, "resample_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(x != y, "resample_batch: the output must not be the input");
    DVAE_CHECK_ARG(stride >= 1 && stride <= (1 << 20), "resample_batch: stride %lld: 1 ... 2^20 is required", (long long)stride);
    DVAE_CHECK_ARG(p >= 1 && q >= 1 && p != q && L >= 1 && p <= (1 << 15) && q <= (1 << 15) && L <= (1 << 24),
                   "resample_batch: taps need p != q >= 1 and L >= 1 (got p %d, q %d, L %d)", p, q, L);
    const RsPlan plan = rs_plan(p, q, L);
    DVAE_CHECK_ARG(plan.run > 0, "resample_batch: 64 outputs at %d / %d with %d taps each need more than the %d input samples a tile holds",
                   p, q, 2 * L / p + 1, kRsSpan);
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && n_items >= U, "resample_batch: bad table (U %d, %lld items)", U, (long long)n_items);
    const RsArgs a{n_x, n_y, stride, x_f64 != 0, y_f64 != 0, U, tables, n_items, p, q, L, 2 * L / p + 1, plan.run};
    const dim3 grid((unsigned)cdiv(n_items, 4));
    if (plan.uniform)
        hipLaunchKernelGGL(rs_resample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, x, taps, y);
    else
        hipLaunchKernelGGL(rs_resample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, x, taps, y);
    DVAE_LAUNCH_OK("rs_resample_kernel");
    return 0;
}

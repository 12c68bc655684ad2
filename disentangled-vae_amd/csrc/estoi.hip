// Intelligibility scores of a ragged batch of utterances (dvae_estoi_batch): STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016)
// as include/dvae.h writes them out (and tests/estoi_ref.py restates them in numpy), for U utterances in six launches whatever U is.
// Double arithmetic throughout; a float32 sample converts to double exactly.
//
// A work item is one utterance and a FIXED run of its work, found by batch_item in one of the table's three item prefixes; one wave
// per item.  The data-dependent counts (kept frames K, spectral frames M, segments) are known on the device only, so the items are
// laid over their upper bounds (J frames, J - 30 segments) and a wave past the real count has nothing to do.
//   1 resample  item = 256 p outputs of x and y.  Output k = p sum_t h[j0 + t p] x[src0 + t], j0 = (L - k q) mod p, src0 = (k q + j0 -
//               L) / p: a lane takes outputs of ONE phase at a time (k = base + (64 s + lane) p + phase), so the taps are wave-uniform
//               (scalar loads); the sum runs over t ascending, one fma per tap, from 0.0, and is multiplied by p at the end.
//   2 energy    item = 16 frames of x: lane l squares w[4l .. 4l + 3] x[...] (fma, ascending), wave_sum, 20 log10(sqrt + EPS).
//   3 mask      one wave per utterance: the maximum (exact in any order), keep = (max - 40) - e < 0 as the reference rounds it, the
//               kept frames' indices in order by ballot / popcount, K.
//   4 tob       item = 16 spectral frames.  Sample i of the silence-removed signal is the sum of at most two kept windowed frames (a
//               two-term sum has no order), so the overlap-add is formed on the fly from the kept list: no compacted signal is
//               stored.  Per frame and signal: 256 windowed points packed into a 256-point complex FFT (upper half zero), four
//               radix-4 Stockham passes with 4 points per lane in registers, lanes exchanging through the wave's private padded LDS
//               buffer (no workgroup barrier), the real-FFT split for bins lane + 64 r, power, band sums in ascending bin order, sqrt.
//   5 segment   item = 8 segments, two at a time (one per 32-lane half, lane = frame of the segment, the 15 bands of both signals in
//               registers): row statistics by 5-level butterflies inside the half (the same value in every lane of it), column
//               statistics in the lane.  One partial per item, the segments' terms added in segment order.
//   6 finish    one wave per utterance adds the partials in item order and divides; info = {resampled length, K, segments}.
// No atomics; every reduction has a fixed order, so an utterance's score has the same bits in every run and every batch.
// Every table entry is rechecked against the scalar extents before memory is touched (es_utterance, by every kernel): a bad entry
// drops that utterance's work and the finish writes NaN (info -1).
#include <math.h>
#include "fft_wave.hpp"
#include "ragged.hpp"

namespace dvae {

constexpr int kEsFrame = 256, kEsHop = 128, kEsBands = DVAE_ESTOI_BANDS, kEsSeg = 30, kEsBins = 256;      // bins 0 ... 255 are formed (the bands end at 219)
constexpr int kEsResRun = DVAE_ESTOI_RES_RUN, kEsFrameRun = DVAE_ESTOI_FRAME_RUN, kEsSegRun = DVAE_ESTOI_SEG_RUN;
constexpr double kEsEps = 0x1p-52, kEsDynRange = 40.0, kEsShort = 1e-5;
constexpr int64_t kEsMaxLen = (int64_t)1 << 31;
constexpr int kEsLds = 256 + 64;                     // one exchange buffer: 256 doubles, one of padding per four

struct EsIn {
    const void* p[2];                                // x (clean), y (processed)
    int64_t count[2];
    int f64[2];
    int U;
    const int64_t* tab;                              // [items_res (U + 1) | items_frame (U + 1) | items_seg (U + 1) | x0 | y0 | len | r0 | f0]
    int64_t n_items[3];
    int64_t n_res, n_frames;                         // extents of the resampled-signal and per-frame workspaces
    const double* taps;                              // [2 L + 1] or null (no resampling)
    int up, down, L;
    const double* window;                            // [256]
    const int64_t* bands;                            // [16]
};

struct EsUtt { int64_t len, off[2], n10, J, r0, f0, i0[3], i1[3]; };

// the two frame-count rules of the contract (tests/estoi_ref.py: frames_silent, frames_spec; metrics.py likewise)
__host__ __device__ __forceinline__ int64_t es_frames_silent(int64_t n) { return n >= kEsFrame ? (n - kEsFrame) / kEsHop + 1 : 0; }
__host__ __device__ __forceinline__ int64_t es_frames_spec(int64_t n) { return n > kEsFrame ? (n - kEsFrame - 1) / kEsHop + 1 : 0; }
__device__ __forceinline__ int64_t es_cdiv1(int64_t a, int64_t b) { const int64_t c = (a + b - 1) / b; return c < 1 ? 1 : c; }
// spectral frames and segments of an utterance with K kept frames
__device__ __forceinline__ int64_t es_spec_frames(int64_t K) { return es_frames_spec(K > 0 ? (K - 1) * kEsHop + kEsFrame : 0); }
__device__ __forceinline__ int64_t es_segments(int64_t M) { return M >= kEsSeg ? M - kEsSeg + 1 : 0; }

__device__ __forceinline__ bool es_utterance(const EsIn& in, int u, EsUtt& r) {
    const int U = in.U;
    const int64_t* t = in.tab + 3 * (U + 1);
    r.off[0] = uni64(t[u]);
    r.off[1] = uni64(t[U + u]);
    r.len = uni64(t[2 * U + u]);
    r.r0 = uni64(t[3 * U + u]);
    r.f0 = uni64(t[4 * U + u]);
    bool ok = r.len >= 1 && r.len <= kEsMaxLen;
    if (!ok) return false;
    r.n10 = (r.len * in.up + in.down - 1) / in.down;
    r.J = es_frames_silent(r.n10);
#pragma unroll
    for (int k = 0; k < 2; ++k) ok = ok && r.off[k] >= 0 && r.len <= in.count[k] - r.off[k];
    ok = ok && r.r0 >= 0 && r.n10 <= in.n_res - r.r0 && r.f0 >= 0 && r.J <= in.n_frames - r.f0;
    const int64_t want[3] = {es_cdiv1(r.n10, (int64_t)kEsResRun * in.up), es_cdiv1(r.J, kEsFrameRun),
                             es_cdiv1(r.J > kEsSeg ? r.J - kEsSeg : 0, kEsSegRun)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.i0[c] = uni64(in.tab[c * (U + 1) + u]);
        r.i1[c] = uni64(in.tab[c * (U + 1) + u + 1]);
        ok = ok && r.i0[c] >= 0 && r.i1[c] <= in.n_items[c] && r.i1[c] - r.i0[c] == want[c];
    }
#pragma unroll
    for (int b = 0; b < kEsBands; ++b) {
        const int64_t lo = uni64(in.bands[b]), hi = uni64(in.bands[b + 1]);
        ok = ok && lo >= 0 && lo <= hi && hi <= kEsBins;
    }
    return ok;
}

// the wave's item of class c -> utterance and local index (u = -1: nothing to do)
__device__ __forceinline__ bool es_item(const EsIn& in, int c, EsUtt& r, int& u, int64_t& local, int64_t& item) {
    item = wave_item();
    if (item >= in.n_items[c]) return false;
    const BatchItem it = batch_item(in.tab + c * (in.U + 1), in.U, item);
    if (it.u < 0) return false;
    u = it.u;
    local = it.local;
    return es_utterance(in, it.u, r);
}

__device__ __forceinline__ double es_half_sum(double v) {        // over the lane's 32-lane half, the same value in every lane of it
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- 1: polyphase resampler ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void es_resample_kernel(EsIn in, double* __restrict__ xr, double* __restrict__ yr) {
    EsUtt r;
    int u;
    int64_t local, item;
    if (!es_item(in, 0, r, u, local, item)) return;
    const int lane = threadIdx.x & 63;
    const int up = in.up, down = in.down, L = in.L;
    const int64_t base = local * ((int64_t)kEsResRun * up);
    if (!in.taps) {                                               // fs == 10 kHz: the samples themselves, as doubles
        for (int s = 0; s < kEsResRun / 64; ++s) {
            const int64_t k = base + s * 64 + lane;
            if (k < r.n10) {
                xr[r.r0 + k] = load_f64(in.p[0], in.f64[0], r.off[0] + k);
                yr[r.r0 + k] = load_f64(in.p[1], in.f64[1], r.off[1] + k);
            }
        }
        return;
    }
    for (int ph = 0; ph < up; ++ph) {
        // base is a multiple of p, so every k below is = ph (mod p): one phase, the same taps in every lane
        const int j0 = (int)((((int64_t)L - (int64_t)ph * down) % up + up) % up);
        const int nt = j0 <= 2 * L ? (2 * L - j0) / up + 1 : 0;
        for (int s = 0; s < kEsResRun / 64; ++s) {
            const int64_t k = base + (int64_t)(s * 64 + lane) * up + ph;
            const int64_t src0 = (k * down + j0 - L) / up;          // exact: the numerator is a multiple of p
            double ax = 0.0, ay = 0.0;
            for (int t = 0; t < nt; ++t) {
                const double h = in.taps[j0 + t * up];
                const int64_t i = src0 + t;
                const bool inside = i >= 0 && i < r.len;
                const double xv = inside ? load_f64(in.p[0], in.f64[0], r.off[0] + i) : 0.0;
                const double yv = inside ? load_f64(in.p[1], in.f64[1], r.off[1] + i) : 0.0;
                ax = fma(h, xv, ax);
                ay = fma(h, yv, ay);
            }
            if (k < r.n10) {
                xr[r.r0 + k] = (double)up * ax;
                yr[r.r0 + k] = (double)up * ay;
            }
        }
    }
}

// ---- 2: frame energies of x ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void es_energy_kernel(EsIn in, const double* __restrict__ xr, double* __restrict__ energy) {
    EsUtt r;
    int u;
    int64_t local, item;
    if (!es_item(in, 1, r, u, local, item)) return;
    const int lane = threadIdx.x & 63;
    double w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = in.window[lane * 4 + c];
    const int64_t j1 = local * kEsFrameRun + kEsFrameRun < r.J ? local * kEsFrameRun + kEsFrameRun : r.J;
    for (int64_t j = local * kEsFrameRun; j < j1; ++j) {
        const double* f = xr + r.r0 + j * kEsHop + lane * 4;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = w[c] * f[c];
            s = fma(v, v, s);
        }
        s = wave_sum(s);
        if (lane == 0) energy[r.f0 + j] = 20.0 * log10(sqrt(s) + kEsEps);       // EPS inside the log: an all-zero frame is finite
    }
}

// ---- 3: mask, kept list, K ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void es_mask_kernel(EsIn in, const double* __restrict__ energy, int64_t* __restrict__ kept,
                                                      int64_t* __restrict__ Kc) {
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= in.U) return;
    EsUtt r;
    if (!es_utterance(in, u, r)) return;
    const int lane = threadIdx.x & 63;
    double mx = -INFINITY;
    for (int64_t j = lane; j < r.J; j += 64) mx = fmax(mx, energy[r.f0 + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    double thr;
    {
#pragma clang fp contract(off)
        thr = mx - kEsDynRange;
    }
    int64_t count = 0;
    for (int64_t b = 0; b < r.J; b += 64) {
        const int64_t j = b + lane;
        const bool keep = j < r.J && (thr - energy[r.f0 + (j < r.J ? j : 0)]) < 0.0;
        const unsigned long long m = __ballot(keep);
        if (keep) kept[r.f0 + count + __popcll(m & ((1ull << lane) - 1ull))] = j;
        count += __popcll(m);
    }
    if (lane == 0) Kc[u] = count;
}

// ---- 4: overlap-add of the kept frames, 256-in-512 real FFT, third-octave bands ----------------------------------------------------
__device__ __forceinline__ int es_pad(int i) { return i + (i >> 2); }

__device__ __forceinline__ void es_dft4(cd (&a)[4]) {             // forward, natural order
    const cd t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]), t2 = cadd(a[1], a[3]), d = csub(a[1], a[3]);
    const cd t3 = cd{d.y, -d.x};                                  // * -i
    a[0] = cadd(t0, t2);
    a[2] = csub(t0, t2);
    a[1] = cadd(t1, t3);
    a[3] = csub(t1, t3);
}

// 256-point complex forward FFT of one wave whose points 128 ... 255 are zero: z0 = point lane, z1 = point lane + 64 in,
// v[r] = Z[lane + 64 r] out; four radix-4 Stockham passes (Ns = 1, 4, 16, 64).
struct EsFft256 {
    double tr[3][3], ti[3][3];                                    // passes Ns = 4, 16, 64: exp(-2 pi i r k / (4 Ns)), k = lane mod Ns, r = 1 .. 3
    __device__ __forceinline__ void init(int lane) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int Ns = 4 << (2 * p);
#pragma unroll
            for (int r = 1; r < 4; ++r) sincospi(-2.0 * (double)(r * (lane & (Ns - 1))) / (double)(4 * Ns), &ti[p][r - 1], &tr[p][r - 1]);
        }
    }
    __device__ __forceinline__ void run(cd z0, cd z1, cd (&v)[4], double* re, double* im, int lane) const {
        // pass Ns = 1 with points 2 and 3 zero: X_r = z0 + (-i)^r z1; outputs to lane * 4 + r
        v[0] = cadd(z0, z1);
        v[1] = cd{z0.x + z1.y, z0.y - z1.x};
        v[2] = csub(z0, z1);
        v[3] = cd{z0.x - z1.y, z0.y + z1.x};
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int i = es_pad(lane * 4 + r); re[i] = v[r].x; im[i] = v[r].y; }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int Ns = 4 << (2 * p);
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int i = es_pad(lane + 64 * r); v[r] = cd{re[i], im[i]}; }
#pragma unroll
            for (int r = 1; r < 4; ++r) v[r] = cmulc(v[r], tr[p][r - 1], ti[p][r - 1]);
            es_dft4(v);
            __builtin_amdgcn_wave_barrier();
            if (p < 2) {
                const int j0 = (lane / Ns) * (4 * Ns) + (lane & (Ns - 1));
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int i = es_pad(j0 + Ns * r); re[i] = v[r].x; im[i] = v[r].y; }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
};

__global__ __launch_bounds__(256) void es_tob_kernel(EsIn in, const double* __restrict__ xr, const double* __restrict__ yr,
                                                     const int64_t* __restrict__ kept, const int64_t* __restrict__ Kc,
                                                     double* __restrict__ tob) {
    __shared__ double lds[4][2][kEsLds];
    EsUtt r;
    int u;
    int64_t local, item;
    if (!es_item(in, 1, r, u, local, item)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double* re = lds[wave][0];
    double* im = lds[wave][1];
    int64_t K = uni64(Kc[u]);
    K = K < 0 ? 0 : (K > r.J ? r.J : K);
    const int64_t M = es_spec_frames(K);
    const int64_t m0 = local * kEsFrameRun, m1 = m0 + kEsFrameRun < M ? m0 + kEsFrameRun : M;
    if (m0 >= m1) return;
    EsFft256 fft;
    fft.init(lane);
    double sr[4], si[4];                                          // split twiddles exp(-2 pi i k / 512), k = lane + 64 r
#pragma unroll
    for (int q = 0; q < 4; ++q) sincospi(-(double)(lane + 64 * q) / 256.0, &si[q], &sr[q]);
    const double w0[2] = {in.window[2 * lane], in.window[2 * lane + 1]}, w1[2] = {in.window[2 * lane + 128], in.window[2 * lane + 129]};
    const int64_t blo = lane < kEsBands ? in.bands[lane] : 0, bhi = lane < kEsBands ? in.bands[lane + 1] : 0;
    for (int64_t m = m0; m < m1; ++m) {
        // the frame covers hop blocks m and m + 1 of the silence-removed signal: kept frames m - 1 (second half), m (both), m + 1 (first half)
        const int64_t ja = m > 0 ? uni64(kept[r.f0 + m - 1]) : -1, jb = uni64(kept[r.f0 + m]), jc = uni64(kept[r.f0 + m + 1]);
        if (ja < -1 || ja >= r.J || jb < 0 || jb >= r.J || jc < 0 || jc >= r.J) continue;
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            const double* src = (sig ? yr : xr) + r.r0 + 2 * lane;
            double v0[2], v1[2];
            {
                // each product and sum rounded on its own, as numpy rounds the arrays of the reference
#pragma clang fp contract(off)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double a = ja >= 0 ? w1[c] * src[ja * kEsHop + 128 + c] : 0.0;
                    const double b = w0[c] * src[jb * kEsHop + c];
                    v0[c] = w0[c] * (a + b);
                    const double d = w1[c] * src[jb * kEsHop + 128 + c];
                    const double e = w0[c] * src[jc * kEsHop + c];
                    v1[c] = w1[c] * (d + e);
                }
            }
            cd v[4];
            fft.run(cd{v0[0], v0[1]}, cd{v1[0], v1[1]}, v, re, im, lane);
            // real-FFT split: X[k] = (Z[k] + conj Z[256 - k]) / 2 + exp(-2 pi i k / 512) (Z[k] - conj Z[256 - k]) / (2 i)
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int i = es_pad(lane + 64 * q); re[i] = v[q].x; im[i] = v[q].y; }
            __builtin_amdgcn_wave_barrier();
            double pw[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = es_pad((256 - (lane + 64 * q)) & 255);
                const cd zc = cd{re[i], -im[i]};
                const cd ev = cd{0.5 * (v[q].x + zc.x), 0.5 * (v[q].y + zc.y)};
                const cd dd = csub(v[q], zc);
                const cd od = cmulc(cd{0.5 * dd.y, -0.5 * dd.x}, sr[q], si[q]);
                const cd X = cadd(ev, od);
                pw[q] = X.x * X.x + X.y * X.y;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; ++q) re[es_pad(lane + 64 * q)] = pw[q];
            __builtin_amdgcn_wave_barrier();
            if (lane < kEsBands) {
                double s = 0.0;
                for (int64_t k = blo; k < bhi; ++k) s += re[es_pad((int)k)];              // es_utterance: 0 <= lo <= hi <= 256
                tob[((int64_t)sig * in.n_frames + r.f0 + m) * kEsBands + lane] = sqrt(s);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ---- 5: segments --------------------------------------------------------------------------------------------------------------------
template <int Cnt>
__device__ __forceinline__ void es_row_normalise(double (&a)[kEsBands], bool act) {          // over the 30 frames (lanes) of each band
#pragma unroll
    for (int j = 0; j < kEsBands; ++j) {
        const double mean = es_half_sum(a[j]) / (double)Cnt;
        a[j] = act ? a[j] - mean : 0.0;
        const double nrm = sqrt(es_half_sum(a[j] * a[j])) + kEsEps;
        a[j] = a[j] / nrm;
    }
}

__device__ __forceinline__ void es_col_normalise(double (&a)[kEsBands]) {                    // over the 15 bands of the lane's frame
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kEsBands; ++j) s += a[j];
    const double mean = s / (double)kEsBands;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kEsBands; ++j) {
        a[j] -= mean;
        q += a[j] * a[j];
    }
    const double nrm = sqrt(q) + kEsEps;
#pragma unroll
    for (int j = 0; j < kEsBands; ++j) a[j] = a[j] / nrm;
}

template <bool Extended>
__global__ __launch_bounds__(256) void es_segment_kernel(EsIn in, const int64_t* __restrict__ Kc, const double* __restrict__ tob,
                                                         double clip, double* __restrict__ part) {
    EsUtt r;
    int u;
    int64_t local, item;
    if (!es_item(in, 2, r, u, local, item)) return;
    const int lane = threadIdx.x & 63, half = lane >> 5, n = lane & 31;
    int64_t K = uni64(Kc[u]);
    K = K < 0 ? 0 : (K > r.J ? r.J : K);
    const int64_t nseg = es_segments(es_spec_frames(K));
    const int64_t s0 = local * kEsSegRun;
    double acc = 0.0;
    for (int it = 0; it < kEsSegRun / 2; ++it) {
        const int64_t sa = s0 + 2 * it;                           // the lower half's segment; the upper half's is sa + 1
        if (sa >= nseg) break;
        const int64_t s = sa + half;
        const bool act = s < nseg && n < kEsSeg;
        double X[kEsBands], Y[kEsBands];
        const double* px = tob + (r.f0 + (act ? s + n : 0)) * kEsBands;
        const double* py = px + in.n_frames * kEsBands;
#pragma unroll
        for (int j = 0; j < kEsBands; ++j) {
            X[j] = act ? px[j] : 0.0;
            Y[j] = act ? py[j] : 0.0;
        }
        double c = 0.0, term;
        if (Extended) {
            es_row_normalise<kEsSeg>(X, act);
            es_row_normalise<kEsSeg>(Y, act);
            es_col_normalise(X);
            es_col_normalise(Y);
#pragma unroll
            for (int j = 0; j < kEsBands; ++j) c += X[j] * Y[j];
            term = es_half_sum(c) / (double)kEsSeg;
        } else {
#pragma unroll
            for (int j = 0; j < kEsBands; ++j) {
                const double nx = sqrt(es_half_sum(X[j] * X[j])), ny = sqrt(es_half_sum(Y[j] * Y[j]));
                const double alpha = nx / (ny + kEsEps);
                Y[j] = fmin(alpha * Y[j], X[j] * clip);
            }
            es_row_normalise<kEsSeg>(X, act);
            es_row_normalise<kEsSeg>(Y, act);
#pragma unroll
            for (int j = 0; j < kEsBands; ++j) c += Y[j] * X[j];
            term = es_half_sum(c) / (double)kEsBands;
        }
        const double lo = __shfl(term, 0, 64), hi = __shfl(term, 32, 64);
        acc += lo;
        if (sa + 1 < nseg) acc += hi;
    }
    if (lane == 0) part[item] = acc;
}

// ---- 6: finish ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void es_finish_kernel(EsIn in, const int64_t* __restrict__ Kc, const double* __restrict__ part,
                                                        double* __restrict__ d, int64_t* __restrict__ info) {
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= in.U) return;
    double out = NAN;
    int64_t inf[3] = {-1, -1, -1};
    EsUtt r;
    if (es_utterance(in, u, r)) {
        int64_t K = uni64(Kc[u]);
        K = K < 0 ? 0 : (K > r.J ? r.J : K);
        const int64_t nseg = es_segments(es_spec_frames(K));
        inf[0] = r.n10;
        inf[1] = K;
        inf[2] = nseg;
        if (nseg == 0) {
            out = kEsShort;
        } else {
            double total = 0.0;
            for (int64_t p = r.i0[2]; p < r.i1[2] && (p - r.i0[2]) * kEsSegRun < nseg; ++p) total += part[p];
            out = total / (double)nseg;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        d[u] = out;
        if (info) {
#pragma unroll
            for (int k = 0; k < 3; ++k) info[(int64_t)u * 3 + k] = inf[k];
        }
    }
}

}  // namespace dvae

using namespace dvae;

static size_t es_round(size_t n) { return (n + 31) & ~(size_t)31; }

extern "C" size_t dvae_estoi_workspace_bytes(int64_t n_res, int64_t n_frames, int64_t n_seg_items, int U) {
    const size_t R = es_round(n_res > 0 ? n_res : 1), F = es_round(n_frames > 0 ? n_frames : 1);
    return (2 * R + F + 2 * F * kEsBands + es_round(n_seg_items > 0 ? n_seg_items : 1) + F + es_round(U > 0 ? U : 1)) * sizeof(double);
}

extern "C" int dvae_estoi_batch(const void* x, int64_t n_x, int x_f64, const void* y, int64_t n_y, int y_f64, int U, const int64_t* tables,
                                int64_t n_res_items, int64_t n_frame_items, int64_t n_seg_items, int64_t n_res, int64_t n_frames,
                                const double* taps, int p, int q, int L, const double* window, const int64_t* bands, int extended,
                                double* d, int64_t* info, double* tob, void* workspace, void* stream) {
    DVAE_CHECK_ARG(x && y && workspace && n_x > 0 && n_y > 0, "estoi_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(d && window && bands, "estoi_batch: the output, the window and the band edges are required");
    DVAE_CHECK_ARG(U > 0 && tables && n_res_items >= U && n_frame_items >= U && n_seg_items >= U && n_res >= U && n_frames >= 0,
                   "estoi_batch: bad table (U %d, %lld / %lld / %lld items)", U, (long long)n_res_items, (long long)n_frame_items,
                   (long long)n_seg_items);
    DVAE_CHECK_ARG(cdiv(n_res_items, 4) < ((int64_t)1 << 31) && cdiv(n_frame_items, 4) < ((int64_t)1 << 31) && cdiv(n_seg_items, 4) < ((int64_t)1 << 31),
                   "estoi_batch: too many work items");
    DVAE_CHECK_ARG(taps ? (p >= 1 && q >= 1 && p != q && L >= 1 && p <= (1 << 15) && q <= (1 << 15) && L <= (1 << 24)) : (p == 1 && q == 1 && L == 0),
                   "estoi_batch: taps need p != q >= 1 and L >= 1; without taps p = q = 1, L = 0 (got p %d, q %d, L %d)", p, q, L);
    EsIn in{{x, y}, {n_x, n_y}, {x_f64 != 0, y_f64 != 0}, U, tables, {n_res_items, n_frame_items, n_seg_items}, n_res, n_frames, taps, p, q, L, window, bands};
    const size_t R = es_round(n_res > 0 ? n_res : 1), F = es_round(n_frames > 0 ? n_frames : 1);
    double* xr = (double*)workspace;
    double* yr = xr + R;
    double* energy = yr + R;
    double* tob_ws = energy + F;
    double* part = tob_ws + 2 * F * kEsBands;
    int64_t* kept = (int64_t*)(part + es_round(n_seg_items));
    int64_t* Kc = kept + F;
    // the debug output has the rows of the caller's n_frames, the workspace copy those of the rounded count: the kernels index by
    // in.n_frames, so the workspace copy simply leaves its tail unused
    double* tb = tob ? tob : tob_ws;
    const hipStream_t s = (hipStream_t)stream;
    const double clip = 1.0 + pow(10.0, 15.0 / 20.0);             // 1 + 10^(-BETA / 20), BETA = -15
    hipLaunchKernelGGL(es_resample_kernel, dim3((unsigned)cdiv(n_res_items, 4)), dim3(256), 0, s, in, xr, yr);
    DVAE_LAUNCH_OK("es_resample_kernel");
    hipLaunchKernelGGL(es_energy_kernel, dim3((unsigned)cdiv(n_frame_items, 4)), dim3(256), 0, s, in, (const double*)xr, energy);
    DVAE_LAUNCH_OK("es_energy_kernel");
    hipLaunchKernelGGL(es_mask_kernel, dim3((unsigned)cdiv(U, 4)), dim3(256), 0, s, in, (const double*)energy, kept, Kc);
    DVAE_LAUNCH_OK("es_mask_kernel");
    hipLaunchKernelGGL(es_tob_kernel, dim3((unsigned)cdiv(n_frame_items, 4)), dim3(256), 0, s, in, (const double*)xr, (const double*)yr,
                       (const int64_t*)kept, (const int64_t*)Kc, tb);
    DVAE_LAUNCH_OK("es_tob_kernel");
    if (extended)
        hipLaunchKernelGGL(es_segment_kernel<true>, dim3((unsigned)cdiv(n_seg_items, 4)), dim3(256), 0, s, in, (const int64_t*)Kc, (const double*)tb, clip, part);
    else
        hipLaunchKernelGGL(es_segment_kernel<false>, dim3((unsigned)cdiv(n_seg_items, 4)), dim3(256), 0, s, in, (const int64_t*)Kc, (const double*)tb, clip, part);
    DVAE_LAUNCH_OK("es_segment_kernel");
    hipLaunchKernelGGL(es_finish_kernel, dim3((unsigned)cdiv(U, 4)), dim3(256), 0, s, in, (const int64_t*)Kc, (const double*)part, d, info);
    DVAE_LAUNCH_OK("es_finish_kernel");
    return 0;
}

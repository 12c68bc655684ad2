// Scale-invariant energy ratios of a ragged batch of waveforms (dvae_si_ratios_batch): SI-SDR, SI-SIR and SI-SAR of the reference's
// packages/metrics.py:12-82 (si_sdr_components, energy_ratios, si_sdr_leroux) for U utterances in three launches.  All accumulation
// is in double (the reference works on the float64 arrays soundfile returns; a float32 sample converts to double exactly).
//
// A work item is one utterance and a run of at most DVAE_SI_CHUNK (4096) of its samples, found by batch_item; one wave per item.
//   pass 1  per item: sum sh s, sum s s, sum sh n, sum n n      (lane-strided fma, then wave_sum: at most 64 fma per lane)
//   pass 2  each wave adds its utterance's pass-1 partials IN ITEM ORDER (a fixed order: the same bits in every wave, every run and
//           every batch the utterance is part of), forms alpha_s = sum sh s / sum s s and alpha_n = sum sh n / sum n n by IEEE
//           division, and sums over its own samples |e_noise + e_art|^2 (= |sh - alpha_s s|^2) and |e_art|^2 = |sh - alpha_s s -
//           alpha_n n|^2.  The residuals are formed per sample with the reference's operations and roundings (metrics.py:27-35,
//           56, 77-80); expanding the squares into the pass-1 sums would cancel (at +50 dB the residual energy is 1e-5 of the
//           terms it would be the difference of).
//   finish  one wave per utterance: the partials in item order again, |s_target|^2 = alpha_s^2 sum s s, |e_noise|^2 = alpha_n^2
//           sum n n, 10 log10 of the three ratios.
// No atomics, no clamping, no epsilon: an all-zero s or n gives NaN and a perfect estimate +inf, as numpy gives the reference.
// Every table entry is rechecked against the scalar extents before memory is touched; a bad entry drops that utterance's work in
// passes 1 and 2 and the finish writes NaN into its rows.
#include <math.h>
#include "ragged.hpp"

namespace dvae {

constexpr int kSiChunk = DVAE_SI_CHUNK;

// the three inputs: sh (estimate), s (clean speech), n (noise; null when absent), each a packed buffer of float32 or float64
struct SiInputs {
    const void* p[3];
    int64_t count[3];
    int f64[3];
};

struct SiItem { int u; int64_t lo, hi, p0, p1, off[3]; bool ok; };

// tab = [items (U + 1) | sh0 (U) | s0 (U) | n0 (U) | len (U)]: utterance u is sh[sh0[u] : sh0[u] + len[u]], s[s0[u] : ...], n[n0[u] : ...]
template <bool HasN>
__device__ __forceinline__ bool si_utterance(const SiInputs& in, const int64_t* __restrict__ tab, int U, int64_t n_items, int u, SiItem& r) {
    const int64_t len = uni64(tab[4 * U + 1 + u]);
    r.u = u;
    r.p0 = uni64(tab[u]);
    r.p1 = uni64(tab[u + 1]);
    bool ok = len >= 1 && r.p0 >= 0 && r.p1 <= n_items && r.p1 - r.p0 == (len + kSiChunk - 1) / kSiChunk;
#pragma unroll
    for (int k = 0; k < (HasN ? 3 : 2); ++k) {
        r.off[k] = uni64(tab[(k + 1) * U + 1 + u]);
        ok = ok && r.off[k] >= 0 && len <= in.count[k] - r.off[k];
    }
    r.lo = 0;
    r.hi = len;
    r.ok = ok;
    return ok;
}

template <bool HasN>
__device__ __forceinline__ SiItem si_item(const SiInputs& in, const int64_t* __restrict__ tab, int U, int64_t n_items, int64_t item) {
    SiItem r{-1, 0, 0, 0, 0, {0, 0, 0}, false};
    const BatchItem it = batch_item(tab, U, item);
    if (it.u < 0 || item >= n_items) return r;
    if (!si_utterance<HasN>(in, tab, U, n_items, it.u, r)) return r;
    const int64_t len = r.hi;
    r.lo = it.local * kSiChunk;
    r.hi = r.lo + kSiChunk < len ? r.lo + kSiChunk : len;
    r.ok = r.lo < len;
    return r;
}

// pass 1: dots[item] = {sum sh s, sum s s, sum sh n, sum n n} over the item's samples
template <bool HasN>
__global__ __launch_bounds__(256) void si_dots_kernel(SiInputs in, int U, const int64_t* __restrict__ tab, int64_t n_items, double* __restrict__ dots) {
    const int64_t item = wave_item();
    const SiItem r = si_item<HasN>(in, tab, U, n_items, item);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double hs = 0.0, ss = 0.0, hn = 0.0, nn = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
        const double h = load_f64(in.p[0], in.f64[0], r.off[0] + i), s = load_f64(in.p[1], in.f64[1], r.off[1] + i);
        hs = fma(h, s, hs);
        ss = fma(s, s, ss);
        if (HasN) {
            const double n = load_f64(in.p[2], in.f64[2], r.off[2] + i);
            hn = fma(h, n, hn);
            nn = fma(n, n, nn);
        }
    }
    hs = wave_sum(hs);
    ss = wave_sum(ss);
    if (HasN) {
        hn = wave_sum(hn);
        nn = wave_sum(nn);
    }
    if (lane == 0) {
        double* d = dots + item * 4;
        d[0] = hs;
        d[1] = ss;
        d[2] = HasN ? hn : NAN;
        d[3] = HasN ? nn : NAN;
    }
}

// the utterance's four sums: its items' partials added one after the other, first item first (every lane the same additions)
__device__ __forceinline__ void si_total_dots(const double* __restrict__ dots, int64_t p0, int64_t p1, double t[4]) {
    t[0] = t[1] = t[2] = t[3] = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += dots[p * 4 + k];
    }
}

// pass 2: res[item] = {sum |e_noise + e_art|^2, sum |e_art|^2} over the item's samples (without n: sum |sh - alpha_s s|^2, NaN)
template <bool HasN>
__global__ __launch_bounds__(256) void si_residuals_kernel(SiInputs in, int U, const int64_t* __restrict__ tab, int64_t n_items,
                                                           const double* __restrict__ dots, double* __restrict__ res) {
    const int64_t item = wave_item();
    const SiItem r = si_item<HasN>(in, tab, U, n_items, item);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double t[4];
    si_total_dots(dots, r.p0, r.p1, t);
    const double alpha_s = t[0] / t[1], alpha_n = HasN ? t[2] / t[3] : 0.0;
    double e1 = 0.0, e2 = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
        const double h = load_f64(in.p[0], in.f64[0], r.off[0] + i), s = load_f64(in.p[1], in.f64[1], r.off[1] + i);
        double d1, d2 = 0.0;
        {
            // every operation rounded on its own, in the reference's order (numpy rounds each array it forms): s_target = alpha_s s,
            // e_art = (sh - s_target) - e_noise, and the SI-SDR denominator e_noise + e_art (metrics.py:27-35, 56); without n it is
            // sh - s_target itself (metrics.py:77-80).  An alpha_n of 0 / 0 therefore reaches all three ratios, as it does there.
#pragma clang fp contract(off)
            const double s_target = alpha_s * s;
            d1 = h - s_target;
            if (HasN) {
                const double e_noise = alpha_n * load_f64(in.p[2], in.f64[2], r.off[2] + i);
                d2 = d1 - e_noise;
                d1 = e_noise + d2;
            }
        }
        e1 = fma(d1, d1, e1);
        if (HasN) e2 = fma(d2, d2, e2);
    }
    e1 = wave_sum(e1);
    if (HasN) e2 = wave_sum(e2);
    if (lane == 0) {
        res[item * 2] = e1;
        res[item * 2 + 1] = HasN ? e2 : NAN;
    }
}

// finish: ratios[u] = {SI-SDR, SI-SIR, SI-SAR} in dB, sums[u] = {sum sh s, sum s s, sum sh n, sum n n, |e_noise + e_art|^2, |e_art|^2,
// |s_target|^2, |e_noise|^2}; NaN rows for an utterance whose table entry is bad (and in the n columns without n)
template <bool HasN>
__global__ __launch_bounds__(256) void si_finish_kernel(SiInputs in, int U, const int64_t* __restrict__ tab, int64_t n_items,
                                                        const double* __restrict__ dots, const double* __restrict__ res,
                                                        double* __restrict__ ratios, double* __restrict__ sums) {
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= U) return;
    double out[8], db[3];
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = NAN;
    db[0] = db[1] = db[2] = NAN;
    SiItem r;
    if (si_utterance<HasN>(in, tab, U, n_items, u, r)) {
        double t[4];
        si_total_dots(dots, r.p0, r.p1, t);
        double e1 = 0.0, e2 = 0.0;
        for (int64_t p = r.p0; p < r.p1; ++p) {
            e1 += res[p * 2];
            e2 += res[p * 2 + 1];
        }
        const double alpha_s = t[0] / t[1];
        const double target = alpha_s * alpha_s * t[1];
        out[0] = t[0];
        out[1] = t[1];
        out[4] = e1;
        out[6] = target;
        db[0] = 10.0 * log10(target / e1);
        if (HasN) {
            const double alpha_n = t[2] / t[3];
            const double noise = alpha_n * alpha_n * t[3];
            out[2] = t[2];
            out[3] = t[3];
            out[5] = e2;
            out[7] = noise;
            db[1] = 10.0 * log10(target / noise);
            db[2] = 10.0 * log10(target / e2);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (ratios) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ratios[(int64_t)u * 3 + k] = db[k];
        }
        if (sums) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sums[(int64_t)u * 8 + k] = out[k];
        }
    }
}

template <bool HasN>
static int si_launch(const SiInputs& in, int U, const int64_t* tab, int64_t n_items, double* ratios, double* sums, double* ws, hipStream_t s) {
    double* dots = ws;
    double* res = ws + n_items * 4;
    const dim3 grid((unsigned)cdiv(n_items, 4));
    hipLaunchKernelGGL(si_dots_kernel<HasN>, grid, dim3(256), 0, s, in, U, tab, n_items, dots);
    DVAE_LAUNCH_OK("si_dots_kernel");
    hipLaunchKernelGGL(si_residuals_kernel<HasN>, grid, dim3(256), 0, s, in, U, tab, n_items, (const double*)dots, res);
    DVAE_LAUNCH_OK("si_residuals_kernel");
    hipLaunchKernelGGL(si_finish_kernel<HasN>, dim3((unsigned)cdiv(U, 4)), dim3(256), 0, s, in, U, tab, n_items, (const double*)dots,
                       (const double*)res, ratios, sums);
    DVAE_LAUNCH_OK("si_finish_kernel");
    return 0;
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_si_ratios_workspace_bytes(int64_t n_items) { return (size_t)(n_items > 0 ? n_items : 1) * 6 * sizeof(double); }

extern "C" int dvae_si_ratios_batch(const void* s_hat, int64_t n_s_hat, int s_hat_f64, const void* s, int64_t n_s, int s_f64, const void* n,
                                    int64_t n_n, int n_f64, int U, const int64_t* tables, int64_t n_items, double* ratios, double* sums,
                                    void* workspace, void* stream) {
    DVAE_CHECK_ARG(s_hat && s && workspace && n_s_hat > 0 && n_s > 0, "si_ratios_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(!n || n_n > 0, "si_ratios_batch: the noise buffer needs its extent");
    DVAE_CHECK_ARG(ratios || sums, "si_ratios_batch: no output asked for");
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && n_items >= U, "si_ratios_batch: bad table (U %d, %lld items)", U, (long long)n_items);
    SiInputs in{{s_hat, s, n}, {n_s_hat, n_s, n ? n_n : 0}, {s_hat_f64 != 0, s_f64 != 0, n_f64 != 0}};
    if (n) return si_launch<true>(in, U, tables, n_items, ratios, sums, (double*)workspace, (hipStream_t)stream);
    return si_launch<false>(in, U, tables, n_items, ratios, sums, (double*)workspace, (hipStream_t)stream);
}

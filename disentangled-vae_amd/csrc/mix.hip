// Noisy mixtures at a target SNR for a ragged batch of utterances (dvae_mix_snr_batch): what the reference's
// scripts/create_test_set.py:95-115 does per utterance -- peak-normalise the speech, scale a noise segment to the target SNR, divide
// speech, noise and mixture by their common peak -- for U utterances in five launches.  All arithmetic is in double (the reference
// works on the float64 arrays soundfile returns; a float32 sample converts to double exactly), every operation rounded on its own in
// the reference's order.
//
// A work item is one utterance and a run of at most DVAE_MIX_CHUNK (4096) of its samples, found by batch_item; one wave per item.
//   pass 1  per item: max |speech|                                           (skipped without normalise_speech)
//   pass 2  p = the max of the utterance's pass-1 partials; per item: sum s^2 with s = speech / p, and sum noise^2
//   pass 3  Ps, Pn = the utterance's pass-2 partials added IN ITEM ORDER (a fixed order: the same bits in every wave, every run and
//           every batch the utterance is part of); k = (Ps factor) / Pn, g = sqrt(k); per item: max(|s|, |g noise|, |s + g noise|)
//   pass 4  norm = the max of the pass-3 partials; writes s / norm, v / norm, (s + v) / norm (the rounded sum divided, not the sum of the
//           two quotients), the zeros of [len, out_extent), and per item the sums of the squares of the first two
//   finish  one wave per utterance: stats = {p, Ps, Pn, k, norm, 10 log10(sum out_speech^2 / sum out_noise^2)}
// A maximum is exact in any order; the sums have a fixed one.  No atomics, no clamping, no epsilon: an all-zero noise segment gives
// NaN outputs (0 inf), an all-zero speech under normalise_speech NaN, and a NaN sample reaches every maximum, as numpy gives the
// reference.  Input ranges may overlap or repeat (they are only read).  Every table entry is rechecked against the scalar extents
// before memory is touched; a bad entry drops that utterance's work in passes 1 to 4 and the finish writes NaN into its stats row.
#include <math.h>
#include "ragged.hpp"

namespace dvae {

constexpr int kMixChunk = DVAE_MIX_CHUNK;

struct MixArgs {
    const void* speech;
    const void* noise;
    int64_t n_speech, n_noise, n_out;
    int speech_f64, noise_f64, out_f64, normalise;
    int U;
    const int64_t* tab;
    int64_t n_items;
    const double* factor;
};

// the workspace: four runs of per-item partials
struct MixWork {
    double* peak;       // [n_items]     max |speech|
    double* power;      // [n_items, 2]  sum s^2, sum noise^2
    double* norm;       // [n_items]     max(|s|, |v|, |s + v|)
    double* out_sq;     // [n_items, 2]  sum out_speech^2, sum out_noise^2
};

struct MixItem { int u; int64_t len, lo, hi, p0, p1, s0, n0, o0, extent; bool ok; };

// tab = [items (U + 1) | speech0 (U) | noise0 (U) | out0 (U) | len (U) | out_extent (U)]
__device__ __forceinline__ bool mix_utterance(const MixArgs& a, int u, MixItem& r) {
    const int U = a.U;
    r.u = u;
    r.p0 = uni64(a.tab[u]);
    r.p1 = uni64(a.tab[u + 1]);
    r.s0 = uni64(a.tab[U + 1 + u]);
    r.n0 = uni64(a.tab[2 * U + 1 + u]);
    r.o0 = uni64(a.tab[3 * U + 1 + u]);
    r.len = uni64(a.tab[4 * U + 1 + u]);
    r.extent = uni64(a.tab[5 * U + 1 + u]);
    r.lo = 0;
    r.hi = r.len;
    r.ok = r.len >= 1 && r.p0 >= 0 && r.p1 <= a.n_items && r.p1 - r.p0 == (r.len + kMixChunk - 1) / kMixChunk &&
           r.s0 >= 0 && r.len <= a.n_speech - r.s0 && r.n0 >= 0 && r.len <= a.n_noise - r.n0 &&
           r.o0 >= 0 && r.extent >= r.len && r.extent <= a.n_out - r.o0;
    return r.ok;
}

__device__ __forceinline__ MixItem mix_item(const MixArgs& a) {
    MixItem r{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, false};
    const int64_t item = wave_item();
    const BatchItem it = batch_item(a.tab, a.U, item);
    if (it.u < 0 || item >= a.n_items) return r;
    if (!mix_utterance(a, it.u, r)) return r;
    r.lo = it.local * kMixChunk;
    r.hi = r.lo + kMixChunk < r.len ? r.lo + kMixChunk : r.len;
    r.ok = r.lo < r.len;
    return r;
}

__device__ __forceinline__ int64_t mix_item_index() { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }

// the maximum of the utterance's partials (exact in any order: lanes stride them)
__device__ __forceinline__ double mix_total_max(const double* __restrict__ partial, const MixItem& r, int lane) {
    double m = 0.0;
    for (int64_t p = r.p0 + lane; p < r.p1; p += 64) m = max_nan(m, partial[p]);
    return wave_max_nan(m);
}

// the utterance's scalars from the partials of the passes before: every wave of the utterance forms the same bits
struct MixScalars { double p, Ps, Pn, k, g; };
__device__ __forceinline__ MixScalars mix_scalars(const MixArgs& a, const MixWork& w, const MixItem& r, int lane, bool with_gain) {
    MixScalars m{1.0, 0.0, 0.0, 0.0, 0.0};
    if (a.normalise) m.p = mix_total_max(w.peak, r, lane);
    if (!with_gain) return m;
    for (int64_t p = r.p0; p < r.p1; ++p) {          // item order, every lane the same additions
        m.Ps += w.power[p * 2];
        m.Pn += w.power[p * 2 + 1];
    }
    {
#pragma clang fp contract(off)
        const double target = m.Ps * a.factor[r.u];  // noise_power_target = speech_power * np.power(10, -snr_dB / 10)
        m.k = target / m.Pn;
        m.g = sqrt(m.k);
    }
    return m;
}

// s = speech / p (create_test_set.py:96; the samples as they are without normalise_speech)
__device__ __forceinline__ double mix_speech(const MixArgs& a, const MixItem& r, int64_t i, double p) {
    const double x = load_f64(a.speech, a.speech_f64, r.s0 + i);
    return a.normalise ? x / p : x;
}

// pass 1: peak[item] = max |speech| over the item's samples
__global__ __launch_bounds__(256) void mix_peak_kernel(MixArgs a, MixWork w) {
    const MixItem r = mix_item(a);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    double m = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) m = max_nan(m, fabs(load_f64(a.speech, a.speech_f64, r.s0 + i)));
    m = wave_max_nan(m);
    if (lane == 0) w.peak[mix_item_index()] = m;
}

// pass 2: power[item] = {sum s^2, sum noise^2} over the item's samples (np.power(x, 2) rounds every square before the sum)
__global__ __launch_bounds__(256) void mix_power_kernel(MixArgs a, MixWork w) {
    const MixItem r = mix_item(a);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    const MixScalars m = mix_scalars(a, w, r, lane, false);
    double ps = 0.0, pn = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
#pragma clang fp contract(off)
        const double s = mix_speech(a, r, i, m.p), n = load_f64(a.noise, a.noise_f64, r.n0 + i);
        ps += s * s;
        pn += n * n;
    }
    ps = wave_sum(ps);
    pn = wave_sum(pn);
    if (lane == 0) {
        w.power[mix_item_index() * 2] = ps;
        w.power[mix_item_index() * 2 + 1] = pn;
    }
}

// pass 3: norm[item] = max(|s|, |v|, |s + v|) over the item's samples, v = noise * g
__global__ __launch_bounds__(256) void mix_norm_kernel(MixArgs a, MixWork w) {
    const MixItem r = mix_item(a);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    const MixScalars m = mix_scalars(a, w, r, lane, true);
    double t = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
#pragma clang fp contract(off)
        const double s = mix_speech(a, r, i, m.p);
        const double v = load_f64(a.noise, a.noise_f64, r.n0 + i) * m.g;
        t = max_nan(max_nan(max_nan(t, fabs(s)), fabs(v)), fabs(s + v));
    }
    t = wave_max_nan(t);
    if (lane == 0) w.norm[mix_item_index()] = t;
}

// pass 4: the three outputs, the zero pad of the utterance's last item, out_sq[item] = {sum out_speech^2, sum out_noise^2}
__global__ __launch_bounds__(256) void mix_write_kernel(MixArgs a, MixWork w, void* __restrict__ out_speech, void* __restrict__ out_noise,
                                                        void* __restrict__ out_mix) {
    const MixItem r = mix_item(a);
    if (!r.ok) return;
    const int lane = threadIdx.x & 63;
    const MixScalars m = mix_scalars(a, w, r, lane, true);
    const double norm = mix_total_max(w.norm, r, lane);
    double qs = 0.0, qn = 0.0;
#pragma unroll 4
    for (int64_t i = r.lo + lane; i < r.hi; i += 64) {
#pragma clang fp contract(off)
        const double s = mix_speech(a, r, i, m.p);
        const double v = load_f64(a.noise, a.noise_f64, r.n0 + i) * m.g;
        const double os = s / norm, ov = v / norm, ox = (s + v) / norm;
        store_f64(out_speech, a.out_f64, r.o0 + i, os);
        store_f64(out_noise, a.out_f64, r.o0 + i, ov);
        store_f64(out_mix, a.out_f64, r.o0 + i, ox);
        qs += os * os;
        qn += ov * ov;
    }
    if (r.hi == r.len) {
        for (int64_t i = r.len + lane; i < r.extent; i += 64) {
            store_f64(out_speech, a.out_f64, r.o0 + i, 0.0);
            store_f64(out_noise, a.out_f64, r.o0 + i, 0.0);
            store_f64(out_mix, a.out_f64, r.o0 + i, 0.0);
        }
    }
    qs = wave_sum(qs);
    qn = wave_sum(qn);
    if (lane == 0) {
        w.out_sq[mix_item_index() * 2] = qs;
        w.out_sq[mix_item_index() * 2 + 1] = qn;
    }
}

// finish: stats[u] = {p, Ps, Pn, k, norm, achieved SNR in dB}; NaN for an utterance whose table entry is bad
__global__ __launch_bounds__(256) void mix_finish_kernel(MixArgs a, MixWork w, double* __restrict__ stats) {
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= a.U) return;
    const int lane = threadIdx.x & 63;
    double out[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = NAN;
    MixItem r;
    if (mix_utterance(a, u, r)) {
        const MixScalars m = mix_scalars(a, w, r, lane, true);
        double qs = 0.0, qn = 0.0;
        for (int64_t p = r.p0; p < r.p1; ++p) {
            qs += w.out_sq[p * 2];
            qn += w.out_sq[p * 2 + 1];
        }
        out[0] = m.p;
        out[1] = m.Ps;
        out[2] = m.Pn;
        out[3] = m.k;
        out[4] = mix_total_max(w.norm, r, lane);
        out[5] = 10.0 * log10(qs / qn);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) stats[(int64_t)u * 6 + k] = out[k];
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_mix_snr_workspace_bytes(int64_t n_items, int U) {
    (void)U;                                          // every partial is per item; the passes keep nothing per utterance
    return (size_t)(n_items > 0 ? n_items : 1) * 6 * sizeof(double);
}

extern "C" int dvae_mix_snr_batch(const void* speech, int64_t n_speech, int speech_f64, const void* noise, int64_t n_noise, int noise_f64, int U,
                                  const int64_t* tables, int64_t n_items, const double* snr_factor, int normalise_speech, void* out_speech,
                                  void* out_noise, void* out_mix, int64_t n_out, int out_f64, double* stats, void* workspace, void* stream) {
    DVAE_CHECK_ARG(speech && noise && workspace && snr_factor && n_speech > 0 && n_noise > 0, "mix_snr_batch: null argument or empty buffer");
    DVAE_CHECK_ARG(out_speech && out_noise && out_mix && n_out > 0, "mix_snr_batch: the three outputs and their extent are required");
    DVAE_CHECK_ARG(out_speech != out_noise && out_speech != out_mix && out_noise != out_mix, "mix_snr_batch: the three outputs must be three buffers");
    DVAE_CHECK_ARG(batch_launch_ok(U, tables, n_items) && n_items >= U, "mix_snr_batch: bad table (U %d, %lld items)", U, (long long)n_items);
    const MixArgs a{speech, noise, n_speech, n_noise, n_out, speech_f64 != 0, noise_f64 != 0, out_f64 != 0, normalise_speech != 0, U, tables, n_items,
                    snr_factor};
    double* ws = (double*)workspace;
    const MixWork w{ws, ws + n_items, ws + 3 * n_items, ws + 4 * n_items};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(n_items, 4));
    if (a.normalise) {
        hipLaunchKernelGGL(mix_peak_kernel, grid, dim3(256), 0, s, a, w);
        DVAE_LAUNCH_OK("mix_peak_kernel");
    }
    hipLaunchKernelGGL(mix_power_kernel, grid, dim3(256), 0, s, a, w);
    DVAE_LAUNCH_OK("mix_power_kernel");
    hipLaunchKernelGGL(mix_norm_kernel, grid, dim3(256), 0, s, a, w);
    DVAE_LAUNCH_OK("mix_norm_kernel");
    hipLaunchKernelGGL(mix_write_kernel, grid, dim3(256), 0, s, a, w, out_speech, out_noise, out_mix);
    DVAE_LAUNCH_OK("mix_write_kernel");
    if (stats) {
        hipLaunchKernelGGL(mix_finish_kernel, dim3((unsigned)cdiv(U, 4)), dim3(256), 0, s, a, w, stats);
        DVAE_LAUNCH_OK("mix_finish_kernel");
    }
    return 0;
}

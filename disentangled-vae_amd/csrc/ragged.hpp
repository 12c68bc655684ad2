// Device side of ragged batches: U utterances of different lengths packed end to end in one buffer (host side: ../ragged.py).  Every
// batch kernel runs one wave per work item -- one utterance and a fixed run of `chunk` of its samples, frames or bins -- in workgroups of
// four waves.  The wave finds its utterance in the item prefix table (batch_item), takes its run of the utterance from the table's
// own entries (item_range) and drops its work if they disagree with each other or with the scalar extents the host passed: no
// table entry is trusted before memory is touched.  A new ragged op starts from these helpers and adds only its own extent checks.
#pragma once
#include "common.hpp"

namespace dvae {

// The wave's work item (or utterance, in a one-wave-per-utterance kernel), in scalar registers.
__device__ __forceinline__ int64_t wave_item() { return (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// `pref` [U + 1] is the prefix of the per-utterance work-item counts (pref[0] = 0); item i belongs to the utterance u
// with pref[u] <= i < pref[u + 1] (a binary search with wave-uniform addresses: scalar loads).  u = -1 past the last item.
struct BatchItem { int u; int64_t local; };
__device__ __forceinline__ int64_t uni64(int64_t v) {          // a wave-uniform 64-bit value in scalar registers
    const uint64_t w = (uint64_t)v;
    return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w));
}
__device__ __forceinline__ BatchItem batch_item(const int64_t* __restrict__ pref, int U, int64_t item) {
    if (U < 1 || item < 0 || item >= uni64(pref[U])) return BatchItem{-1, 0};
    int lo = 0, hi = U;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (uni64(pref[mid]) <= item) lo = mid; else hi = mid;
    }
    const int64_t local = item - uni64(pref[lo]);
    return local < 0 ? BatchItem{-1, 0} : BatchItem{lo, local};
}

// One work item of a batch whose utterance u spans `extent` units (samples, frames or bins) in runs of `chunk`: [lo, hi) of them,
// with the utterance's partials at [p0, p1).  ok = false for an entry the host's checks would have refused.
struct ItemRange { int u; int64_t lo, hi, p0, p1; bool ok; };
__device__ __forceinline__ ItemRange item_range(const int64_t* __restrict__ tab, int U, int64_t n_items, int64_t item, int64_t extent, int chunk,
                                                BatchItem it) {
    ItemRange r{it.u, 0, 0, 0, 0, false};
    const int64_t p0 = uni64(tab[it.u]), p1 = uni64(tab[it.u + 1]);
    r.lo = it.local * chunk;
    r.hi = r.lo + chunk < extent ? r.lo + chunk : extent;
    r.p0 = p0;
    r.p1 = p1;
    r.ok = extent >= 1 && item < n_items && p0 >= 0 && p1 <= n_items && p1 - p0 == (extent + chunk - 1) / chunk && r.lo < extent;
    return r;
}

// element i of a packed buffer of float32 or float64, as a double (a float32 sample converts exactly)
__device__ __forceinline__ double load_f64(const void* p, int is_f64, int64_t i) {
    return is_f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}
__device__ __forceinline__ void store_f64(void* p, int is_f64, int64_t i, double v) {
    if (is_f64) ((double*)p)[i] = v; else ((float*)p)[i] = (float)v;
}

// what every batch entry point asks of its table before it launches: one workgroup per four items, in a 31-bit grid
static inline bool batch_launch_ok(int U, const int64_t* tables, int64_t n_items) {
    return U > 0 && tables && n_items > 0 && cdiv(n_items, 4) < ((int64_t)1 << 31);
}

}  // namespace dvae

// STFT / ISTFT for packages/processing/stft.py (librosa semantics restated in oracle/stft_oracle.py): the HOST side.  Every extern "C"
// entry, its argument checks, the environment switches and the choice between the kernels; no device code.  The forward kernels, with
// the description of the transform, are in stft_fwd.hip, the inverse kernels in istft.hip, each with the launchers called here
// (declared in stft_types.hpp); the FFT pieces the kernels share are in fft_wave.hpp.
#include <stdlib.h>
#include "common.hpp"
#include "stft_types.hpp"

namespace dvae {

static inline int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

}  // namespace dvae

using namespace dvae;

extern "C" int dvae_stft(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop,
                         int64_t T, void* out, int layout, void* stream) {
    DVAE_CHECK_ARG(x && window && out && n > 0 && nfft >= 4 && (nfft % 2) == 0 && hop > 0 && T >= 0, "stft: bad argument");
    DVAE_CHECK_ARG(layout >= 0 && layout <= 2, "stft: unknown output layout %d", layout);
    DVAE_CHECK_ARG(T == 0 || (T - 1) * (int64_t)hop + nfft <= n, "stft: %lld frames do not fit in %lld samples", (long long)T, (long long)n);
    if (T == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int lg = ilog2_exact(nfft);
    static const bool legacy = getenv("DVAE_STFT_LEGACY") != nullptr;       // A/B switch for the workgroup-per-frame kernel
    if (nfft == 1024 && !legacy) {
        if (layout == 0) return launch_stft1024(x, in_f64, n, window, hop, T, 1, out, layout, s);
        // one round of waves: 256 CUs x 4 SIMDs x 2 resident waves = 2048 slots; a wave takes ceil(T / 2048) frames
        int chunk = (int)cdiv(T, 2048);
        chunk = chunk < 1 ? 1 : chunk;
        // hop 256 and everything addressable with 32-bit byte offsets: the walk with buffer addressing and the register ring
        static const bool oldwalk = getenv("DVAE_STFT_WALK") != nullptr && !strcmp(getenv("DVAE_STFT_WALK"), "r3");
        const bool ring = hop == 256 && !oldwalk && n * (in_f64 ? 8 : 4) < ((int64_t)1 << 31) && T * 513 * (layout == 1 ? 4 : 8) < ((int64_t)1 << 31);
        if (!ring) return launch_stft1024(x, in_f64, n, window, hop, T, chunk, out, layout, s);
        // DVAE_STFT_OCC=3 (diagnostic build): three waves per SIMD with the window and two twiddle tables read from LDS every frame
        // (166 registers, 50 KB of LDS per workgroup) -- measured SLOWER, 63.3 / 64.9 us against 57.8 / 61.4 (complex / power frames,
        // ten minutes of float64 audio, alternating on one box): the 19 extra ds_read_b128 per frame cost more than the third wave hides
        static const bool occ3 = kDiagBuild && getenv("DVAE_STFT_OCC") != nullptr && atoi(getenv("DVAE_STFT_OCC")) == 3;
        if (occ3) {
            chunk = (int)cdiv(T, 3072);                        // one round of 256 CUs x 4 SIMDs x 3 resident waves
            chunk = chunk < 1 ? 1 : chunk;
        }
        return launch_stft1024_walk(x, in_f64, n, window, T, chunk, out, layout, occ3, nullptr, 0, 0, s);
    }
    if (lg >= 3 && nfft <= 2048) return launch_stft_pow2(x, in_f64, n, window, nfft, lg - 1, hop, T, out, layout, s);
    DVAE_CHECK_ARG(nfft <= 2048, "stft: window length %d not supported (max 2048)", nfft);
    return launch_stft_dft(x, in_f64, n, window, nfft, hop, T, out, layout, s);
}

extern "C" int dvae_stft_f32(const float* x, int64_t n, const float* window, int nfft, int hop, int64_t T, void* out, int layout, void* stream) {
    DVAE_CHECK_ARG(x && window && out && n > 0 && T >= 0, "stft_f32: bad argument");
    DVAE_CHECK_ARG(nfft == 1024 && hop == 256, "stft_f32: the float32-arithmetic transform exists for nfft 1024 / hop 256 (got %d / %d): use dvae_stft", nfft, hop);
    DVAE_CHECK_ARG(layout == 1 || layout == 2, "stft_f32: frame-major layouts only (1 power frames, 2 complex frames), got %d", layout);
    DVAE_CHECK_ARG(T == 0 || (T - 1) * (int64_t)hop + nfft <= n, "stft_f32: %lld frames do not fit in %lld samples", (long long)T, (long long)n);
    DVAE_CHECK_ARG(n * 4 < ((int64_t)1 << 31) && T * 513 * (layout == 1 ? 4 : 8) < ((int64_t)1 << 31), "stft_f32: signal or spectrogram beyond 2 GB (32-bit buffer offsets)");
    if (T == 0) return 0;
    // one round of waves: 256 CUs x 4 SIMDs x STFT_F32_OCC resident waves
    int chunk = (int)cdiv(T, (int64_t)1024 * STFT_F32_OCC);
    chunk = chunk < 1 ? 1 : chunk;
    return launch_stft1024_walk_f32(x, n, window, T, chunk, out, layout, (hipStream_t)stream);
}

extern "C" size_t dvae_istft_workspace_bytes(int64_t T, int nfft) {
    return (size_t)(T > 0 ? T : 0) * (size_t)nfft * sizeof(double);
}

// the 1024 / 256 transform (every caller of the reference) runs as one kernel and needs no frame scratch
extern "C" size_t dvae_istft_workspace_bytes_hop(int64_t T, int nfft, int hop) {
    if (nfft == 1024 && hop == 256 && getenv("DVAE_STFT_LEGACY") == nullptr && getenv("DVAE_ISTFT_2PASS") == nullptr)
        return T >= ISTFT_TR_MIN_T ? (size_t)T * 513 * sizeof(float2) + 16 : 16;      // long bin-major input: its frame-major copy
    return dvae_istft_workspace_bytes(T, nfft);
}

// S(bin f, frame t) = S[f * ld + t] (tf = false: bin-major, ld >= T) or S[t * ld + f] (tf = true: frame-major, ld >= nfft / 2 + 1)
static int istft_run(const void* S, int64_t T, int64_t ld, bool tf, const double* window, int nfft, int hop,
                     int64_t start, float* y, int64_t out_len, void* ws, void* stream) {
    DVAE_CHECK_ARG(S && window && y && ws && T > 0 && nfft >= 4 && (nfft % 2) == 0 && hop > 0 && start >= 0 && out_len >= 0,
                   "istft: bad argument");
    DVAE_CHECK_ARG(ld >= (tf ? (int64_t)(nfft / 2 + 1) : T), "istft: leading dimension %lld too small", (long long)ld);
    DVAE_CHECK_ARG(nfft <= 2048, "istft: window length %d not supported (max 2048)", nfft);
    hipStream_t s = (hipStream_t)stream;
    const int64_t sf = tf ? 1 : ld, st = tf ? ld : 1;
    const int lg = ilog2_exact(nfft);
    static const bool legacy = getenv("DVAE_STFT_LEGACY") != nullptr;
    const bool two_pass = getenv("DVAE_ISTFT_2PASS") != nullptr;             // A/B switch (read per call): frames to scratch + gather overlap-add
    if (nfft == 1024 && hop == 256 && !legacy && !two_pass) {
        if (out_len == 0) return 0;
        if (tf && getenv("DVAE_ISTFT_STAGED") == nullptr) {                  // A/B switch (read per call): frame-major input through the staged kernel
            // one round of waves (2048 slots, as the forward transform): the shortest walk per wave, ceil(T / 2048) own frames + 3 halo
            // frames (short utterances: 4 transforms for 1 own frame, all waves side by side -- 12 us at 309 frames against 19 us with 4 own)
            const char* const slots_s = getenv("DVAE_ISTFT_SLOTS");          // experiment switch: waves the frames are dealt to (default: one round of 2048)
            const int slots = slots_s && atoi(slots_s) >= 64 ? atoi(slots_s) : 2048;
            int chunk = (int)cdiv(T, slots);
            chunk = chunk < 1 ? 1 : chunk;
            return launch_istft1024_walk((const float2*)S, T, ld, window, start, y, out_len, chunk, s);
        }
        if (!tf && T >= ISTFT_TR_MIN_T && getenv("DVAE_ISTFT_STAGED") == nullptr) {
            // long bin-major spectrograms: one transposing pass into the workspace, then the frame-major walk (ten minutes of audio:
            // 88 + 81 us against the staged kernel's 207; the same arithmetic, bit-identical)
            if (const int rc = launch_c64_transpose((const float2*)S, T, ld, (float2*)ws, s)) return rc;
            int chunk = (int)cdiv(T, 2048);
            chunk = chunk < 1 ? 1 : chunk;
            return launch_istft1024_walk((const float2*)ws, T, (int64_t)513, window, start, y, out_len, chunk, s);
        }
        // the staged kernel (frame-major input: diagnostic builds only, DVAE_ISTFT_STAGED)
        return launch_istft1024_fused((const float2*)S, T, ld, tf, window, start, y, out_len, s);
    }
    int rc;
    if (nfft == 1024 && !legacy) rc = launch_istft1024_frames((const float2*)S, T, sf, st, window, (double*)ws, s);
    else if (lg >= 3) rc = launch_istft_frames_pow2((const float*)S, T, sf, st, window, nfft, lg - 1, (double*)ws, s);
    else rc = launch_istft_frames_dft((const float*)S, T, sf, st, window, nfft, (double*)ws, s);
    if (rc) return rc;
    if (out_len == 0) return 0;
    return launch_istft_ola((const double*)ws, window, T, nfft, hop, start, y, out_len, s);
}

extern "C" int dvae_istft(const void* S, int64_t T, int64_t ldT, const double* window, int nfft, int hop,
                          int64_t start, float* y, int64_t out_len, void* ws, void* stream) {
    return istft_run(S, T, ldT, false, window, nfft, hop, start, y, out_len, ws, stream);
}

extern "C" int dvae_istft_frames(const void* S, int64_t T, int64_t ldF, const double* window, int nfft, int hop,
                                 int64_t start, float* y, int64_t out_len, void* ws, void* stream) {
    return istft_run(S, T, ldF, true, window, nfft, hop, start, y, out_len, ws, stream);
}

// Ragged batches (nfft 1024 / hop 256 only).  Work items: one utterance and a run of at most `chunk` of its frames, chunk = one round of
// 2048 wave slots over the batch's frames (as the single-signal walks), so item counts and the launch depend on the tables the host
// built; the kernels check every table entry against the scalar extents below before they touch memory.
extern "C" int dvae_stft_batch(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop, int U, const int64_t* tables,
                               int64_t n_items, int chunk, int64_t T_total, void* out, int layout, void* stream) {
    DVAE_CHECK_ARG(nfft == 1024 && hop == 256, "stft_batch: the batch transform exists for nfft 1024 / hop 256 (got %d / %d): use dvae_stft per signal",
                   nfft, hop);
    DVAE_CHECK_ARG(x && window && tables && out && n > 0 && U > 0 && n_items > 0 && chunk > 0 && T_total > 0, "stft_batch: bad argument");
    DVAE_CHECK_ARG(layout == 1 || layout == 2, "stft_batch: frame-major layouts only (1 power frames, 2 complex frames), got %d", layout);
    DVAE_CHECK_ARG(n_items <= T_total && cdiv(n_items, 4) < ((int64_t)1 << 31), "stft_batch: %lld work items for %lld frames", (long long)n_items,
                   (long long)T_total);
    return launch_stft1024_walk(x, in_f64, n, window, T_total, chunk, out, layout, false, tables, U, n_items, (hipStream_t)stream);
}

extern "C" int dvae_istft_batch(const void* S, int64_t T_total, const double* window, int nfft, int hop, int U, const int64_t* tables, int64_t n_items,
                                int chunk, int64_t start, float* y, int64_t y_total, const float* gain0, const float* gain1, int64_t ldg, float* y1,
                                void* stream) {
    DVAE_CHECK_ARG(nfft == 1024 && hop == 256, "istft_batch: the batch transform exists for nfft 1024 / hop 256 (got %d / %d): use dvae_istft_frames per "
                   "signal", nfft, hop);
    DVAE_CHECK_ARG(S && window && tables && y && T_total > 0 && U > 0 && n_items > 0 && chunk > 0 && start >= 0 && y_total > 0, "istft_batch: bad argument");
    DVAE_CHECK_ARG(n_items <= T_total && cdiv(n_items, 4) < ((int64_t)1 << 31), "istft_batch: %lld work items for %lld frames", (long long)n_items,
                   (long long)T_total);
    DVAE_CHECK_ARG(gain0 || !gain1, "istft_batch: a second gain plane needs a first");
    DVAE_CHECK_ARG(!gain0 || (ldg > 0 && 513 * ldg * 4 < ((int64_t)1 << 31)), "istft_batch: gain leading dimension %lld (a gain plane is read below 2 GB)",
                   (long long)ldg);
    DVAE_CHECK_ARG(!gain1 || y1, "istft_batch: the second gain plane needs its output");
    const IstftBatch bt{tables, U, T_total, y_total, {gain0, gain1}, ldg, y1};
    return launch_istft1024_walk_batch((const float2*)S, window, start, y, chunk, n_items, bt, (hipStream_t)stream);
}

// float32-arithmetic inverse transform (istft_pytorch): S bin-major ([513][ld], frames = 0: transposed into ws first, T * 513 complex64)
// or frame-major ([T][ld], frames = 1: read in place, ws unused)
extern "C" int dvae_istft_f32(const void* S, int64_t T, int64_t ld, int frames, const float* window, int nfft, int hop,
                              int64_t start, float* y, int64_t out_len, void* ws, void* stream) {
    DVAE_CHECK_ARG(S && window && y && T > 0 && start >= 0 && out_len >= 0, "istft_f32: bad argument");
    DVAE_CHECK_ARG(nfft == 1024 && hop == 256, "istft_f32: window length 1024 / hop 256 only (got %d / %d): use dvae_istft", nfft, hop);
    DVAE_CHECK_ARG(ld >= (frames ? (int64_t)513 : T), "istft_f32: leading dimension %lld too small", (long long)ld);
    DVAE_CHECK_ARG(frames || ws, "istft_f32: bin-major input needs the workspace (T * 513 complex64)");
    DVAE_CHECK_ARG(T * (frames ? ld : (int64_t)513) * 8 < ((int64_t)1 << 31), "istft_f32: spectrograms of 2 GB and more are not addressed (use dvae_istft)");
    hipStream_t s = (hipStream_t)stream;
    if (out_len == 0) return 0;
    const float2* Sf = (const float2*)S;
    int64_t ldf = ld;
    if (!frames) {
        if (const int rc = launch_c64_transpose((const float2*)S, T, ld, (float2*)ws, s)) return rc;
        Sf = (const float2*)ws;
        ldf = 513;
    }
    const char* const slots_s = getenv("DVAE_ISTFT_SLOTS");          // experiment switch, as in the double walk
    const int slots = slots_s && atoi(slots_s) >= 64 ? atoi(slots_s) : 2048;
    int chunk = (int)cdiv(T, slots);                               // one round of waves, as the double walk
    chunk = chunk < 1 ? 1 : chunk;
    return launch_istft1024_walk_f32(Sf, T, ldf, window, start, y, out_len, chunk, s);
}

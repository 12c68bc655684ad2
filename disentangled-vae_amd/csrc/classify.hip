// The classifier stage of the M2_info evaluation for a whole ragged batch in one launch (disentangled-vae_amd/classify.py; the
// reference's `model.classifier(torch.t(S_abs_2))` and `y_hat_soft > 0.5`, scripts/evaluate_ntcd_M2_info_vad.py:175-219), and the
// confusion counts that f1_loss takes from hard labels (packages/models/utils.py:147-150), per utterance.
//
// dvae_classify_batch: 513 -> 128 (relu) -> 128 (relu) -> y_dim (sigmoid), y_dim 1 or 513, exact fp32 on v_mfma_f32_32x32x2_f32.
// One 256-thread workgroup walks 64-frame tiles, grid-strided.  Layer 1 consumes k in 32-deep slabs as gemm_f32.hip does: the
// power slab [64][32] (squared on the way in from complex input, spec_power.hpp) and the W1 slab [128][32] are staged in LDS with
// a register prefetch of the next slab, W1 streaming from L2.  Wave w owns output columns 32 w .. 32 w + 31 of all 64 frames (two
// 32 x 32 accumulators).  h1, then h2 in its place, stay in LDS [64][129]; W2 and (y_dim 513) W3 stream through the same slab
// buffer.  The y_dim 1 output layer is one fma chain per frame on the vector units.
//
// Every output element is one chain over k ascending (layer 1 padded with zero products to 544), whatever the frame's place in its
// tile, the tile's place in the grid and the frames around it: a frame gives the same bits alone, in any batch and from run to run.
// Frames outside [frame_off[0], frame_off[U]) or past N are neither read nor written.  The slab loaders, the MFMA slab and the table
// check are frame_tiles.hpp, shared with encode.hip.
#include "common.hpp"
#include "frame_tiles.hpp"
#include "spec_power.hpp"

namespace dvae {

struct ClassifyArgs {
    const void* src;      // complex64 [N][513] or float32 [N][ld]
    int is_complex;
    int64_t ld, N, lo, hi;                   // frames lo <= r < hi are classified (0 <= lo <= hi <= N, checked by the host)
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    int y_dim;
    float *soft, *hard, *logits;             // [N][y_dim]; logits may be null
    int64_t tile0, ntiles;
};

// the next layer-1 slab of the input tile: 64 frames x 32 bins, thread -> bin (tid & 31), frames (tid >> 5) + 8 i
__device__ __forceinline__ void load_power(const ClassifyArgs& g, int64_t r0, int kc, int tid, const int* rowok, float (&r)[8]) {
    const int k = kc + (tid & 31), rr = tid >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = rr + 8 * i;
        float p = 0.f;
        if (k < CF && rowok[row]) {
            const int64_t at = (r0 + row) * g.ld + k;
            if (g.is_complex) {
                const float2 v = ((const float2*)g.src)[at];
                p = np_power_c64(v.x, v.y);
            } else {
                p = ((const float*)g.src)[at];
            }
        }
        r[i] = p;
    }
}

__device__ __forceinline__ void store_hidden(float* H, const float* __restrict__ bias, int wave, int l31, int h, const f32x16& acc0, const f32x16& acc1) {
    const int col = wave * 32 + l31;
    const float b = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, h);
        const float v0 = acc0[r] + b, v1 = acc1[r] + b;
        H[row * HLD + col] = v0 > 0.f ? v0 : 0.f;
        H[(32 + row) * HLD + col] = v1 > 0.f ? v1 : 0.f;
    }
}

__device__ __forceinline__ void write_label(const ClassifyArgs& g, int64_t at, float logit) {
    const float s = 1.f / (1.f + expf(-logit));
    g.soft[at] = s;
    g.hard[at] = s > 0.5f ? 1.f : 0.f;
    if (g.logits) g.logits[at] = logit;
}

__global__ __launch_bounds__(256) void classify_kernel(const ClassifyArgs g) {
    __shared__ float H[CT * HLD];
    __shared__ float As[CT * SLD];
    __shared__ float Bs[CH * SLD];
    __shared__ int rowok[CT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;

    for (int64_t tile = g.tile0 + blockIdx.x; tile < g.tile0 + g.ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * CT;
        __syncthreads();                                   // the previous tile's readers of rowok and H are done
        if (tid < CT) rowok[tid] = (r0 + tid >= g.lo && r0 + tid < g.hi && r0 + tid < g.N) ? 1 : 0;
        __syncthreads();

        // ---- layer 1: h1 = relu(P W1^T + b1), k = 0 .. 543 in 17 slabs ----
        f32x16 acc0, acc1;
        zero(acc0); zero(acc1);
        float ra[8], rb[16];
        load_power(g, r0, 0, tid, rowok, ra);
        load_w(g.W1, CH, CF, 0, 0, tid, rb);
        for (int kc = 0; kc < CF; kc += CK) {
            {
                const int c = tid & 31, rr = tid >> 5;
#pragma unroll
                for (int i = 0; i < 8; ++i) As[(rr + 8 * i) * SLD + c] = ra[i];
            }
            store_w(Bs, tid, rb);
            __syncthreads();
            if (kc + CK < CF) {
                load_power(g, r0, kc + CK, tid, rowok, ra);
                load_w(g.W1, CH, CF, 0, kc + CK, tid, rb);
            }
            mfma_slab(As, SLD, 0, Bs, wave, l31, h, acc0, acc1);
            __syncthreads();
        }
        store_hidden(H, g.b1, wave, l31, h, acc0, acc1);

        // ---- layer 2: h2 = relu(h1 W2^T + b2), in h1's place once every wave has read it ----
        zero(acc0); zero(acc1);
        load_w(g.W2, CH, CH, 0, 0, tid, rb);
        for (int kc = 0; kc < CH; kc += CK) {
            store_w(Bs, tid, rb);
            __syncthreads();                               // also orders layer 1's writes of H before the first read
            if (kc + CK < CH) load_w(g.W2, CH, CH, 0, kc + CK, tid, rb);
            mfma_slab(H, HLD, kc, Bs, wave, l31, h, acc0, acc1);
            __syncthreads();
        }
        store_hidden(H, g.b2, wave, l31, h, acc0, acc1);
        __syncthreads();

        // ---- output layer ----
        if (g.y_dim == 1) {
            if (tid < CT && rowok[tid]) {
                float s = 0.f;
#pragma unroll 8
                for (int k = 0; k < CH; ++k) s = __fmaf_rn(H[tid * HLD + k], g.W3[k], s);
                write_label(g, r0 + tid, s + g.b3[0]);
            }
        } else {
            for (int n0 = 0; n0 < g.y_dim; n0 += CH) {       // column tiles of 128: wave w owns columns n0 + 32 w .. + 31
                zero(acc0); zero(acc1);
                load_w(g.W3, g.y_dim, CH, n0, 0, tid, rb);
                for (int kc = 0; kc < CH; kc += CK) {
                    store_w(Bs, tid, rb);
                    __syncthreads();
                    if (kc + CK < CH) load_w(g.W3, g.y_dim, CH, n0, kc + CK, tid, rb);
                    mfma_slab(H, HLD, kc, Bs, wave, l31, h, acc0, acc1);
                    __syncthreads();
                }
                const int col = n0 + wave * 32 + l31;
                if (col < g.y_dim) {
                    const float b = g.b3[col];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = acc_row(r, h);
                        if (rowok[row]) write_label(g, (r0 + row) * g.y_dim + col, acc0[r] + b);
                        if (rowok[32 + row]) write_label(g, (r0 + 32 + row) * g.y_dim + col, acc1[r] + b);
                    }
                }
            }
        }
    }
}

// ---- confusion counts ----------------------------------------------------------------------------------------------------------------------

constexpr int LC_RUN = 4096;        // elements per wave: the sums are integers, so the split changes nothing

// One wave per run of LC_RUN elements of the flat range [off[0] * y, off[U] * y); the run is cut where an utterance ends, each piece
// reduced in the wave and added to its utterance's four counters.  `off` is the device copy of the table the host checked; every entry
// is clamped to [lo, hi] before use, so a copy that differs cannot take a read outside the rows.
__global__ __launch_bounds__(256) void label_counts_kernel(const float* __restrict__ pred, int64_t ldp, const float* __restrict__ truth, int64_t ldt,
                                                           int y, int U, const int64_t* __restrict__ off, int64_t lo, int64_t hi,
                                                           unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t e_lo = lo * y, e_hi = hi * y;
    int64_t e = e_lo + item * LC_RUN;
    if (e >= e_hi) return;
    const int64_t e_end = e + LC_RUN < e_hi ? e + LC_RUN : e_hi;
    const int64_t row0 = e / y;
    int a = 0, b = U;                                      // off[a] <= row0 < off[b]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (off[mid] <= row0) a = mid; else b = mid;
    }
    for (int u = a; u < U && e < e_end; ++u) {
        int64_t u_end = off[u + 1];
        u_end = (u_end < lo ? lo : u_end > hi ? hi : u_end) * y;
        const int64_t stop = u_end < e_end ? u_end : e_end;
        if (stop <= e) continue;
        unsigned tp = 0, tn = 0, fp = 0, fn = 0;
        for (int64_t i = e + lane; i < stop; i += 64) {
            const uint32_t local = (uint32_t)(i - row0 * y);          // < LC_RUN + y
            const uint32_t rr = local / (uint32_t)y, cc = local - rr * (uint32_t)y;
            const bool p = pred[(row0 + rr) * ldp + cc] != 0.f, t = truth[(row0 + rr) * ldt + cc] != 0.f;
            tp += p && t; tn += !p && !t; fp += p && !t; fn += !p && t;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            tp += __shfl_xor(tp, o, 64); tn += __shfl_xor(tn, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64);
        }
        if (lane == 0) {
            if (tp) atomicAdd(counts + 4 * u + 0, (unsigned long long)tp);
            if (tn) atomicAdd(counts + 4 * u + 1, (unsigned long long)tn);
            if (fp) atomicAdd(counts + 4 * u + 2, (unsigned long long)fp);
            if (fn) atomicAdd(counts + 4 * u + 3, (unsigned long long)fn);
        }
        e = stop;
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_classify_weights_floats(int y_dim) {
    if (y_dim != 1 && y_dim != CF) return 0;
    return (size_t)CH * CF + CH + (size_t)CH * CH + CH + (size_t)y_dim * CH + y_dim;
}

extern "C" int dvae_classify_batch(const void* src, int src_complex, int64_t ld, int64_t N, int U, const int64_t* frame_off_host,
                                   const float* weights, int y_dim, float* soft, float* hard, float* logits, void* stream) {
    DVAE_CHECK_ARG(src && frame_off_host && weights && soft && hard, "classify_batch: null pointer");
    DVAE_CHECK_ARG(y_dim == 1 || y_dim == CF, "classify_batch: y_dim %d (the kernel covers 1 and %d)", y_dim, CF);
    DVAE_CHECK_ARG(N > 0 && U > 0, "classify_batch: %lld rows, %d utterances", (long long)N, U);
    DVAE_CHECK_ARG(src_complex == 0 || src_complex == 1, "classify_batch: src_complex %d", src_complex);
    DVAE_CHECK_ARG(src_complex ? ld == CF : ld >= CF, "classify_batch: leading dimension %lld (%s)", (long long)ld,
                   src_complex ? "complex frames are packed: 513" : "at least 513");
    DVAE_CHECK_ARG(N < ((int64_t)1 << 40) && ld < ((int64_t)1 << 20), "classify_batch: %lld rows of %lld", (long long)N, (long long)ld);
    if (int rc = check_frame_off("classify_batch", frame_off_host, U, N)) return rc;
    ClassifyArgs g{};
    g.src = src; g.is_complex = src_complex; g.ld = ld; g.N = N;
    g.lo = frame_off_host[0]; g.hi = frame_off_host[U];
    if (g.hi == g.lo) return 0;
    g.W1 = weights;              g.b1 = g.W1 + (size_t)CH * CF;
    g.W2 = g.b1 + CH;            g.b2 = g.W2 + (size_t)CH * CH;
    g.W3 = g.b2 + CH;            g.b3 = g.W3 + (size_t)y_dim * CH;
    g.y_dim = y_dim; g.soft = soft; g.hard = hard; g.logits = logits;
    g.tile0 = g.lo / CT;
    g.ntiles = cdiv(g.hi, CT) - g.tile0;
    const int64_t blocks = g.ntiles < 2048 ? g.ntiles : 2048;         // 256 CUs x 2 resident workgroups x 4 rounds; the rest strides
    hipLaunchKernelGGL(classify_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g);
    DVAE_LAUNCH_OK("classify_kernel");
    return 0;
}

extern "C" int dvae_label_counts_batch(const float* pred, int64_t ldp, const float* truth, int64_t ldt, int64_t N, int y_dim, int U,
                                       const int64_t* frame_off_host, const int64_t* frame_off_dev, int64_t* counts, void* stream) {
    DVAE_CHECK_ARG(pred && truth && frame_off_host && frame_off_dev && counts, "label_counts_batch: null pointer");
    DVAE_CHECK_ARG(N > 0 && U > 0, "label_counts_batch: %lld rows, %d utterances", (long long)N, U);
    DVAE_CHECK_ARG(y_dim >= 1 && y_dim <= (1 << 20), "label_counts_batch: y_dim %d", y_dim);
    DVAE_CHECK_ARG(ldp >= y_dim && ldt >= y_dim && ldp < ((int64_t)1 << 24) && ldt < ((int64_t)1 << 24), "label_counts_batch: leading dimensions %lld, %lld for y_dim %d",
                   (long long)ldp, (long long)ldt, y_dim);
    DVAE_CHECK_ARG(N < ((int64_t)1 << 38), "label_counts_batch: %lld rows", (long long)N);
    if (int rc = check_frame_off("label_counts_batch", frame_off_host, U, N)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DVAE_HIP(hipMemsetAsync(counts, 0, (size_t)U * 4 * sizeof(int64_t), s));
    const int64_t lo = frame_off_host[0], hi = frame_off_host[U];
    if (hi == lo) return 0;
    const int64_t items = cdiv((hi - lo) * y_dim, LC_RUN);
    DVAE_CHECK_ARG(cdiv(items, 4) < ((int64_t)1 << 31), "label_counts_batch: %lld elements", (long long)((hi - lo) * y_dim));
    hipLaunchKernelGGL(label_counts_kernel, dim3((unsigned)cdiv(items, 4)), dim3(256), 0, s, pred, ldp, truth, ldt, y_dim, U, frame_off_dev, lo, hi,
                       (unsigned long long*)counts);
    DVAE_LAUNCH_OK("label_counts_kernel");
    return 0;
}

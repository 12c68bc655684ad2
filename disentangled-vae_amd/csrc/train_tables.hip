// The kernels every fused train step of any covered size launches behind its own rows kernel (train_generic.hip: M1 / M2;
// train_info.hip: M2_info; train_classifier.hip: the label classifier), driven by the tables of train_tables.hpp, and their launches:
//   * weight-gradient kernel: one launch for all weight matrices of a step and their biases, dW = dPre^T in over the frames on
//     v_mfma_f32_16x16x4_f32 (k = frames), driven by a host-built table of (matrix, 64-row output group, four 64-column blocks, frame
//     slice) items; a wave keeps a 64 x 64 block of dW in sixteen accumulators.  x and y are read from the caller's memory (through the
//     gather table when there is one); the bias is the product with a column of ones.  Every item writes its blocks of its slice's
//     slab: no atomics, and the same inputs give the same bits.
//   * apply kernel: one thread per parameter: slab sum in slab order, adam_element (apply_common.hpp), both packed copies refreshed,
//     loss scalars finalised from the rows kernel's per-workgroup sums (and added to the optional float64 accumulator).
//   * reduce kernel (gradient accumulation, data parallelism): the slabs of a micro-batch summed into one flat gradient; and, for
//     global-norm clipping on the device, a norm kernel over that flat gradient (per-chunk sums of squares in double, fixed order) in
//     front of a guarded instantiation of the apply kernel's body (train_tables.hpp: GNormArgs / GClipArgs).
// The kernels keep the names they had in train_generic.hip: profiles, tools and tests refer to them.
#include <math.h>
#include "common.hpp"
#include "../../include/dvae_train.h"
#include "apply_common.hpp"
#include "train_tables.hpp"

namespace dvae {
namespace tg {

using fused::ApplyArgs;

// ---------------------------------------------------------------------------------------------------------------------------------
// weight-gradient kernel (GWgradArgs: train_tables.hpp)
// One item = 64 rows of one matrix (four 16-row tiles of dPre) x four 64-column blocks of its input (the bias is one more block behind
// them), one block a wave, x one frame slice.  A wave keeps a 64 x 64 block of dW in 16 accumulators: per four frames it loads one dPre value
// per row tile (a quarter wave reads 16 consecutive floats of a frame) and ONE 16-byte piece of the input row -- columns 4 j .. 4 j + 3 of
// the block, so column tile c holds the block's columns 4 j + c, j = 0 .. 15 -- for sixteen MFMAs.
__global__ __launch_bounds__(256) void train_generic_wgrad_kernel(const GWgradArgs g) {
    const GItem it = g.items[blockIdx.x];
    const GGemm m = g.gm[it.gemm];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, quad = lane >> 4;
    const int64_t f0 = (int64_t)it.slice * g.slice_frames;
    const int64_t f1 = f0 + g.slice_frames < g.B ? f0 + g.slice_frames : g.B;
    const int nb0 = (m.in_w + 63) >> 6, nb1 = (m.y_w + 63) >> 6, nb = nb0 + nb1 + 1;
    const int nrt = m.nrt - 4 * it.rt < 4 ? m.nrt - 4 * it.rt : 4;           // row tiles of this item (it.rt counts 64-row groups)
    const float* dp = g.stash + m.dpre + 64 * it.rt + j;
    float* slab = g.slabs + (int64_t)it.slice * g.slab_stride;
    const int cb = it.cb0 + wave;                       // the wave's 64-column block
    if (cb < nb) {
        // the block's source: rows of `ld` floats at `base` with `w` valid columns, this lane's four from c4; output columns from ocol
        const bool bias = cb == nb0 + nb1, lab = !bias && cb >= nb0;
        const bool gather = g.row_index && (lab || m.in_kind == 0);
        const float* base = lab ? g.y : (m.in_kind == 0 ? g.x : g.stash + m.in_off);
        const int64_t ld = lab ? g.ldy : (m.in_kind == 0 ? g.ldx : (int64_t)g.S);
        const int w = bias ? 1 : (lab ? m.y_w : m.in_w), ocol = lab ? m.in_w : 0;
        const int c4 = 64 * (lab ? cb - nb0 : (bias ? 0 : cb)) + 4 * j;
        const int ntc = w - (c4 - 4 * j) < 4 ? w - (c4 - 4 * j) : 4;          // column tiles with a valid column
        const int nv = w - c4 < 0 ? 0 : (w - c4 > 4 ? 4 : w - c4);            // this lane's valid columns
        f32x4 acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the operands of the four frames from f: frame f + quad; past the slice: zeros
        auto load = [&](int64_t f, float (&a)[4], f32x4& b) __attribute__((always_inline)) {
            const int64_t fr = f + quad;
            const bool ok = fr < f1;
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = (ok && r < nrt) ? dp[fr * g.S + 16 * r] : 0.f;
            b = f32x4{0.f, 0.f, 0.f, 0.f};
            if (bias) {
                b[0] = 1.f;
            } else if (ok && nv > 0) {
                int64_t s = fr;
                if (gather) {
                    s = g.row_index[fr];
                    if (s < 0 || s >= g.row_count) s = 0;
                }
                const float* p = base + s * ld + c4;
                if (nv == 4) b = reinterpret_cast<const G4U*>(p)->v;
                else { b[0] = p[0]; if (nv > 1) b[1] = p[1]; if (nv > 2) b[2] = p[2]; }
            }
        };
        float a[4], an[4];
        f32x4 b, bn;
        load(f0, a, b);
        for (int64_t f = f0; f < f1; f += 4) {
            load(f + 4, an, bn);                        // requested before this round's MFMAs (all zeros past the slice)
            if (nrt == 4 && ntc == 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[c], acc[r][c], 0, 0, 0);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (r < nrt && c < ntc) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[c], acc[r][c], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = an[r];
            b = bn;
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 64 * it.rt + 16 * rt + 4 * quad + r;
                    if (rt >= nrt || row >= m.rows || c >= nv) continue;
                    if (bias) {
                        if (j == 0) slab[g.toff[m.bt] + row] = acc[rt][c][r];
                    } else {
                        slab[g.toff[m.wt] + (int64_t)row * m.cols + ocol + c4 + c] = acc[rt][c][r];
                    }
                }
    }
}

// the finalising workgroup of the apply and reduce launches: loss scalars, the classifier's counts, the M2_info fifth sum (256 threads,
// every thread calls)
__device__ __forceinline__ void finalize_step(const GApplyArgs& g, double (*red)[4]) {
    fused::finalize_losses(g.a, red);
    if (g.cnt_partials && threadIdx.x < 4) {            // integers, workgroup order
        long long c = 0;
        for (int i = 0; i < g.cnt_wgs; ++i) c += g.cnt_partials[4 * (int64_t)i + threadIdx.x];
        g.counts4[threadIdx.x] = c;
        if (g.cnt_accum) g.cnt_accum[threadIdx.x] += c;
    }
    if (g.kl_partials) {                                // the weighted KL term: one partial a thread, then waves in order, as below
        __syncthreads();                                // write_losses has read `red`
        double v = (int)threadIdx.x < g.a.npartials ? g.kl_partials[(int64_t)threadIdx.x * g.kl_stride] : 0.0;
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma clang fp contract(off)
            const float kc = (float)((red[0][0] + red[1][0] + red[2][0] + red[3][0]) / (double)g.a.B);
            const float wk = g.kl_w * kc;
            g.a.losses3[0] = g.a.losses3[1] + wk;                            // the objective: recon + w mean sum max(k, floor); [1], [2] stay raw
            if (g.a.info) g.a.losses3[3] = g.a.losses3[0] + g.a.losses3[4] - g.a.losses3[6];
            if (g.kl_accum) for (int q = 0; q < (g.a.info ? 8 : 3); ++q) g.kl_accum[q] += (double)g.a.losses3[q];
        }
    }
    if (g.v_partials) {                                 // one partial a thread: workgroup order within a wave's sum, waves in order
        static_assert(G_ROWS_GRID <= 256, "one thread of the finalising workgroup per rows workgroup");
        __syncthreads();                                // write_losses has read `red`
        double v = (int)threadIdx.x < g.a.npartials ? g.v_partials[threadIdx.x] : 0.0;
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float bv = (float)((red[0][0] + red[1][0] + red[2][0] + red[3][0]) / (double)g.a.B);
            const float aux_enc = g.a.beta * bv;
            g.a.losses3[3] = g.a.losses3[0] + g.a.losses3[4] - aux_enc;      // enc_loss = ELBO + classif_loss - beta V
            g.a.losses3[6] = aux_enc;
            if (g.v_accum) for (int q = 0; q < 8; ++q) g.v_accum[q] += (double)g.a.losses3[q];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// apply kernel: optimizer step, both packed copies, loss scalars (GApplyArgs: train_tables.hpp; the classifier step launches it with
// its confusion counts to finalise)
// CLIP (the guarded form, train_generic_apply_clipped_kernel): `ga` is g.a with the effective scale in gscale; the element arithmetic
// is the same code either way
template <bool CLIP>
__device__ __forceinline__ void apply_body(const GApplyArgs& g, const ApplyArgs& ga, double (*red)[4]) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < g.a.n_params) {
        int t = -1;
#pragma unroll
        for (int k = 0; k < G_NT; ++k)
            if (idx >= g.t[k].off && idx < g.t[k].off + (int64_t)g.t[k].rows * g.t[k].cols) t = k;
        if (t >= 0) {
            const GTensor d = g.t[t];
            float pi = g.a.p[idx];
            if (g.adam) {
                const float gi = fused::slab_sum_at(g.a, idx);
                float mi, vi;
                fused::adam_element(CLIP ? ga : g.a, pi, g.a.m[idx], g.a.v[idx], gi, mi, vi);
                g.a.p[idx] = pi; g.a.m[idx] = mi; g.a.v[idx] = vi;
            }
            const int i = (int)(idx - d.off);
            const int r = i / d.cols, c = i - r * d.cols;
            if (d.bias) {
                g.ws[d.f0 + d.roff + r] = pi;
            } else {
                if (c < d.split) g.ws[d.f0 + frag_pos(r + d.roff, c, d.kb0)] = pi;
                else g.ws[d.f1 + frag_pos(r + d.roff, c - d.split, d.kb1)] = pi;
                if (d.t0 >= 0 && c < d.tcmax) g.ws[d.t0 + frag_pos(c, r + d.tkoff, d.tkb)] = pi;
                if (d.tkb1 > 0 && c >= d.split) g.ws[d.t1 + frag_pos(c - d.split, r, d.tkb1)] = pi;
            }
        }
    }
    if (g.finalize && blockIdx.x == 0) finalize_step(g, red);
}

__global__ __launch_bounds__(256) void train_generic_apply_kernel(const GApplyArgs g) {
    __shared__ double red[4][4];
    apply_body<false>(g, g.a, red);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// global-norm clipping (GNormArgs / GClipArgs: train_tables.hpp).  The norm kernel: one workgroup a chunk of G_NORM_CHUNK floats.
__global__ __launch_bounds__(256) void train_generic_gradnorm_kernel(const GNormArgs g) {
    __shared__ double wsum[4];
    const int64_t base = (int64_t)blockIdx.x * G_NORM_CHUNK;
    f32x4 v[4];
    int i4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                       // every load before the first addition; n_params is a multiple of 4 below 2^31
        const int64_t i = base + ((int64_t)j * 256 + threadIdx.x) * 4;
        i4[j] = (int)i;
        v[j] = i < g.n_params ? *reinterpret_cast<const f32x4*>(g.flat + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int nv = 0;                                     // this piece's floats that belong to a tensor (the reduce kernel's rule)
#pragma unroll
        for (int k = 0; k < G_NT; ++k)
            if ((unsigned)(i4[j] - g.off[k]) < (unsigned)g.cnt[k]) nv = g.off[k] + g.cnt[k] - i4[j];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nv) s += (double)v[j][q] * (double)v[j][q];       // address order; the square is exact in double
    }
    s = wave_sum(s);                                    // lanes: the same tree on every lane
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g.partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];       // waves in order
}

// The guarded apply kernel.  Every workgroup forms the same s from the same partials in the same order (a few hundred doubles from L2),
// so every workgroup takes the same branch: return without a store (s not finite), or the element loop of the apply kernel under
// gscale_eff = fl32(grad_scale * coef).  coef == 1 leaves fl32(grad_scale): the unguarded kernel's bits.
__global__ __launch_bounds__(256) void train_generic_apply_clipped_kernel(const GApplyArgs g, const GClipArgs c) {
    __shared__ double red[4][4];
    __shared__ double wsum[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < c.nchunks; i += 256) s += c.partials[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    s = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const bool ok = isfinite(s);                        // (workgroup- and grid-uniform)
    const double total_norm = fabs(c.grad_scale) * sqrt(s);
    const double coef = ok ? fmin(1.0, c.max_norm / (total_norm + 1e-6)) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        c.norm2_out[0] = (float)total_norm;
        c.norm2_out[1] = (float)coef;
        if (!ok) *c.skipped += 1;                       // launches of a stream are ordered: no atomic needed
    }
    if (!ok) return;
    ApplyArgs ga = g.a;
    ga.gscale = (float)(c.grad_scale * coef);           // formed in double, rounded once
    apply_body<true>(g, ga, red);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// reduce kernel (GReduceArgs: train_tables.hpp): the frame-slice slabs of one micro-batch summed into the flat gradient accumulator, for
// gradient accumulation (reduce K times, apply once) and data parallelism (reduce, all-reduce, apply).  A thread owns four consecutive
// floats: every 16-byte slab load (and the accumulator's, when it is read) is issued before the first addition, the additions run in
// slab order -- fused::slab_sum_at's order, element for element --, then weight * sum (its own rounding: 1.0 leaves the bits alone),
// then accumulator + that, one 16-byte store.  No atomics, and no LDS outside the finalising workgroup: the same inputs give the same
// bits.  With accumulate 0 the accumulator is written and never read; the alignment gaps between tensors receive zeros in every call,
// whatever the slabs hold there.  The workgroup behind the last block of elements finalises the micro-batch's loss scalars.
template <int NS>
__device__ __forceinline__ f32x4 slab_sum4(const float* slabs, int64_t stride, int64_t i4) {
    f32x4 part[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) part[k] = *reinterpret_cast<const f32x4*>(slabs + k * stride + i4);       // independent loads
    f32x4 t = part[0];
#pragma unroll
    for (int k = 1; k < NS; ++k) t += part[k];                                                              // fixed order
    return t;
}

__global__ __launch_bounds__(256) void train_generic_reduce_kernel(const GReduceArgs g) {
    __shared__ double red[4][4];
    if (blockIdx.x == gridDim.x - 1) {                  // (workgroup-uniform)
        if (g.f.finalize) finalize_step(g.f, red);
        return;
    }
    const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= g.f.a.n_params) return;                   // (n_params is a multiple of 64)
    int nv = 0;                                         // this thread's floats that belong to a tensor; the others are the gap behind it
    const int i = (int)i4;                              // (the 26 tensors hold far fewer than 2^31 floats: 32-bit compares, a third of the ALU work)
#pragma unroll
    for (int k = 0; k < G_NT; ++k) {
        const int off = (int)g.f.t[k].off, n = g.f.t[k].rows * g.f.t[k].cols;     // (unused entries: n = 0)
        if ((unsigned)(i - off) < (unsigned)n) nv = off + n - i < 4 ? off + n - i : 4;
    }
    f32x4 old = {0.f, 0.f, 0.f, 0.f};
    if (g.accumulate) old = *reinterpret_cast<const f32x4*>(g.flat + i4);
    const float* sl = g.f.a.slabs;
    const int64_t st = g.f.a.slab_stride;
    const int ns = g.f.a.nslabs;
    f32x4 t;
    switch (ns) {                                       // the exact slab count (wave-uniform): no load beyond the slabs there are
#define DVAE_SLABS(n) case n: t = slab_sum4<n>(sl, st, i4); break;
        DVAE_SLABS(1) DVAE_SLABS(2) DVAE_SLABS(3) DVAE_SLABS(4) DVAE_SLABS(5) DVAE_SLABS(6) DVAE_SLABS(7) DVAE_SLABS(8)
        DVAE_SLABS(9) DVAE_SLABS(10) DVAE_SLABS(11) DVAE_SLABS(12) DVAE_SLABS(13) DVAE_SLABS(14) DVAE_SLABS(15) DVAE_SLABS(16)
#undef DVAE_SLABS
        default:
            t = *reinterpret_cast<const f32x4*>(sl + i4);
            for (int k = 1; k < ns; ++k) t += *reinterpret_cast<const f32x4*>(sl + k * st + i4);
    }
    f32x4 out;
    {
#pragma clang fp contract(off)
        const f32x4 wt = t * g.weight;
        out = g.accumulate ? old + wt : wt;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j >= nv) out[j] = 0.f;
    *reinterpret_cast<f32x4*>(g.flat + i4) = out;
}

int launch_wgrad_table(const GWgradArgs& g, int n_items, hipStream_t s) {
    hipLaunchKernelGGL(train_generic_wgrad_kernel, dim3((unsigned)n_items), dim3(256), 0, s, g);
    DVAE_LAUNCH_OK("train_generic_wgrad_kernel");
    return 0;
}

int launch_apply_table(const GApplyArgs& g, hipStream_t s) {
    const int64_t blocks = g.a.n_params > 0 ? (g.a.n_params + 255) / 256 : 1;
    hipLaunchKernelGGL(train_generic_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g);
    DVAE_LAUNCH_OK("train_generic_apply_kernel");
    return 0;
}

int launch_reduce_table(const GReduceArgs& g, hipStream_t s) {
    DVAE_CHECK_ARG(g.f.a.n_params >= 0 && g.f.a.n_params < ((int64_t)1 << 31) && g.f.a.n_params % 64 == 0,
                   "train_generic_reduce_kernel: %lld parameters (a multiple of 64 below 2^31: the kernel indexes tensors in 32 bits)", (long long)g.f.a.n_params);
    const int64_t blocks = (g.f.a.n_params / 4 + 255) / 256 + 1;         // + the finalising workgroup
    hipLaunchKernelGGL(train_generic_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g);
    DVAE_LAUNCH_OK("train_generic_reduce_kernel");
    return 0;
}

int launch_apply_clipped_table(const GApplyArgs& g, const GClipHost& h, hipStream_t s) {
    const int64_t P = g.a.n_params;
    DVAE_CHECK_ARG(P >= 1 && P < ((int64_t)1 << 31) - G_NORM_CHUNK && P % 64 == 0 && g.a.nslabs == 1,
                   "train_generic_gradnorm_kernel: %lld parameters (a multiple of 64 below 2^31: the kernel indexes tensors in 32 bits)", (long long)P);
    GNormArgs n;
    memset(&n, 0, sizeof(n));
    n.flat = g.a.slabs; n.n_params = P; n.partials = (double*)h.scratch;
    for (int k = 0; k < G_NT; ++k) { n.off[k] = (int32_t)g.t[k].off; n.cnt[k] = g.t[k].rows * g.t[k].cols; }
    const int64_t chunks = gradnorm_chunks(P);
    hipLaunchKernelGGL(train_generic_gradnorm_kernel, dim3((unsigned)chunks), dim3(256), 0, s, n);
    DVAE_LAUNCH_OK("train_generic_gradnorm_kernel");
    GClipArgs c;
    memset(&c, 0, sizeof(c));
    c.partials = (const double*)h.scratch; c.nchunks = (int)chunks; c.grad_scale = h.grad_scale; c.max_norm = h.max_norm;
    c.norm2_out = h.norm2_out; c.skipped = h.skipped;
    hipLaunchKernelGGL(train_generic_apply_clipped_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, g, c);
    DVAE_LAUNCH_OK("train_generic_apply_clipped_kernel");
    return 0;
}

int check_clip_args(const char* who, const float* flat, const GClipHost& h) {
    DVAE_CHECK_ARG(h.scratch && h.norm2_out && h.skipped, "%s: null pointer", who);
    DVAE_CHECK_ARG(h.max_norm > 0.0, "%s: max_norm %g (a positive number; +inf clips nothing)", who, h.max_norm);      // (a NaN fails the comparison)
    DVAE_CHECK_ARG(((uintptr_t)flat & 15) == 0 && ((uintptr_t)h.scratch & 7) == 0,
                   "%s: the flat gradient must be 16-byte aligned and the scratch buffer 8-byte aligned", who);
    return 0;
}

int check_reduce_args(const char* who, const void* ws, const float* flat, int accumulate, float weight) {
    DVAE_CHECK_ARG(ws && flat, "%s: null pointer", who);
    DVAE_CHECK_ARG(((uintptr_t)flat & 15) == 0, "%s: the flat gradient must be 16-byte aligned", who);
    DVAE_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate %d (0: overwrite the flat gradient, 1: add to it)", who, accumulate);
    DVAE_CHECK_ARG(isfinite(weight), "%s: the weight of the micro-batch is not finite", who);
    return 0;
}

int check_apply_flat_args(const char* who, const float* params, const float* m, const float* v, const void* ws, const float* flat, int step,
                          double lr, double grad_scale) {
    DVAE_CHECK_ARG(params && m && v && ws && flat, "%s: null pointer", who);
    DVAE_CHECK_ARG(step >= 1, "%s: step %d (1-based)", who, step);
    DVAE_CHECK_ARG(isfinite(grad_scale) && isfinite(lr), "%s: grad_scale / lr is not finite", who);
    return 0;
}

int raise_lds_limit(const void* kernel, const char* name, int64_t lds_bytes, bool (&done)[64]) {
    if (lds_bytes > G_LDS_MAX) { set_error("%s: %lld B of LDS needed, %lld available", name, (long long)lds_bytes, (long long)G_LDS_MAX); return DVAE_E_UNSUPPORTED; }
    if (lds_bytes <= 64 * 1024) return 0;
    int dev = 0;
    DVAE_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !done[dev]) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G_LDS_MAX);
        if (e != hipSuccess) {
            (void)hipGetLastError();                    // reported here, not left for the caller's next runtime call
            set_error("hipFuncSetAttribute(%s, %lld B LDS): %s", name, (long long)G_LDS_MAX, hipGetErrorString(e));
            return (int)e;
        }
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
    return 0;
}

}  // namespace tg
}  // namespace dvae

extern "C" int64_t dvae_train_gradnorm_scratch_bytes(int64_t n_params) {
    using namespace dvae;
    using namespace dvae::tg;
    if (n_params < 1 || n_params >= ((int64_t)1 << 31) - G_NORM_CHUNK) {
        set_error("train_gradnorm_scratch_bytes: n_params %lld (the plan's n_params: at least 1, below 2^31)", (long long)n_params);
        return 0;
    }
    return gradnorm_chunks(n_params) * (int64_t)sizeof(double);
}

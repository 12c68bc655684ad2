// What the fused train steps of any covered size share (train_generic.hip: the M1 / M2 step, dvae_train_generic_*; train_classifier.hip:
// the label classifier's step, dvae_train_clf_*; train_info.hip: the M2_info step, dvae_train_info_*; include/dvae_train.h): the packed
// weight copies in fragment order and the product that reads them, the tables the weight-gradient and optimizer launches read, and the
// launches of those kernels, which live in train_tables.hip and serve all three steps.  The host code the three steps run around these
// launches is train_step_host.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "common.hpp"
#include "apply_types.hpp"

namespace dvae {
namespace tg {

constexpr int GT = 16;                          // frames per tile
constexpr int GX = 513, GXP = 528, GKX = GXP / 16;
constexpr int G_HMAX = 512, G_ZMAX = 128;       // the limits of dvae_mcem_plan_dims / mlp_generic.hip
constexpr int G_NT = 26, G_NG = 13;             // tensors (state_dict order), weight matrices: the sizes of the tables (M2_info fills them: train_info.hip; M1 / M2 use 14 / 7, the classifier 6 / 3)
constexpr int G_KERNARG_MAX = 4096;             // bytes the runtime takes as the arguments of one kernel
constexpr int G_ROWS_GRID = 256, G_MAX_SLICES = 16;   // one rows workgroup per compute unit, the other tiles strided over; slabs the apply kernel sums

inline int up16(int v) { return (v + 15) / 16 * 16; }
inline int64_t al64(int64_t v) { return (v + 63) / 64 * 64; }        // floats: 256 bytes
inline int64_t al256(int64_t v) { return (v + 255) / 256 * 256; }
struct __attribute__((packed, aligned(4))) G4U { f32x4 v; };      // 16 bytes at dword alignment (rows of 513 floats)

// element (row, k) of a matrix packed in fragment order [row tile][k block of 16][lane][4] with kb k blocks (mlp_generic.hip: lane l
// holds row l & 15, inputs 16 b + 4 i + (l >> 4))
__host__ __device__ inline int64_t frag_pos(int row, int k, int kb) {
    return ((((int64_t)(row >> 4) * kb + (k >> 4)) * 64 + (((k & 3) << 4) | (row & 15))) << 2) + ((k & 15) >> 2);
}

// acc += W[row tile] (16 x 16 kb) * act (16 kb x 16 frames): W in fragment order, act in LDS as [k][16]
__device__ __forceinline__ f32x4 tg_gemm(f32x4 acc, const float* __restrict__ wt, int kb, const float* act, int lane) {
    // k ascending, four k blocks a round with the next round's fragments requested before this round's MFMAs: the loads are L2 hits of
    // several hundred cycles and a workgroup may be alone on its CU
    const f32x4* w = reinterpret_cast<const f32x4*>(wt) + lane;
    auto step = [&](const f32x4& a, int b) __attribute__((always_inline)) {
        const float* bp = act + b * 256 + lane;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bp[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bp[64], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bp[128], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bp[192], acc, 0, 0, 0);
    };
    const int kb4 = kb & ~3;
    if (kb4) {
        f32x4 c0 = w[0], c1 = w[64], c2 = w[128], c3 = w[192];
        for (int b = 0; b < kb4; b += 4) {
            f32x4 n0 = c0, n1 = c1, n2 = c2, n3 = c3;
            if (b + 4 < kb4) {
                const f32x4* wn = w + (int64_t)(b + 4) * 64;
                n0 = wn[0]; n1 = wn[64]; n2 = wn[128]; n3 = wn[192];
            }
            step(c0, b); step(c1, b + 1); step(c2, b + 2); step(c3, b + 3);
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        }
    }
    for (int b = kb4; b < kb; ++b) step(w[(int64_t)b * 64], b);
    return acc;
}

// where a parameter lives in the packed copies
struct GTensor {
    int64_t off;
    int32_t rows, cols;
    int64_t f0, f1;                 // forward copies: columns < split -> f0 (kb0 k blocks), the others -> f1 (kb1); a bias: f0 = its padded copy
    int32_t kb0, kb1, split, roff;  // row r -> r + roff
    int64_t t0;                     // transposed copy, -1 = none: element (r, c < tcmax) -> row c, input r + tkoff
    int32_t tkb, tkoff, tcmax, bias;
    int64_t t1;                     // transposed copy of the columns >= split, tkb1 = 0: none: element (r, c) -> row c - split, input r
    int32_t tkb1, pad1;
};

// one weight matrix of the weight-gradient launch: dW = dPre^T [in | y] and db = dPre^T 1 over the frames
struct GGemm {
    int64_t dpre;                   // stash column of dPre
    int64_t in_off;                 // stash column of the input (in_kind 1)
    int32_t nrt, rows, wt, bt;      // output tiles, rows, weight / bias tensor
    int32_t in_kind, in_w, y_w, cols;   // in_kind 0: the caller's x; in_w valid input columns; y_w label columns behind them (0: none)
};

struct GItem { int32_t gemm, rt, slice, cb0; };      // rt: the 64-row group of the matrix; cb0: the first of its four 64-column blocks

// items of one matrix and one frame slice: 64-row groups x groups of four 64-column blocks (input, labels, one block for the bias)
inline int gemm_col_groups(const GGemm& m) { return ((m.in_w + 63) / 64 + (m.y_w + 63) / 64 + 1 + 3) / 4; }
inline int gemm_items(const GGemm& m) { return (m.nrt + 3) / 4 * gemm_col_groups(m); }

// the item table of a weight-gradient launch: per frame slice, the matrices in `order` (the widest inputs first: their items run longest)
inline std::vector<GItem> make_items(const GGemm* gm, const int* order, int ng, int nslices) {
    std::vector<GItem> items;
    for (int sl = 0; sl < nslices; ++sl)
        for (int gi = 0; gi < ng; ++gi)
            for (int rt = 0; rt < (gm[order[gi]].nrt + 3) / 4; ++rt)
                for (int cg = 0; cg < gemm_col_groups(gm[order[gi]]); ++cg) items.push_back(GItem{order[gi], rt, sl, 4 * cg});
    return items;
}

// frame slices of the weight-gradient reduction for `row_tiles` items a slice: about three workgroups a compute unit, at least 64 frames
// a slice (hint > 0: as asked); -> frames of a slice (a multiple of 16), slices
inline void choose_slices(int64_t B, int row_tiles, int ksplit_hint, int64_t& slice_frames, int& nslices) {
    int64_t ks = ksplit_hint;
    if (ks <= 0) {
        ks = (768 + row_tiles - 1) / row_tiles;
        if (ks > B / 64) ks = B / 64;
    }
    if (ks > G_MAX_SLICES) ks = G_MAX_SLICES;
    if (ks < 1) ks = 1;
    slice_frames = ((B + ks - 1) / ks + 15) / 16 * 16;
    nslices = (int)((B + slice_frames - 1) / slice_frames);
}

// weight-gradient kernel (train_tables.hip: train_generic_wgrad_kernel)
struct GWgradArgs {
    const float* x; int64_t ldx;
    const float* y; int64_t ldy;
    const int64_t* row_index; int64_t row_count;
    const float* stash; float* slabs; int64_t slab_stride;
    int64_t B, slice_frames;
    const GItem* items;
    int S;
    GGemm gm[G_NG];
    int64_t toff[G_NT];
};

// apply kernel (train_tables.hip: train_generic_apply_kernel): optimizer step, both packed copies, loss scalars; with `cnt_partials`
// also the confusion counts of the classifier step: [cnt_wgs][4] integers summed in workgroup order into counts4 (and added to cnt_accum);
// with `v_partials` (the M2_info step whose adversarial term is not a cross entropy, train_info.hip) a fifth loss sum per rows workgroup
// (a.npartials <= G_ROWS_GRID of them): aux_enc_loss = beta V replaces beta BCE in the loss scalars, and the running sums go to v_accum
// (a.accum is then null); with `kl_partials` (the M1 / M2 and M2_info steps under a weighted KL term: dvae_train_generic_plan_t.kl_weight /
// kl_floor other than 1 / 0) one more loss sum per rows workgroup, at kl_partials[i * kl_stride]: the KL elements clamped from below at
// kl_floor.  The ELBO slot becomes fl32(recon + fl32(kl_w * mean)) -- and enc_loss is rebuilt on it --, the recon and KL slots stay the
// raw means, and the running sums go to kl_accum (a.accum is then null; where v_partials is set too, v_accum takes them behind both).
// Null -- every other caller -- leaves the finalising workgroup's arithmetic as it is.
struct GApplyArgs {
    fused::ApplyArgs a;
    GTensor t[G_NT];
    float* ws;
    int adam, finalize;
    const long long* cnt_partials; int cnt_wgs;
    long long* counts4; long long* cnt_accum;
    const double* v_partials; double* v_accum;
    const double* kl_partials; double* kl_accum;
    int kl_stride; float kl_w;
};

// reduce kernel (train_tables.hip: train_generic_reduce_kernel), between _grads and _apply_flat: flat = [flat +] weight * (the slabs of
// f.a summed in slab order), zeros in the alignment gaps between the tensors of f.t; one more workgroup finalises the micro-batch's loss
// scalars (and counts) exactly as the apply kernel's finalising workgroup does (f.adam is unused, f.finalize 1)
struct GReduceArgs {
    GApplyArgs f;
    float* flat;
    int accumulate;
    float weight;
};

// Global-norm clipping of the flat gradient (include/dvae_train.h: dvae_train_*_apply_flat_clipped): two launches, no host round trip.
//   * norm kernel (train_tables.hip: train_generic_gradnorm_kernel): workgroup c owns chunk c = floats [c G_NORM_CHUNK, (c + 1)
//     G_NORM_CHUNK) of the flat gradient, whatever the grid of any other launch or the part: a thread loads four 16-byte pieces,
//     squares and adds them in double in address order (a float32 square is exact in double), then lanes (xor butterfly: every lane
//     forms the same tree), waves in order, and partials[c] is written.  Floats that belong to no tensor (the alignment gaps) count
//     as zero whatever they hold.  No atomics: the same gradient gives the same partials on every run and every rank.
//   * the guarded apply kernel (train_generic_apply_clipped_kernel) sums the partials in a fixed order too -- thread t of every
//     workgroup takes chunks t, t + 256, ... ascending, then lanes, then waves -- and forms total_norm, coef and the effective scale.
constexpr int G_NORM_CHUNK = 4096;              // floats of a chunk: 256 threads x 4 loads x 4 floats
struct GNormArgs {
    const float* flat; int64_t n_params;
    double* partials;
    int32_t off[G_NT], cnt[G_NT];               // the tensors (unused entries: cnt 0)
};
struct GClipArgs {
    const double* partials; int nchunks;
    double grad_scale, max_norm;
    float* norm2_out;                           // [total_norm, coef]
    int32_t* skipped;                           // + 1 when the sum of squares is not finite (the update is then not made)
};

static_assert(sizeof(GWgradArgs) <= G_KERNARG_MAX && sizeof(GApplyArgs) <= G_KERNARG_MAX && sizeof(GReduceArgs) <= G_KERNARG_MAX &&
              sizeof(GApplyArgs) + sizeof(GClipArgs) <= G_KERNARG_MAX && sizeof(GNormArgs) <= G_KERNARG_MAX,
              "the tables travel as kernel arguments");

// the launches, for a caller that has filled the tables (unused entries zeroed): n_items workgroups; one thread a parameter of
// g.a.n_params (0: one workgroup that only finalises); one thread per four floats of g.f.a.n_params and one finalising workgroup
int launch_wgrad_table(const GWgradArgs& g, int n_items, hipStream_t s);
int launch_apply_table(const GApplyArgs& g, hipStream_t s);
int launch_reduce_table(const GReduceArgs& g, hipStream_t s);
// the norm launch over g.a.slabs (the flat gradient: g.a.nslabs 1) into h.scratch, then the guarded apply launch with the caller's
// grad_scale as a double (g.a.gscale is not read)
struct GClipHost { double grad_scale, max_norm; void* scratch; float* norm2_out; int32_t* skipped; };
int launch_apply_clipped_table(const GApplyArgs& g, const GClipHost& h, hipStream_t s);
inline int64_t gradnorm_chunks(int64_t n_params) { return (n_params + G_NORM_CHUNK - 1) / G_NORM_CHUNK; }
// what the _apply_flat_clipped entry points refuse on top of check_apply_flat_args
int check_clip_args(const char* who, const float* flat, const GClipHost& h);
// what the _reduce / _apply_flat entry points of the three steps refuse before anything touches the device (0: fine)
int check_reduce_args(const char* who, const void* ws, const float* flat, int accumulate, float weight);
int check_apply_flat_args(const char* who, const float* params, const float* m, const float* v, const void* ws, const float* flat, int step,
                          double lr, double grad_scale);
// dynamic LDS past the default 64 KB limit for a rows kernel: raised once per device (done: the caller's flags, one per device)
int raise_lds_limit(const void* kernel, const char* name, int64_t lds_bytes, bool (&done)[64]);
constexpr int64_t G_LDS_MAX = 160 * 1024;

}  // namespace tg
}  // namespace dvae

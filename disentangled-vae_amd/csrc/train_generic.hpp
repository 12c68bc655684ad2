// Plain structs of the generic fused train step (train_generic.hip; include/dvae_train.h: dvae_train_generic_*): the packed weight
// copies, the stash of one frame, the workspace, and the tables the weight-gradient and optimizer launches read.
#pragma once
#include <stdint.h>

namespace dvae {
namespace tg {

constexpr int GT = 16;                          // frames per tile
constexpr int GX = 513, GXP = 528, GKX = GXP / 16;
constexpr int G_HMAX = 512, G_ZMAX = 128;       // the limits of dvae_mcem_plan_dims / mlp_generic.hip
constexpr int G_NT = 14, G_NG = 7;              // tensors (state_dict order), weight matrices
constexpr int G_ROWS_GRID = 256, G_MAX_SLICES = 16;   // one rows workgroup per compute unit, the other tiles strided over; slabs the apply kernel sums

// element (row, k) of a matrix packed in fragment order [row tile][k block of 16][lane][4] with kb k blocks (mlp_generic.hip: lane l
// holds row l & 15, inputs 16 b + 4 i + (l >> 4))
__host__ __device__ inline int64_t frag_pos(int row, int k, int kb) {
    return ((((int64_t)(row >> 4) * kb + (k >> 4)) * 64 + (((k & 3) << 4) | (row & 15))) << 2) + ((k & 15) >> 2);
}

struct GLayout {
    int y, z, h1, h2, yp, zp, h1p, h2p, hm;     // sizes and their multiples of 16 (yp 0 without labels); hm = max(h1p, h2p, zp)
    // packed copies, float offsets from the start of the workspace: forward [out tile][k block], x / z block and label block apart;
    // the heads are one matrix (mu rows 0 .. z - 1, log_var rows zp .. zp + z - 1)
    int64_t W1x, W1y, W2, Wh, D1z, D1y, D2, D3;
    int64_t D3T, D2T, D1zT, WhT, W2T;           // the transposed copies of the backward-data products
    int64_t b1, b2, bh, bd1, bd2, bd3;          // zero-padded biases
    int64_t wpack_elems;
    // the stash of one frame (floats): layer inputs, then the pre-activation gradients
    int S, s_h1e, s_h2e, s_z, s_d1, s_d2, s_pe1, s_pe2, s_ph, s_pd1, s_pd2, s_da;
    // workspace (bytes)
    int64_t o_items, o_partials, o_stash, o_grads, ws_bytes;
    int64_t B, Bp, tiles, rows_grid, slice_frames, n_params;
    int nslices, n_items;
    int64_t lds_bytes;
    int64_t toff[G_NT];
    int trows[G_NT], tcols[G_NT];
};

// where a parameter lives in the packed copies
struct GTensor {
    int64_t off;
    int32_t rows, cols;
    int64_t f0, f1;                 // forward copies: columns < split -> f0 (kb0 k blocks), the others -> f1 (kb1); a bias: f0 = its padded copy
    int32_t kb0, kb1, split, roff;  // row r -> r + roff
    int64_t t0;                     // transposed copy, -1 = none: element (r, c < tcmax) -> row c, input r + tkoff
    int32_t tkb, tkoff, tcmax, bias;
};

// one weight matrix of the weight-gradient launch: dW = dPre^T [in | y] and db = dPre^T 1 over the frames
struct GGemm {
    int64_t dpre;                   // stash column of dPre
    int64_t in_off;                 // stash column of the input (in_kind 1)
    int32_t nrt, rows, wt, bt;      // output tiles, rows, weight / bias tensor
    int32_t in_kind, in_w, y_w, cols;   // in_kind 0: the caller's x; in_w valid input columns; y_w label columns behind them (0: none)
};

struct GItem { int32_t gemm, rt, slice, cb0; };      // rt: the 64-row group of the matrix; cb0: the first of its four 64-column blocks

}  // namespace tg
}  // namespace dvae

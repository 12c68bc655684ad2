// The fused train step for M2_info models of ANY covered size, exact fp32, THREE launches per step whatever the geometry and the batch
// (include/dvae_train.h: dvae_train_info_*; disentangled-vae_amd/trainer_info.py).  M2_info is the reference's DeepGenerativeModel_v5
// (packages/models/models.py:390-444) under the loop body of scripts/training_M2_info_vad.py:159-198:
//   encoder 513 -> h1 -> h2 -> {mu, log_var} (tanh), decoder [z | y] -> h2 -> h1 -> 513 (tanh, exp), classifier 513 -> h1 -> h2 -> y and
//   auxiliary net z -> h1 -> h2 -> y (relu, relu, sigmoid): 26 tensors, 13 weight matrices;
//   enc_loss = ELBO + alpha BCE(clf(x), y) - beta BCE(aux(z), y) into every enc_dec_clf tensor (the -beta term through z into the
//   encoder), aux_loss = gamma BCE(aux(z.detach()), y); the auxiliary tensors are stepped with (gamma - beta) dBCE, because the
//   script never zeroes what enc_loss.backward() left in them; one Adam update over all 26 tensors at the same step count.
// The resident step (train_rows*.hip) is written for 513-128-128-16 / y 1 and stays the default there; this file serves every other size
// within x 513, y_dim 1..513, h1 / h2 1..512, z 1..128 -- and the reference geometry too when asked.
//
// The design is train_generic.hip's and train_classifier.hip's, composed; the weight-gradient and apply kernels of train_tables.hip serve
// this step (one launch each), and the host path around the launches is train_step_host.hpp's (IStep below describes this step to it):
//   * rows kernel (here): 256 threads own a tile of 16 frames; products on v_mfma_f32_16x16x4_f32 from packed copies in fragment order,
//     zero-padded to multiples of 16 (tg_gemm).  LDS holds the tiles of the M1 / M2 kernel and no more -- X [528][16], Y [yp][16], A and
//     Bf [hm][16] with hm = max(h1p, h2p, zp), C [3 zp][16]: 154 KB at 512 / 512 / z 128 / y 513, sized from the dims at launch -- so the
//     two side nets have no tiles of their own: the phases reuse them, and operands are re-read (x from the caller's memory through the
//     gather table, z and the first auxiliary layer from the stash) instead of kept.  Phases of a tile, a barrier between each:
//       1. classifier: c1 = relu(x) -> A, c2 -> Bf, p = sigmoid, BCE; dpre_o (weight alpha / B) takes the place of x in X; dpre_c2 -> Bf;
//          dpre_c1 -> stash only.  x is loaded again.
//       2. encoder forward: h1e -> A, h2e -> Bf, heads -> C, z -> Bf (and always to the stash), the KL terms.
//       3. decoder forward: d1 -> A, d2 -> Bf, the Itakura-Saito sum, d loss / d a -> X; decoder backward: dpre_d2 -> Bf, dpre_d1 -> A.
//       4. auxiliary net (X and Bf are free, A keeps dpre_d1): z from the stash -> Bf, a1 = relu -> X, a2 -> Bf, p = sigmoid, BCE;
//          the pre-activation gradients are formed ONCE at weight 1 / B: dpre_ao -> X, dpre_a2 -> Bf, dpre_a1 -> X (the relu mask of a1
//          from this thread's own stash entry).  They are stashed times (gamma - beta) for the weight gradients.
//       5. dz = dpre_d1 D1[:, :z] - beta (dpre_a1 Wa1): beta = 0 divides nothing; d mu, d log_var -> C; encoder backward as in the
//          M1 / M2 kernel (tanh' from the stash).
//     Every layer input and every pre-activation gradient goes to the stash ([frame][S] floats, 16-byte stores from the accumulators).
//     Frames past B carry zero pre-activation gradients and finite activations; padded units carry zeros throughout.  The four loss
//     sums (Itakura-Saito, KL, BCE of the classifier, BCE of the auxiliary net) per workgroup in double, waves in order.
//   * weight-gradient kernel: one launch for the thirteen matrices and their biases; the first layers of encoder and classifier read the
//     caller's x, decoder layer 1 reads [z | y].  One slab per frame slice: no atomics on floats, the same inputs give the same bits.
//   * apply kernel: slab sums in slab order, adam_element, both packed copies, the eight loss scalars of the resident step
//     (apply_common.hpp: write_losses with `info`).
//   * 64-bit indexing throughout; a gather index outside [0, row_count) is never dereferenced (row 0 instead, counted).
// Two options (dvae_train_info_plan_mode, known at plan time: stash and workspace depend on them) give the loop body of
// scripts/training_M2_info_vad_pretrain.py:162-200: the decoder fed [z | clf(x)], and binary_cross_entropy_v2 / _v3 of aux(z) as the
// encoder's adversarial term.  They are template parameters of the rows kernel (see there); the instantiation <false, 0> is the step
// above, statement for statement.  LDS is the same at every mode: p_c lives in the label tile Y, and the labels are read again through
// the gather table where a later phase needs them.  The weight-gradient launch reads [z | p_c] of decoder layer 1 from the stash, where
// the rows kernel lays them side by side; the apply kernel keeps one more packed copy, the label block of that layer transposed.
#include <math.h>
#include <vector>
#include "common.hpp"
#include "../../include/dvae_train.h"
#include "train_step_host.hpp"

namespace dvae {
namespace ti {

using namespace dvae::tg;
using fused::ApplyArgs;

constexpr int I_NT = 26, I_NG = 13;
constexpr int I_LAUNCHES = 3;
static_assert(I_NT <= G_NT && I_NG <= G_NG, "the tables of train_tables.hpp hold this step");

struct ILayout {
    int y, z, h1, h2, yp, zp, h1p, h2p, hm;     // sizes and their multiples of 16; hm = max(h1p, h2p, zp)
    // packed copies, float offsets from the start of the workspace (fragment order, train_tables.hpp); the heads are one matrix
    int64_t W1, W2, Wh, D1z, D1y, D2, D3, D3T, D2T, D1zT, WhT, W2T;       // the VAE: forward copies, then the transposed ones
    int64_t C1, C2, Co, CoT, C2T;                                        // classifier on x
    int64_t A1, A2, Ao, AoT, A2T, A1T;                                   // auxiliary net on z
    int64_t b1, b2, bh, bd1, bd2, bd3, bc1, bc2, bco, ba1, ba2, bao;     // zero-padded biases
    int64_t D1yT;                                                        // the label block of decoder layer 1, transposed (dec_label "classifier" only)
    int64_t wpack_elems;
    // the stash of one frame (floats): layer inputs, then the pre-activation gradients
    int S, s_h1e, s_h2e, s_z, s_d1, s_d2, s_pe1, s_pe2, s_ph, s_pd1, s_pd2, s_da;
    int s_c1, s_c2, s_pc1, s_pc2, s_pco, s_a1, s_a2, s_pa1, s_pa2, s_pao;
    int s_zc;                                                            // [z | p_c], the input of decoder layer 1 (dec_label "classifier" only)
    int mode;                                                            // DVAE_INFO_* bits
    int64_t o_items, o_partials, o_stash, o_grads, ws_bytes;             // workspace (bytes)
    int64_t B, Bp, tiles, rows_grid, slice_frames, n_params;
    int nslices, n_items;
    int64_t lds_bytes;
    int64_t toff[I_NT];
    int trows[I_NT], tcols[I_NT];
};

constexpr int MODE_AUX = DVAE_INFO_AUX_UNIFORM | DVAE_INFO_AUX_ENTROPY, MODE_ALL = DVAE_INFO_DEC_CLASSIFIER | MODE_AUX;
static bool mode_ok(int mode) { return (mode & ~MODE_ALL) == 0 && (mode & MODE_AUX) != MODE_AUX; }

static bool dims_ok(int y, int z, int h1, int h2) {
    return y >= 1 && y <= GX && h1 >= 1 && h1 <= G_HMAX && h2 >= 1 && h2 <= G_HMAX && z >= 1 && z <= G_ZMAX;
}

static void make_gemms(const ILayout& L, GGemm* G) {
    auto set = [&](int i, int dpre, int nrt, int rows, int kind, int in_off, int in_w, int y_w) {
        GGemm& m = G[i];
        memset(&m, 0, sizeof(m));
        m.dpre = dpre; m.nrt = nrt; m.rows = rows; m.wt = 2 * i; m.bt = 2 * i + 1; m.in_kind = kind; m.in_off = in_off; m.in_w = in_w; m.y_w = y_w;
        m.cols = in_w + y_w;
    };
    set(0, L.s_pe1, L.h1p / 16, L.h1, 0, 0, GX, 0);                     // the encoder sees x alone
    set(1, L.s_pe2, L.h2p / 16, L.h2, 1, L.s_h1e, L.h1, 0);
    set(2, L.s_ph, L.zp / 16, L.z, 1, L.s_h2e, L.h2, 0);
    set(3, L.s_ph + L.zp, L.zp / 16, L.z, 1, L.s_h2e, L.h2, 0);
    if (L.mode & DVAE_INFO_DEC_CLASSIFIER) set(4, L.s_pd1, L.h2p / 16, L.h2, 1, L.s_zc, L.z + L.y, 0);      // [z | p_c] lies in the stash
    else set(4, L.s_pd1, L.h2p / 16, L.h2, 1, L.s_z, L.z, L.y);
    set(5, L.s_pd2, L.h1p / 16, L.h1, 1, L.s_d1, L.h2, 0);
    set(6, L.s_da, GKX, GX, 1, L.s_d2, L.h1, 0);
    set(7, L.s_pc1, L.h1p / 16, L.h1, 0, 0, GX, 0);
    set(8, L.s_pc2, L.h2p / 16, L.h2, 1, L.s_c1, L.h1, 0);
    set(9, L.s_pco, L.yp / 16, L.y, 1, L.s_c2, L.h2, 0);
    set(10, L.s_pa1, L.h1p / 16, L.h1, 1, L.s_z, L.z, 0);
    set(11, L.s_pa2, L.h2p / 16, L.h2, 1, L.s_a1, L.h1, 0);
    set(12, L.s_pao, L.yp / 16, L.y, 1, L.s_a2, L.h2, 0);
}

static ILayout make_layout(int y, int z, int h1, int h2, int64_t B, int ksplit_hint, int mode) {
    ILayout L;
    memset(&L, 0, sizeof(L));
    L.mode = mode;
    const bool dec_clf = (mode & DVAE_INFO_DEC_CLASSIFIER) != 0, aux_v = (mode & MODE_AUX) != 0;
    L.y = y; L.z = z; L.h1 = h1; L.h2 = h2;
    L.yp = up16(y); L.zp = up16(z); L.h1p = up16(h1); L.h2p = up16(h2);
    L.hm = L.h1p > L.h2p ? L.h1p : L.h2p;
    if (L.zp > L.hm) L.hm = L.zp;
    // parameters: DeepGenerativeModel_v5.state_dict() order, 256-byte aligned
    const int rows[I_NT] = {h1, h1, h2, h2, z, z, z, z, h2, h2, h1, h1, GX, GX, h1, h1, h2, h2, y, y, h1, h1, h2, h2, y, y};
    const int cols[I_NT] = {GX, 1, h1, 1, h2, 1, h2, 1, z + y, 1, h2, 1, h1, 1, GX, 1, h1, 1, h2, 1, z, 1, h1, 1, h2, 1};
    int64_t o = 0;
    for (int t = 0; t < I_NT; ++t) {
        L.toff[t] = o; L.trows[t] = rows[t]; L.tcols[t] = cols[t];
        o = al64(o + (int64_t)rows[t] * cols[t]);
    }
    L.n_params = o;
    // packed copies
    o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o = al64(o + n); return at; };
    L.W1 = take((int64_t)L.h1p * GXP); L.W2 = take((int64_t)L.h2p * L.h1p); L.Wh = take((int64_t)2 * L.zp * L.h2p);
    L.D1z = take((int64_t)L.h2p * L.zp); L.D1y = take((int64_t)L.h2p * L.yp);
    L.D2 = take((int64_t)L.h1p * L.h2p); L.D3 = take((int64_t)GXP * L.h1p);
    L.D3T = take((int64_t)L.h1p * GXP); L.D2T = take((int64_t)L.h2p * L.h1p); L.D1zT = take((int64_t)L.zp * L.h2p);
    L.WhT = take((int64_t)L.h2p * 2 * L.zp); L.W2T = take((int64_t)L.h1p * L.h2p);
    L.C1 = take((int64_t)L.h1p * GXP); L.C2 = take((int64_t)L.h2p * L.h1p); L.Co = take((int64_t)L.yp * L.h2p);
    L.CoT = take((int64_t)L.h2p * L.yp); L.C2T = take((int64_t)L.h1p * L.h2p);
    L.A1 = take((int64_t)L.h1p * L.zp); L.A2 = take((int64_t)L.h2p * L.h1p); L.Ao = take((int64_t)L.yp * L.h2p);
    L.AoT = take((int64_t)L.h2p * L.yp); L.A2T = take((int64_t)L.h1p * L.h2p); L.A1T = take((int64_t)L.zp * L.h1p);
    L.b1 = take(L.h1p); L.b2 = take(L.h2p); L.bh = take(2 * L.zp); L.bd1 = take(L.h2p); L.bd2 = take(L.h1p); L.bd3 = take(GXP);
    L.bc1 = take(L.h1p); L.bc2 = take(L.h2p); L.bco = take(L.yp); L.ba1 = take(L.h1p); L.ba2 = take(L.h2p); L.bao = take(L.yp);
    if (dec_clf) L.D1yT = take((int64_t)L.yp * L.h2p);
    L.wpack_elems = o;
    // the stash of a frame
    int s = 0;
    auto col = [&](int n) { const int at = s; s += n; return at; };
    L.s_h1e = col(L.h1p); L.s_h2e = col(L.h2p); L.s_z = col(L.zp); L.s_d1 = col(L.h2p); L.s_d2 = col(L.h1p);
    L.s_pe1 = col(L.h1p); L.s_pe2 = col(L.h2p); L.s_ph = col(2 * L.zp); L.s_pd1 = col(L.h2p); L.s_pd2 = col(L.h1p); L.s_da = col(GXP);
    L.s_c1 = col(L.h1p); L.s_c2 = col(L.h2p); L.s_pc1 = col(L.h1p); L.s_pc2 = col(L.h2p); L.s_pco = col(L.yp);
    L.s_a1 = col(L.h1p); L.s_a2 = col(L.h2p); L.s_pa1 = col(L.h1p); L.s_pa2 = col(L.h2p); L.s_pao = col(L.yp);
    if (dec_clf) L.s_zc = col((L.z + L.y + 3) / 4 * 4);                   // (a multiple of 4: the 16-byte stores of the next frame stay aligned)
    L.S = s;
    // frames, tiles, slices
    L.B = B;
    L.tiles = (B + GT - 1) / GT;
    L.Bp = L.tiles * GT;
    L.rows_grid = L.tiles < G_ROWS_GRID ? L.tiles : G_ROWS_GRID;
    GGemm gm[I_NG];
    make_gemms(L, gm);
    int row_tiles = 0;                                    // weight-gradient items of one frame slice
    for (int i = 0; i < I_NG; ++i) row_tiles += gemm_items(gm[i]);
    choose_slices(B, row_tiles, ksplit_hint, L.slice_frames, L.nslices);
    L.n_items = row_tiles * L.nslices;
    // workspace
    int64_t w = al256(L.wpack_elems * 4);
    L.o_items = w; w = al256(w + (int64_t)L.n_items * sizeof(GItem));
    // the fifth sum (V) behind the [rows_grid][4]; the clamped KL sums behind whichever comes last (partials_k_off)
    L.o_partials = w; w = al256(w + L.rows_grid * (aux_v ? 6 : 5) * sizeof(double));
    L.o_stash = w; w = al256(w + L.Bp * (int64_t)L.S * 4);
    L.o_grads = w; w = al256(w + (int64_t)L.nslices * L.n_params * 4);
    L.ws_bytes = w;
    // the tiles of the M1 / M2 kernel: the side nets reuse them
    L.lds_bytes = (int64_t)GT * (GXP + L.yp + 2 * L.hm + 3 * L.zp) * 4 + GT * sizeof(int64_t);
    return L;
}

// the clamped KL sums of the weighted KL term, in doubles from o_partials
static int64_t partials_k_off(const ILayout& L) { return ((L.mode & (DVAE_INFO_AUX_UNIFORM | DVAE_INFO_AUX_ENTROPY)) ? 5 : 4) * L.rows_grid; }

static void make_tensors(const ILayout& L, GTensor* T) {
    for (int t = 0; t < G_NT; ++t) memset(&T[t], 0, sizeof(GTensor));
    for (int t = 0; t < I_NT; ++t) {
        GTensor& d = T[t];
        d.off = L.toff[t]; d.rows = L.trows[t]; d.cols = L.tcols[t];
        d.t0 = -1; d.split = d.cols; d.bias = t & 1;
    }
    const int k1 = L.h1p / 16, k2 = L.h2p / 16, kz = L.zp / 16, ky = L.yp / 16;
    T[0].f0 = L.W1; T[0].kb0 = GKX;
    T[1].f0 = L.b1;
    T[2].f0 = L.W2; T[2].kb0 = k1; T[2].t0 = L.W2T; T[2].tkb = k2; T[2].tcmax = L.h1;
    T[3].f0 = L.b2;
    T[4].f0 = L.Wh; T[4].kb0 = k2; T[4].t0 = L.WhT; T[4].tkb = 2 * kz; T[4].tcmax = L.h2;
    T[5].f0 = L.bh;
    T[6].f0 = L.Wh; T[6].kb0 = k2; T[6].roff = L.zp; T[6].t0 = L.WhT; T[6].tkb = 2 * kz; T[6].tkoff = L.zp; T[6].tcmax = L.h2;
    T[7].f0 = L.bh; T[7].roff = L.zp;
    T[8].f0 = L.D1z; T[8].kb0 = kz; T[8].split = L.z; T[8].f1 = L.D1y; T[8].kb1 = ky; T[8].t0 = L.D1zT; T[8].tkb = k2; T[8].tcmax = L.z;
    if (L.mode & DVAE_INFO_DEC_CLASSIFIER) { T[8].t1 = L.D1yT; T[8].tkb1 = k2; }
    T[9].f0 = L.bd1;
    T[10].f0 = L.D2; T[10].kb0 = k2; T[10].t0 = L.D2T; T[10].tkb = k1; T[10].tcmax = L.h2;
    T[11].f0 = L.bd2;
    T[12].f0 = L.D3; T[12].kb0 = k1; T[12].t0 = L.D3T; T[12].tkb = GKX; T[12].tcmax = L.h1;
    T[13].f0 = L.bd3;
    T[14].f0 = L.C1; T[14].kb0 = GKX;
    T[15].f0 = L.bc1;
    T[16].f0 = L.C2; T[16].kb0 = k1; T[16].t0 = L.C2T; T[16].tkb = k2; T[16].tcmax = L.h1;
    T[17].f0 = L.bc2;
    T[18].f0 = L.Co; T[18].kb0 = k2; T[18].t0 = L.CoT; T[18].tkb = ky; T[18].tcmax = L.h2;
    T[19].f0 = L.bco;
    T[20].f0 = L.A1; T[20].kb0 = kz; T[20].t0 = L.A1T; T[20].tkb = k1; T[20].tcmax = L.z;
    T[21].f0 = L.ba1;
    T[22].f0 = L.A2; T[22].kb0 = k1; T[22].t0 = L.A2T; T[22].tkb = k2; T[22].tcmax = L.h1;
    T[23].f0 = L.ba2;
    T[24].f0 = L.Ao; T[24].kb0 = k2; T[24].t0 = L.AoT; T[24].tkb = ky; T[24].tcmax = L.h2;
    T[25].f0 = L.bao;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rows kernel
struct IRowsArgs {
    const float* x; int64_t ldx;
    const float* y; int64_t ldy;
    const float* eps;                 // [B][z]
    const int64_t* row_index; int64_t row_count; int* bad;
    float* ws;                        // the packed copies start the workspace
    float* stash; double* partials;
    float elbo_eps, invB;
    float clf_scale;                  // alpha / B: the weight of d BCE(clf(x), y)
    float aux_z_scale;                // -beta: the unit auxiliary gradients where they flow to z
    float aux_w_scale;                // gamma - beta: ... where they are stashed for the weight gradients
    float aux_gamma;                  // gamma: the weight of d BCE in the auxiliary tensors when the adversarial term is not a cross entropy
    double* partials_v;               // [rows_grid] the sums of V (then only)
    int fwd_only;
    // the weighted KL term (plan->kl_weight w, plan->kl_floor; train_generic.hip: GRowsArgs): kl_scale = fl32(fl32(w) * invB), invB itself at w = 1
    float kl_scale, kl_floor;
    double* partials_k;               // [rows_grid] the sums of the KL elements clamped from below at kl_floor
};
static_assert(sizeof(ILayout) + sizeof(IRowsArgs) <= G_KERNARG_MAX, "layout and arguments travel as kernel arguments");

// DC: the decoder is fed the classifier's output p_c instead of the label (dec_label "classifier"); AV: the adversarial term V on the
// encoder is 0 the cross entropy, 1 binary_cross_entropy_v2 (targets 0.5), 2 binary_cross_entropy_v3 (the entropy of aux(z)).  <false, 0>
// is the step described at the top of the file.  What the other instantiations change:
//   DC  phase 1 ends with p_c in Y (the labels are done with until the classifier's backward pass) and in the stash behind z; phase 3 runs
//       as it is, on p_c; behind it, with dpre_d1 in A: d p_c = alpha dBCE / d p_c + dpre_d1 D1[:, z:] (the transposed label block D1yT),
//       dpre_o -> X, and the thread puts the label it read for this -- again through the frame's row of the gather table, so a refused
//       index stays counted once -- back into Y; dpre_c2 -> Bf and dpre_c1 with the relu masks from the stash.
//   AV  the output layer of the auxiliary net forms two gradients: gamma dBCE - beta dV at weight 1 / B -> X (towards the weights: the
//       chain that is stashed) and dV at weight 1 / B -> Y (towards z; the labels are done with for this tile).  The weight chain runs
//       first, then the z chain through the same relu masks, read from the stash; dpre_a1 of the z chain -> X for phase 5.
// KLW (plan->kl_weight / kl_floor other than 1 / 0): the weighted KL term as in train_generic_rows_kernel -- kl_scale = w / B on the KL parts
//   of d mu and d log_var where the element is not below kl_floor, exact zeros below it, and the sums of max(k, kl_floor) in partials_k.
//   A template flag: the six instantiations without it are the code they were (the compiler spills in three of them when the two
//   scalars are read at run time: DESIGN 4a''').
template <bool DC, int AV, bool KLW = false>
__global__ __launch_bounds__(256) void train_info_rows_kernel(const ILayout L, const IRowsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ism[];
    float* X = ism;                                     // [528][16] x; dpre_o of the classifier; x again; d loss / d a; a1, dpre_ao, dpre_a1
    float* Y = X + GT * GXP;                            // [yp][16]
    float* A = Y + GT * L.yp;                           // [hm][16] c1; h1e; d1, dpre_d1
    float* Bf = A + GT * L.hm;                          // [hm][16] c2, dpre_c2; h2e, z; d2, dpre_d2; z, a2, dpre_a2; dpre_e2
    float* C = Bf + GT * L.hm;                          // [3 zp][16] heads; then mu / B | KL part of d log_var | eps std / 2; then d mu | d log_var
    int64_t* srow = reinterpret_cast<int64_t*>(C + GT * 3 * L.zp);     // [16] the frame's row of x / y, -1: past B

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int ky = L.yp >> 4, k1 = L.h1p >> 4, k2 = L.h2p >> 4, kz = L.zp >> 4;
    const float* wp = g.ws;
    const bool bwd = !g.fwd_only;
    double sum_is = 0.0, sum_kl = 0.0, sum_bc = 0.0, sum_ba = 0.0;
    [[maybe_unused]] double sum_bv = 0.0;                // V, where it is not the cross entropy
    [[maybe_unused]] double sum_kc = 0.0;               // KLW: the KL elements clamped from below at kl_floor

    for (int64_t tile = blockIdx.x; tile < L.tiles; tile += gridDim.x) {
        const int64_t r0 = tile * GT;
        // the weight base is opaque per tile: the addresses of the twenty-odd phases are formed where they are used, not all of them
        // ahead of the loop, where they would not fit the registers
        asm volatile("" : "+s"(wp));
        __syncthreads();                                // the previous tile's readers of every tile are done
        if (tid < GT) {
            const int64_t r = r0 + tid;
            int64_t s = -1;
            if (r < L.B) {
                s = r;
                if (g.row_index) {
                    s = g.row_index[r];
                    if (s < 0 || s >= g.row_count) {
                        s = 0;
                        if (g.bad) atomicAdd(g.bad, 1);
                    }
                }
            }
            srow[tid] = s;
        }
        __syncthreads();
        const bool fok = srow[col] >= 0;                // this lane's frame of the accumulator tiles
        float* const sfr = g.stash + (r0 + col) * (int64_t)L.S + 4 * quad;
        auto st4 = [&](int off, int t, const f32x4& v) { if (bwd) *reinterpret_cast<f32x4*>(sfr + off + 16 * t) = v; };
        auto ld4 = [&](int off, int t) { return *reinterpret_cast<const f32x4*>(sfr + off + 16 * t); };
        // the x tile: a quarter wave reads 16 consecutive inputs of one frame
        auto load_x = [&]() {
            for (int b = wave; b < GKX; b += 4) {
#pragma unroll
                for (int cq = 0; cq < 4; ++cq) {
                    const int k = 16 * b + col, c = 4 * cq + quad;
                    const int64_t s = srow[c];
                    X[k * GT + c] = (k < GX && s >= 0) ? g.x[s * g.ldx + k] : 0.f;
                }
            }
        };
        // p = sigmoid(a) against the label yv: the frame's BCE terms and d BCE / d a at weight `scale` (oracle/vae_oracle.py: bce_bwd, the eps
        // terms kept; zero where !ok)
        auto bce = [&](float a, float yv, bool ok, float scale, double& sum) {
            const float p = 1.f / (1.f + expf(-a));
            const float q = 1.f - p;
            if (ok) sum -= (double)(yv * logf(p + g.elbo_eps) + (1.f - yv) * logf(q + g.elbo_eps));
            const float dp = -scale * (yv / (p + g.elbo_eps) - (1.f - yv) / (q + g.elbo_eps));
            return ok ? dp * p * q : 0.f;
        };

        load_x();
        for (int b = wave; b < ky; b += 4) {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
                const int k = 16 * b + col, c = 4 * cq + quad;
                const int64_t s = srow[c];
                Y[k * GT + c] = (k < L.y && s >= 0) ? g.y[s * g.ldy + k] : 0.f;
            }
        }
        __syncthreads();

        // ================================ 1. the classifier on x (train_classifier.hip's arrangement) ================================
        // ---- c1 = relu(x C1^T + b) -> A ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.C1 + (int64_t)t * GKX * 256, GKX, X, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.bc1 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                A[row * GT + col] = h[r];
            }
            st4(L.s_c1, t, h);
        }
        __syncthreads();
        // ---- c2 = relu(c1 C2^T + b) -> Bf ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.C2 + (int64_t)t * k1 * 256, k1, A, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.bc2 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                Bf[row * GT + col] = h[r];
            }
            st4(L.s_c2, t, h);
        }
        __syncthreads();
        // ---- a = c2 Co^T + b, p = sigmoid(a); BCE; dpre_o = alpha / B d BCE / d a -> X rows 0 .. yp - 1 ----
        for (int t = wave; t < ky; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.Co + (int64_t)t * k2 * 256, k2, Bf, lane);
            if constexpr (DC) {
                // p_c takes the label's place in Y (zero in padded columns and frames past B) and lies behind z in the stash
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const bool ok = fok && row < L.y;
                    const float p = 1.f / (1.f + expf(-(acc[r] + wp[L.bco + row])));
                    const float q = 1.f - p, yv = Y[row * GT + col];
                    if (ok) sum_bc -= (double)(yv * logf(p + g.elbo_eps) + (1.f - yv) * logf(q + g.elbo_eps));
                    Y[row * GT + col] = ok ? p : 0.f;
                    if (bwd && ok) g.stash[(r0 + col) * (int64_t)L.S + L.s_zc + L.z + row] = p;
                }
                continue;
            }
            f32x4 da;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                da[r] = bce(acc[r] + wp[L.bco + row], Y[row * GT + col], fok && row < L.y, g.clf_scale, sum_bc);
                if (bwd) X[row * GT + col] = da[r];
            }
            st4(L.s_pco, t, da);
        }
        if (!DC && bwd) {
            __syncthreads();
            // ---- d c2 = dpre_o Co; dpre_c2 = d c2 [c2 > 0] -> Bf (c2: this thread's own entry) ----
            for (int t = wave; t < k2; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.CoT + (int64_t)t * ky * 256, ky, X, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    d[r] = Bf[row * GT + col] > 0.f ? acc[r] : 0.f;
                    Bf[row * GT + col] = d[r];
                }
                st4(L.s_pc2, t, d);
            }
            __syncthreads();
            // ---- d c1 = dpre_c2 C2; dpre_c1 = d c1 [c1 > 0]: only the stash needs it ----
            for (int t = wave; t < k1; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.C2T + (int64_t)t * k2 * 256, k2, Bf, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = A[(16 * t + 4 * quad + r) * GT + col] > 0.f ? acc[r] : 0.f;
                st4(L.s_pc1, t, d);
            }
            load_x();                                   // (the readers of dpre_o in X are two barriers back)
        }
        __syncthreads();

        // ================================ 2. encoder forward ================================
        // ---- h1e = tanh(x W1^T + b1) -> A ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W1 + (int64_t)t * GKX * 256, GKX, X, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                h[r] = tanhf(acc[r] + wp[L.b1 + row]);
                A[row * GT + col] = h[r];
            }
            st4(L.s_h1e, t, h);
        }
        __syncthreads();
        // ---- h2e = tanh(h1e W2^T + b2) -> Bf ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W2 + (int64_t)t * k1 * 256, k1, A, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                h[r] = tanhf(acc[r] + wp[L.b2 + row]);
                Bf[row * GT + col] = h[r];
            }
            st4(L.s_h2e, t, h);
        }
        __syncthreads();
        // ---- heads: [mu | log_var] -> C rows 0 .. 2 zp - 1 ----
        for (int t = wave; t < 2 * kz; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.Wh + (int64_t)t * k2 * 256, k2, Bf, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                C[row * GT + col] = acc[r] + wp[L.bh + row];
            }
        }
        __syncthreads();
        // ---- z = mu + exp(log_var / 2) eps -> Bf and the stash (the auxiliary phase reads it back); the KL terms; what the backward
        // pass needs of the heads -> C ----
        for (int i = tid; i < GT * L.zp; i += 256) {
            const int c = i & 15, j = i >> 4;
            const bool ok = srow[c] >= 0 && j < L.z;
            const float mu = C[j * GT + c], lv = C[(L.zp + j) * GT + c];
            const float e = ok ? g.eps[(r0 + c) * L.z + j] : 0.f;
            const float sd = expf(0.5f * lv), ev = expf(lv);
            const float zv = mu + sd * e;
            Bf[j * GT + c] = zv;
            if constexpr (KLW) {
                // the KL element and its weight: w / B where it is not below the floor (torch.clamp's gradient), zero below it
                const float k = -0.5f * (lv - mu * mu - ev);
                const float ks = (ok && !(k < g.kl_floor)) ? g.kl_scale : 0.f;
                C[j * GT + c] = ok ? mu * ks : 0.f;
                C[(L.zp + j) * GT + c] = ok ? -0.5f * (1.f - ev) * ks : 0.f;
                C[(2 * L.zp + j) * GT + c] = 0.5f * sd * e;
                if (ok) { sum_kl += (double)k; sum_kc += (double)(k < g.kl_floor ? g.kl_floor : k); }
            } else {
                C[j * GT + c] = ok ? mu * g.invB : 0.f;
                C[(L.zp + j) * GT + c] = ok ? -0.5f * (1.f - ev) * g.invB : 0.f;
                C[(2 * L.zp + j) * GT + c] = 0.5f * sd * e;
                if (ok) sum_kl += (double)(-0.5f * (lv - mu * mu - ev));
            }
            g.stash[(r0 + c) * (int64_t)L.S + L.s_z + j] = zv;
            if constexpr (DC) {
                if (bwd && j < L.z) g.stash[(r0 + c) * (int64_t)L.S + L.s_zc + j] = zv;     // [z | p_c] for the weight gradient of decoder layer 1
            }
        }
        __syncthreads();

        // ================================ 3. decoder forward and backward ================================
        // ---- d1 = tanh([z | y] D1^T + b) -> A ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.D1z + (int64_t)t * kz * 256, kz, Bf, lane);
            acc = tg_gemm(acc, wp + L.D1y + (int64_t)t * ky * 256, ky, Y, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                h[r] = tanhf(acc[r] + wp[L.bd1 + row]);
                A[row * GT + col] = h[r];
            }
            st4(L.s_d1, t, h);
        }
        __syncthreads();
        // ---- d2 = tanh(d1 D2^T + b) -> Bf ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.D2 + (int64_t)t * k2 * 256, k2, A, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                h[r] = tanhf(acc[r] + wp[L.bd2 + row]);
                Bf[row * GT + col] = h[r];
            }
            st4(L.s_d2, t, h);
        }
        __syncthreads();
        // ---- a = d2 D3^T + b, r = exp(a); Itakura-Saito x / r - log(x + eps) + a - 1; d loss / d a = (1 - x / r) / B -> X ----
        for (int t = wave; t < GKX; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.D3 + (int64_t)t * k1 * 256, k1, Bf, lane);
            f32x4 da;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const bool ok = fok && row < GX;
                const float a = acc[r] + wp[L.bd3 + row];
                const float xv = X[row * GT + col];
                const float q = xv * expf(-a);
                if (ok) sum_is += (double)(q - logf(xv + g.elbo_eps) + a - 1.f);
                da[r] = ok ? (1.f - q) * g.invB : 0.f;
                if (bwd) X[row * GT + col] = da[r];
            }
            st4(L.s_da, t, da);
        }
        __syncthreads();
        if (bwd) {
            // ---- d d2 = da D3; dpre_d2 = d d2 (1 - d2^2) -> Bf ----
            for (int t = wave; t < k1; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.D3T + (int64_t)t * GKX * 256, GKX, X, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const float o = Bf[row * GT + col];
                    d[r] = acc[r] * (1.f - o * o);
                    Bf[row * GT + col] = d[r];
                }
                st4(L.s_pd2, t, d);
            }
            __syncthreads();
            // ---- d d1 = dpre_d2 D2; dpre_d1 = d d1 (1 - d1^2) -> A, where it stays until dz ----
            for (int t = wave; t < k2; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.D2T + (int64_t)t * k1 * 256, k1, Bf, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const float o = A[row * GT + col];
                    d[r] = acc[r] * (1.f - o * o);
                    A[row * GT + col] = d[r];
                }
                st4(L.s_pd1, t, d);
            }
            __syncthreads();
            if constexpr (DC) {
                // ---- the classifier's backward pass: d p_c = alpha d BCE / d p_c + dpre_d1 D1[:, z:]; dpre_o -> X rows 0 .. yp - 1 (d loss / d a
                // is done with); the label, read again through the frame's row, returns to Y ----
                for (int t = wave; t < ky; t += 4) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    acc = tg_gemm(acc, wp + L.D1yT + (int64_t)t * k2 * 256, k2, A, lane);
                    f32x4 da;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * t + 4 * quad + r;
                        const bool ok = fok && row < L.y;
                        const float yv = ok ? g.y[srow[col] * g.ldy + row] : 0.f;
                        const float p = Y[row * GT + col], q = 1.f - p;
                        const float dp = acc[r] - g.clf_scale * (yv / (p + g.elbo_eps) - (1.f - yv) / (q + g.elbo_eps));
                        da[r] = ok ? dp * p * q : 0.f;
                        X[row * GT + col] = da[r];
                        Y[row * GT + col] = yv;
                    }
                    st4(L.s_pco, t, da);
                }
                __syncthreads();
                // ---- d c2 = dpre_o Co; dpre_c2 = d c2 [c2 > 0] -> Bf (c2: this thread's own stash entry; dpre_d2 is done with) ----
                for (int t = wave; t < k2; t += 4) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    acc = tg_gemm(acc, wp + L.CoT + (int64_t)t * ky * 256, ky, X, lane);
                    const f32x4 o = ld4(L.s_c2, t);
                    f32x4 d;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        d[r] = o[r] > 0.f ? acc[r] : 0.f;
                        Bf[(16 * t + 4 * quad + r) * GT + col] = d[r];
                    }
                    st4(L.s_pc2, t, d);
                }
                __syncthreads();
                // ---- d c1 = dpre_c2 C2; dpre_c1 = d c1 [c1 > 0]: only the stash needs it ----
                for (int t = wave; t < k1; t += 4) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    acc = tg_gemm(acc, wp + L.C2T + (int64_t)t * k2 * 256, k2, Bf, lane);
                    const f32x4 o = ld4(L.s_c1, t);
                    f32x4 d;
#pragma unroll
                    for (int r = 0; r < 4; ++r) d[r] = o[r] > 0.f ? acc[r] : 0.f;
                    st4(L.s_pc1, t, d);
                }
                __syncthreads();
            }
        }

        // ================================ 4. the auxiliary net on z: X and Bf are free ================================
        // ---- z back from the stash -> Bf (the entries this thread wrote) ----
        for (int i = tid; i < GT * L.zp; i += 256) {
            const int c = i & 15, j = i >> 4;
            Bf[j * GT + c] = g.stash[(r0 + c) * (int64_t)L.S + L.s_z + j];
        }
        if constexpr (DC) {
            if (!bwd) {                                 // no backward pass has put the labels back into Y
                for (int b = wave; b < ky; b += 4) {
#pragma unroll
                    for (int cq = 0; cq < 4; ++cq) {
                        const int k = 16 * b + col, c = 4 * cq + quad;
                        const int64_t s = srow[c];
                        Y[k * GT + c] = (k < L.y && s >= 0) ? g.y[s * g.ldy + k] : 0.f;
                    }
                }
            }
        }
        __syncthreads();
        // ---- a1 = relu(z A1^T + b) -> X ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.A1 + (int64_t)t * kz * 256, kz, Bf, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.ba1 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                X[row * GT + col] = h[r];
            }
            st4(L.s_a1, t, h);
        }
        __syncthreads();
        // ---- a2 = relu(a1 A2^T + b) -> Bf ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.A2 + (int64_t)t * k1 * 256, k1, X, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.ba2 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                Bf[row * GT + col] = h[r];
            }
            st4(L.s_a2, t, h);
        }
        __syncthreads();
        // ---- a = a2 Ao^T + b, p = sigmoid(a); BCE; dpre_ao = 1 / B d BCE / d a -> X rows 0 .. yp - 1; times (gamma - beta) -> stash ----
        for (int t = wave; t < ky; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.Ao + (int64_t)t * k2 * 256, k2, Bf, lane);
            f32x4 da;
            if constexpr (AV != 0) {
                // V and d V / d p (oracle/vae_oracle.py: bce_v2_bwd, bce_v3_bwd, the eps terms kept); towards the weights gamma dBCE - beta dV
                // -> X and the stash, towards z dV -> Y (times -beta where dz is formed: beta = 0 divides nothing)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const bool ok = fok && row < L.y;
                    const float p = 1.f / (1.f + expf(-(acc[r] + wp[L.bao + row])));
                    const float q = 1.f - p, yv = Y[row * GT + col];
                    const float lp = logf(p + g.elbo_eps), lq = logf(q + g.elbo_eps);
                    const float ip = 1.f / (p + g.elbo_eps), iq = 1.f / (q + g.elbo_eps);
                    if (ok) {
                        sum_ba -= (double)(yv * lp + (1.f - yv) * lq);
                        sum_bv -= (double)(AV == 1 ? 0.5f * lp + 0.5f * lq : p * lp + q * lq);
                    }
                    const float db = -g.invB * (yv * ip - (1.f - yv) * iq);
                    const float dv = AV == 1 ? -g.invB * (0.5f * ip - 0.5f * iq) : -g.invB * (lp + p * ip - lq - q * iq);
                    da[r] = ok ? (g.aux_gamma * db + g.aux_z_scale * dv) * p * q : 0.f;
                    if (bwd) {
                        X[row * GT + col] = da[r];
                        Y[row * GT + col] = ok ? dv * p * q : 0.f;
                    }
                }
                st4(L.s_pao, t, da);
                continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float d = bce(acc[r] + wp[L.bao + row], Y[row * GT + col], fok && row < L.y, g.invB, sum_ba);
                if (bwd) X[row * GT + col] = d;
                da[r] = d * g.aux_w_scale;
            }
            st4(L.s_pao, t, da);
        }
        if (!bwd) continue;
        __syncthreads();
        if constexpr (AV != 0) {
            // ---- the chain towards the weights: dpre_a2 = (dpre_ao Ao) [a2 > 0] -> Bf (a2: this thread's own entry) and the stash ----
            for (int t = wave; t < k2; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.AoT + (int64_t)t * ky * 256, ky, X, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    d[r] = Bf[row * GT + col] > 0.f ? acc[r] : 0.f;
                    Bf[row * GT + col] = d[r];
                }
                st4(L.s_pa2, t, d);
            }
            __syncthreads();
            // ---- dpre_a1 = (dpre_a2 A2) [a1 > 0]: only the stash needs this chain's ----
            for (int t = wave; t < k1; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.A2T + (int64_t)t * k2 * 256, k2, Bf, lane);
                const f32x4 o = ld4(L.s_a1, t);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = o[r] > 0.f ? acc[r] : 0.f;
                st4(L.s_pa1, t, d);
            }
            __syncthreads();
            // ---- the chain towards z, from Y: the same masks, a2 now from the stash; dpre_a2 -> Bf, dpre_a1 -> X for phase 5 ----
            for (int t = wave; t < k2; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.AoT + (int64_t)t * ky * 256, ky, Y, lane);
                const f32x4 o = ld4(L.s_a2, t);
#pragma unroll
                for (int r = 0; r < 4; ++r) Bf[(16 * t + 4 * quad + r) * GT + col] = o[r] > 0.f ? acc[r] : 0.f;
            }
            __syncthreads();
            for (int t = wave; t < k1; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.A2T + (int64_t)t * k2 * 256, k2, Bf, lane);
                const f32x4 o = ld4(L.s_a1, t);
#pragma unroll
                for (int r = 0; r < 4; ++r) X[(16 * t + 4 * quad + r) * GT + col] = o[r] > 0.f ? acc[r] : 0.f;
            }
            __syncthreads();
        } else {
            // ---- d a2 = dpre_ao Ao; dpre_a2 = d a2 [a2 > 0] -> Bf (a2: this thread's own entry) ----
            for (int t = wave; t < k2; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.AoT + (int64_t)t * ky * 256, ky, X, lane);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const float v = Bf[row * GT + col] > 0.f ? acc[r] : 0.f;
                    Bf[row * GT + col] = v;
                    d[r] = v * g.aux_w_scale;
                }
                st4(L.s_pa2, t, d);
            }
            __syncthreads();
            // ---- d a1 = dpre_a2 A2; dpre_a1 = d a1 [a1 > 0] -> X (a1: this thread's own stash entry; dpre_ao in X is done with) ----
            for (int t = wave; t < k1; t += 4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = tg_gemm(acc, wp + L.A2T + (int64_t)t * k2 * 256, k2, Bf, lane);
                const f32x4 o = ld4(L.s_a1, t);
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * quad + r;
                    const float v = o[r] > 0.f ? acc[r] : 0.f;
                    X[row * GT + col] = v;
                    d[r] = v * g.aux_w_scale;
                }
                st4(L.s_pa1, t, d);
            }
            __syncthreads();
        }

        // ================================ 5. dz and the encoder's backward pass ================================
        // ---- dz = dpre_d1 D1[:, :z] - beta dpre_a1 A1; d mu = dz + mu / B; d log_var = dz eps std / 2 + its KL part -> C rows 0 .. 2 zp - 1 ----
        for (int t = wave; t < kz; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f}, aux = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.D1zT + (int64_t)t * k2 * 256, k2, A, lane);
            aux = tg_gemm(aux, wp + L.A1T + (int64_t)t * k1 * 256, k1, X, lane);
            f32x4 dm, dl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float dz = acc[r] + g.aux_z_scale * aux[r];
                dm[r] = dz + C[row * GT + col];
                dl[r] = dz * C[(2 * L.zp + row) * GT + col] + C[(L.zp + row) * GT + col];
                C[row * GT + col] = dm[r];
                C[(L.zp + row) * GT + col] = dl[r];
            }
            st4(L.s_ph, t, dm);
            st4(L.s_ph + L.zp, t, dl);
        }
        __syncthreads();
        // ---- d h2e = [d mu | d log_var] [Wmu; Wlv]; dpre_e2 = d h2e (1 - h2e^2) -> Bf (h2e: this thread's own stash entry) ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.WhT + (int64_t)t * 2 * kz * 256, 2 * kz, C, lane);
            const f32x4 o = ld4(L.s_h2e, t);
            f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                d[r] = acc[r] * (1.f - o[r] * o[r]);
                Bf[row * GT + col] = d[r];
            }
            st4(L.s_pe2, t, d);
        }
        __syncthreads();
        // ---- d h1e = dpre_e2 W2; dpre_e1 = d h1e (1 - h1e^2): only the stash needs it ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W2T + (int64_t)t * k2 * 256, k2, Bf, lane);
            const f32x4 o = ld4(L.s_h1e, t);
            f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = acc[r] * (1.f - o[r] * o[r]);
            st4(L.s_pe1, t, d);
        }
    }
    // the workgroup's loss sums: waves in order
    sum_is = wave_sum(sum_is); sum_kl = wave_sum(sum_kl); sum_bc = wave_sum(sum_bc); sum_ba = wave_sum(sum_ba);
    __syncthreads();                                    // the last tile's readers of X are done: its first bytes hold the sums
    double (*red)[4] = reinterpret_cast<double (*)[4]>(ism);
    if (lane == 0) { red[wave][0] = sum_is; red[wave][1] = sum_kl; red[wave][2] = sum_bc; red[wave][3] = sum_ba; }
    __syncthreads();
    if (tid < 4) g.partials[4 * (int64_t)blockIdx.x + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if constexpr (AV != 0) {
        sum_bv = wave_sum(sum_bv);
        double* redv = reinterpret_cast<double*>(ism) + 16;
        if (lane == 0) redv[wave] = sum_bv;
        __syncthreads();
        if (tid == 0) g.partials_v[blockIdx.x] = ((redv[0] + redv[1]) + redv[2]) + redv[3];
    }
    if constexpr (KLW) {
        sum_kc = wave_sum(sum_kc);
        double* redk = reinterpret_cast<double*>(ism) + 20;
        if (lane == 0) redk[wave] = sum_kc;
        __syncthreads();
        if (tid == 0) g.partials_k[blockIdx.x] = ((redk[0] + redk[1]) + redk[2]) + redk[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
static const char* LIMITS = "the M2_info train step covers DeepGenerativeModel_v5 at x 513, y_dim 1..513, hidden widths 1..512, z_dim 1..128, exact fp32, one GPU";

template <bool DC, int AV, bool KLW>
static int launch_rows_klw(const ILayout& L, const IRowsArgs& g, hipStream_t s) {
    static bool attr_done[64] = {};                     // (one per instantiation: the limit is a property of the kernel)
    if (int rc = raise_lds_limit((const void*)train_info_rows_kernel<DC, AV, KLW>, "train_info_rows_kernel", L.lds_bytes, attr_done)) return rc;
    hipLaunchKernelGGL((train_info_rows_kernel<DC, AV, KLW>), dim3((unsigned)L.rows_grid), dim3(256), (size_t)L.lds_bytes, s, L, g);
    DVAE_LAUNCH_OK("train_info_rows_kernel");
    return 0;
}
template <bool DC, int AV>
static int launch_rows_mode(const ILayout& L, const IRowsArgs& g, bool klw, hipStream_t s) {
    return klw ? launch_rows_klw<DC, AV, true>(L, g, s) : launch_rows_klw<DC, AV, false>(L, g, s);
}

// the M2_info step as train_step_host.hpp reads it
struct IStep {
    using Plan = dvae_train_info_plan_t;
    using Layout = ILayout;
    static constexpr int NT = I_NT, NG = I_NG;
    static constexpr int ORDER[I_NG] = {0, 7, 6, 4, 1, 5, 8, 11, 2, 3, 9, 12, 10};     // the widest inputs first: their items run longest
    static constexpr bool COUNTS = false, WGRAD_Y = true;

    static int plan_layout(const char* who, const Plan* plan, ILayout& L, bool) {
        DVAE_CHECK_ARG(plan, "%s: null plan", who);
        DVAE_CHECK_ARG(dims_ok(plan->y_dim, plan->z_dim, plan->h1, plan->h2) && plan->B >= 1 && plan->n_tensors == I_NT && mode_ok(plan->info_mode),
                       "%s: not a plan of dvae_train_info_plan", who);
        DVAE_CHECK_ARG(plan->kl_weight >= 0.0 && isfinite(plan->kl_weight) && plan->kl_floor >= 0.0 && isfinite(plan->kl_floor),
                       "%s: kl_weight %g / kl_floor %g in the plan (finite numbers >= 0; the planner sets 1 and 0)", who, plan->kl_weight, plan->kl_floor);
        L = make_layout(plan->y_dim, plan->z_dim, plan->h1, plan->h2, plan->B, plan->ksplit, plan->info_mode);
        DVAE_CHECK_ARG(L.ws_bytes == plan->workspace_bytes && L.nslices == plan->ksplit && L.n_params == plan->n_params &&
                       L.slice_frames == plan->slice_frames, "%s: the plan was changed after dvae_train_info_plan", who);
        return 0;
    }

    static int check_inputs(const char* who, const Plan* plan, const void* ws, const StepInputs& in) {
        DVAE_CHECK_ARG(ws && in.x && in.y && in.eps, "%s: null pointer", who);
        DVAE_CHECK_ARG(in.ldx >= GX && in.ldx < ((int64_t)1 << 20), "%s: leading dimension of x %lld (at least 513)", who, (long long)in.ldx);
        DVAE_CHECK_ARG(in.ldy >= plan->y_dim && in.ldy < ((int64_t)1 << 20), "%s: leading dimension of y %lld for y_dim %d", who, (long long)in.ldy,
                       plan->y_dim);
        DVAE_CHECK_ARG(!plan->row_index || plan->row_count >= 1, "%s: a gather table needs row_count >= 1 (got %lld)", who, (long long)plan->row_count);
        return 0;
    }

    static int launch_rows(const Plan* plan, const ILayout& L, char* ws, const StepInputs& in, bool fwd_only, hipStream_t s) {
        IRowsArgs g;
        memset(&g, 0, sizeof(g));
        g.x = in.x; g.ldx = in.ldx; g.y = in.y; g.ldy = in.ldy; g.eps = in.eps;
        g.row_index = (const int64_t*)(uintptr_t)plan->row_index; g.row_count = plan->row_count; g.bad = (int*)(uintptr_t)plan->bad_row_counter;
        g.ws = (float*)ws; g.stash = (float*)(ws + L.o_stash); g.partials = (double*)(ws + L.o_partials);
        g.elbo_eps = in.loss_eps; g.invB = (float)(1.0 / (double)L.B); g.fwd_only = fwd_only ? 1 : 0;
        g.clf_scale = (float)(plan->info_alpha / (double)L.B);
        g.aux_z_scale = (float)(-plan->info_beta);
        g.aux_w_scale = (float)(plan->info_gamma - plan->info_beta);
        g.aux_gamma = (float)plan->info_gamma;
        g.partials_v = g.partials + 4 * L.rows_grid;
        g.partials_k = g.partials + partials_k_off(L);
        g.kl_scale = (float)plan->kl_weight * g.invB; g.kl_floor = (float)plan->kl_floor;        // (read by the KLW instantiations)
        const bool dc = (L.mode & DVAE_INFO_DEC_CLASSIFIER) != 0;
        const int av = (L.mode & DVAE_INFO_AUX_UNIFORM) ? 1 : ((L.mode & DVAE_INFO_AUX_ENTROPY) ? 2 : 0);
        const bool klw = kl_weighted(plan);
        if (!dc) return av == 0 ? launch_rows_mode<false, 0>(L, g, klw, s) : (av == 1 ? launch_rows_mode<false, 1>(L, g, klw, s) : launch_rows_mode<false, 2>(L, g, klw, s));
        return av == 0 ? launch_rows_mode<true, 0>(L, g, klw, s) : (av == 1 ? launch_rows_mode<true, 1>(L, g, klw, s) : launch_rows_mode<true, 2>(L, g, klw, s));
    }

    static void tensors(const ILayout& L, GTensor* T) { make_tensors(L, T); }
    static void gemms(const ILayout& L, GGemm* G) { make_gemms(L, G); }
    static size_t partials_bytes(const ILayout& L) { return (size_t)L.rows_grid * ((L.mode & MODE_AUX) ? 6 : 5) * sizeof(double); }
    // the eight loss scalars; under MODE_AUX the apply kernel corrects them first, and the running sums go through v_accum (extend_table)
    static void extend_apply_args(const Plan* plan, const ILayout& L, ApplyArgs& a) {
        if (L.mode & MODE_AUX) a.accum = nullptr;
        a.info = 1; a.alpha = (float)plan->info_alpha; a.beta = (float)plan->info_beta; a.gamma = (float)plan->info_gamma;
    }
    // MODE_AUX: the fifth loss sum.  Then the weighted KL term of a finalising launch (train_generic.hip: MStep::extend_table); where the
    // fifth sum is finalised too, its block runs last on the rebuilt ELBO and v_accum takes the running sums.
    static void extend_table(const Plan* plan, const ILayout& L, char* ws, long long*, GApplyArgs& g) {
        if (L.mode & MODE_AUX) {
            g.v_partials = (const double*)(ws + L.o_partials) + 4 * L.rows_grid;
            g.v_accum = (double*)(uintptr_t)plan->loss_accum;
        }
        if (!g.finalize || !kl_weighted(plan)) return;
        g.kl_partials = (const double*)(ws + L.o_partials) + partials_k_off(L); g.kl_stride = 1; g.kl_w = (float)plan->kl_weight;
        if (!(L.mode & MODE_AUX)) { g.kl_accum = g.a.accum; g.a.accum = nullptr; }
    }
};

}  // namespace ti
}  // namespace dvae

using namespace dvae;
using namespace dvae::ti;

extern "C" int dvae_train_info_plan(int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint, dvae_train_info_plan_t* plan) {
    return dvae_train_info_plan_mode(y_dim, z_dim, h1, h2, B, ksplit_hint, 0, plan);
}

extern "C" int dvae_train_info_plan_mode(int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint, int mode, dvae_train_info_plan_t* plan) {
    DVAE_CHECK_ARG(plan, "train_info_plan: null plan");
    DVAE_CHECK_ARG(mode_ok(mode), "train_info_plan: mode 0x%x; the bits are DVAE_INFO_DEC_CLASSIFIER (%d: the decoder is fed the classifier's output; "
                   "otherwise the label) and at most one of DVAE_INFO_AUX_UNIFORM (%d) and DVAE_INFO_AUX_ENTROPY (%d) (the adversarial term on the "
                   "encoder; neither: the cross entropy)", mode, DVAE_INFO_DEC_CLASSIFIER, DVAE_INFO_AUX_UNIFORM, DVAE_INFO_AUX_ENTROPY);
    DVAE_CHECK_ARG(dims_ok(y_dim, z_dim, h1, h2), "train_info_plan: y_dim %d, hidden %d / %d, z_dim %d; %s", y_dim, h1, h2, z_dim, LIMITS);
    DVAE_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 31), "train_info_plan: %lld frames", (long long)B);
    DVAE_CHECK_ARG(ksplit_hint >= 0 && ksplit_hint <= G_MAX_SLICES, "train_info_plan: %d frame slices (0 = choose, at most %d)", ksplit_hint, G_MAX_SLICES);
    const ILayout L = make_layout(y_dim, z_dim, h1, h2, B, ksplit_hint, mode);
    memset(plan, 0, sizeof(*plan));
    plan->info_mode = mode;
    plan->y_dim = y_dim; plan->z_dim = z_dim; plan->h1 = h1; plan->h2 = h2;
    plan->ksplit = L.nslices; plan->n_tensors = I_NT; plan->launches_per_step = I_LAUNCHES; plan->B = B; plan->n_params = L.n_params;
    for (int t = 0; t < I_NT; ++t) { plan->tensor_offset[t] = L.toff[t]; plan->tensor_rows[t] = L.trows[t]; plan->tensor_cols[t] = L.tcols[t]; }
    plan->workspace_bytes = L.ws_bytes; plan->grad_offset_bytes = L.o_grads; plan->Bp = L.Bp; plan->rows_grid = L.rows_grid;
    plan->slice_frames = L.slice_frames; plan->wgrad_items = L.n_items; plan->lds_bytes = L.lds_bytes;
    plan->info_alpha = 0.0; plan->info_beta = 10.0; plan->info_gamma = 1.0;        // scripts/training_M2_info_vad.py:53-55
    plan->kl_weight = 1.0; plan->kl_floor = 0.0;
    return 0;
}

// the entry points: train_step_host.hpp under this step's description
extern "C" int dvae_train_info_repack(const dvae_train_info_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_repack<IStep>("train_info_repack", plan, params, ws, stream);
}

extern "C" int dvae_train_info_init(const dvae_train_info_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_init<IStep>("train_info_init", plan, params, ws, stream);
}

extern "C" int dvae_train_info_grads(const dvae_train_info_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                     const float* eps_noise, float elbo_eps, void* stream) {
    return step_grads<IStep>("train_info_grads", plan, ws, {x, ldx, y, ldy, eps_noise, elbo_eps}, stream);
}

extern "C" int dvae_train_info_apply(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr,
                                     double beta1, double beta2, double adam_eps, double grad_scale, float* losses8, void* stream) {
    return step_apply<IStep>("train_info_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, {losses8, nullptr}, stream);
}

extern "C" int dvae_train_info_reduce(const dvae_train_info_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses8,
                                      void* stream) {
    return step_reduce<IStep>("train_info_reduce", plan, ws, flat, accumulate, weight, {losses8, nullptr}, stream);
}

extern "C" int dvae_train_info_apply_flat(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step,
                                          double lr, double beta1, double beta2, double adam_eps, double grad_scale, void* stream) {
    return step_apply_flat<IStep>("train_info_apply_flat", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, nullptr, stream);
}

extern "C" int dvae_train_info_apply_flat_clipped(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat,
                                                  int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale,
                                                  double max_norm, void* scratch, float* norm2_out, int32_t* skipped_counter, void* stream) {
    const GClipHost clip = {grad_scale, max_norm, scratch, norm2_out, skipped_counter};
    return step_apply_flat<IStep>("train_info_apply_flat_clipped", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, &clip,
                                  stream);
}

extern "C" int dvae_train_info_step(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                                    const float* y, int64_t ldy, const float* eps_noise, float elbo_eps, int step, double lr, double beta1,
                                    double beta2, double adam_eps, float* losses8, void* stream) {
    return step_step<IStep>("train_info_step", "train_info_grads", "train_info_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, 1.0}, ws,
                            {x, ldx, y, ldy, eps_noise, elbo_eps}, {losses8, nullptr}, stream);
}

extern "C" int dvae_train_info_eval(const dvae_train_info_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                    const float* eps_noise, float elbo_eps, float* losses8, void* stream) {
    return step_eval<IStep>("train_info_eval", plan, ws, {x, ldx, y, ldy, eps_noise, elbo_eps}, {losses8, nullptr}, stream);
}


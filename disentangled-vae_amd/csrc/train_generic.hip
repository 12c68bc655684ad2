// The fused train step for M1 / M2 models of ANY covered size, exact fp32, three launches per step (include/dvae_train.h:
// dvae_train_generic_*; disentangled-vae_amd/trainer_generic.py).  The resident step (train_rows*.hip, train_wgrad.hip, train_fused.hip)
// is written for 513-128-128-16 and stays the default there; this file serves every other size within the limits of
// dvae_mcem_plan_dims -- x 513, y_dim 0..513, h1 / h2 1..512, z 1..128 -- and the reference geometry too when asked.
//
// The design is mlp_generic.hip's, carried through the backward pass:
//   * rows kernel: 256 threads own a tile of 16 frames.  Products run on v_mfma_f32_16x16x4_f32: 16 weight rows are the A operand, the
//     tile's 16 frames the B columns; the four waves split a layer's row tiles.  Weights stream from packed copies in fragment order,
//     zero-padded to multiples of 16 (runtime trip counts, no tails); the x / z block and the label block are padded separately and
//     summed x (z) first, then y.  The backward-data products read a second, transposed packed copy.  Activations sit in LDS as
//     [k][16]: the x tile (its place later takes d loss / d a), the label tile, two hidden tiles of max(h1, h2, z) rows and three
//     latent tiles (mu / B, the KL part of d log_var, eps std / 2 -- then d mu, d log_var): 154 KB at 512 / 512 / z 128 / y 513, sized
//     from the dims at launch.  The hidden activations of the encoder are NOT kept for the backward pass: every layer input and every
//     pre-activation gradient goes to the stash ([frame][S] floats, 16-byte stores straight from the accumulators) for the weight
//     gradients anyway, and the thread that wrote h reads it back where tanh' needs it.
//     Frames past B carry zero pre-activation gradients and finite activations; padded units carry zeros throughout.
//   * weight-gradient, apply, reduce and norm kernels: train_tables.hip, which the M2_info and the classifier step launch too; here one
//     weight-gradient launch covers the seven matrices and their biases.  The host path around the launches is train_step_host.hpp's,
//     shared with those two steps; this file describes the step to it (MStep).
//   * module modes of the rows kernel (dvae_module_generic_forward / _backward; module_path.py: GenericModuleEngine): the forward chain
//     with the model's outputs written, and the backward chain started from upstream gradients of (r, z, mu, log_var) in the place of
//     the ELBO's -- the drop-in modules' forward as ONE autograd Function under the caller's own loss and optimizer.
//   * the M2_info body in the module modes (DEC; plans of dvae_module_generic_plan, model M2_DEC): encoder layer 1 on x alone -- W1y
//     has no elements --, the label tile for decoder layer 1 only, and in the backward mode the label gradient g_y = dpre_d1 D1[:, z:]
//     beside dz, from one more transposed copy D1yT behind the last packed copy (dvae_module_generic_backward_y).  The weight-gradient,
//     reduce and apply kernels are the same code on this plan's tables.
//   * 64-bit indexing throughout; a gather index outside [0, row_count) is never dereferenced (row 0 instead, counted).
#include <math.h>
#include <vector>
#include "common.hpp"
#include "../../include/dvae_train.h"
#include "train_step_host.hpp"

namespace dvae {
namespace tg {

struct GLayout {
    int y, z, h1, h2, yp, zp, h1p, h2p, hm;     // sizes and their multiples of 16 (yp 0 without labels); hm = max(h1p, h2p, zp)
    int dec;                                    // M2_DEC (dvae_module_generic_plan): the encoder reads x alone.  In the four bytes that padded hm: no other field moves
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
    // std_norm (dvae_train_generic_plan_norm): encoder layer 1 reads the standardised x; its stash block of GXP columns sits behind s_da, so
    // every other column, S and the workspace of a plan without std_norm are what they are without these two fields
    int norm, s_xn;
};

static_assert(offsetof(GLayout, W1x) == 40 && offsetof(GLayout, dec) == 36, "dec sits in the padding behind hm: the kernel arguments of the train step do not move");

static void make_gemms(const GLayout& L, GGemm* G);
constexpr int M_NT = 14, M_NG = 7;               // this step's share of the tables (G_NT / G_NG entries: train_tables.hpp)

static bool dims_ok(int y, int z, int h1, int h2) {
    return y >= 0 && y <= GX && h1 >= 1 && h1 <= G_HMAX && h2 >= 1 && h2 <= G_HMAX && z >= 1 && z <= G_ZMAX;
}

static GLayout make_layout(int y, int z, int h1, int h2, int64_t B, int ksplit_hint, bool norm, bool dec = false) {
    GLayout L;
    memset(&L, 0, sizeof(L));
    L.y = y; L.z = z; L.h1 = h1; L.h2 = h2; L.dec = dec ? 1 : 0;
    L.yp = y ? up16(y) : 0; L.zp = up16(z); L.h1p = up16(h1); L.h2p = up16(h2);
    L.hm = L.h1p > L.h2p ? L.h1p : L.h2p;
    if (L.zp > L.hm) L.hm = L.zp;
    // parameters: state_dict order, 256-byte aligned
    const int rows[M_NT] = {h1, h1, h2, h2, z, z, z, z, h2, h2, h1, h1, GX, GX};
    const int cols[M_NT] = {GX + (dec ? 0 : y), 1, h1, 1, h2, 1, h2, 1, z + y, 1, h2, 1, h1, 1};
    int64_t o = 0;
    for (int t = 0; t < M_NT; ++t) {
        L.toff[t] = o; L.trows[t] = rows[t]; L.tcols[t] = cols[t];
        o = al64(o + (int64_t)rows[t] * cols[t]);
    }
    L.n_params = o;
    // packed copies
    o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o = al64(o + n); return at; };
    L.W1x = take((int64_t)L.h1p * GXP); L.W1y = take(dec ? 0 : (int64_t)L.h1p * L.yp);
    L.W2 = take((int64_t)L.h2p * L.h1p); L.Wh = take((int64_t)2 * L.zp * L.h2p);
    L.D1z = take((int64_t)L.h2p * L.zp); L.D1y = take((int64_t)L.h2p * L.yp);
    L.D2 = take((int64_t)L.h1p * L.h2p); L.D3 = take((int64_t)GXP * L.h1p);
    L.D3T = take((int64_t)L.h1p * GXP); L.D2T = take((int64_t)L.h2p * L.h1p); L.D1zT = take((int64_t)L.zp * L.h2p);
    L.WhT = take((int64_t)L.h2p * 2 * L.zp); L.W2T = take((int64_t)L.h1p * L.h2p);
    L.b1 = take(L.h1p); L.b2 = take(L.h2p); L.bh = take(2 * L.zp); L.bd1 = take(L.h2p); L.bd2 = take(L.h1p); L.bd3 = take(GXP);
    if (dec) take((int64_t)L.yp * L.h2p);                  // D1yT, behind the last packed copy: d1yT_off
    L.wpack_elems = o;
    // the stash of a frame
    int s = 0;
    auto col = [&](int n) { const int at = s; s += n; return at; };
    L.s_h1e = col(L.h1p); L.s_h2e = col(L.h2p); L.s_z = col(L.zp); L.s_d1 = col(L.h2p); L.s_d2 = col(L.h1p);
    L.s_pe1 = col(L.h1p); L.s_pe2 = col(L.h2p); L.s_ph = col(2 * L.zp); L.s_pd1 = col(L.h2p); L.s_pd2 = col(L.h1p); L.s_da = col(GXP);
    L.norm = norm ? 1 : 0;
    if (norm) L.s_xn = col(GXP);                          // behind every other block: their columns do not move
    L.S = s;
    // frames, tiles, slices
    L.B = B;
    L.tiles = (B + GT - 1) / GT;
    L.Bp = L.tiles * GT;
    L.rows_grid = L.tiles < G_ROWS_GRID ? L.tiles : G_ROWS_GRID;
    GGemm gm[M_NG];
    make_gemms(L, gm);
    int row_tiles = 0;                                    // weight-gradient items of one frame slice
    for (int i = 0; i < M_NG; ++i) row_tiles += gemm_items(gm[i]);
    choose_slices(B, row_tiles, ksplit_hint, L.slice_frames, L.nslices);
    L.n_items = row_tiles * L.nslices;
    // workspace
    int64_t w = al256(L.wpack_elems * 4);
    L.o_items = w; w = al256(w + (int64_t)L.n_items * sizeof(GItem));
    L.o_partials = w; w = al256(w + L.rows_grid * 4 * sizeof(double));
    L.o_stash = w; w = al256(w + L.Bp * (int64_t)L.S * 4);
    L.o_grads = w; w = al256(w + (int64_t)L.nslices * L.n_params * 4);
    L.ws_bytes = w;
    L.lds_bytes = (int64_t)GT * (GXP + L.yp + 2 * L.hm + 3 * L.zp) * 4 + GT * sizeof(int64_t);
    return L;
}

// DEC: the transposed copy of decoder layer 1's label columns ([yp][h2p], fragment order as D1zT) starts where the packed copies of a
// plan without it end
static int64_t d1yT_off(const GLayout& L) { return al64(L.bd3 + GXP); }

static void make_tensors(const GLayout& L, GTensor* T) {
    for (int t = 0; t < G_NT; ++t) {
        GTensor& d = T[t];
        memset(&d, 0, sizeof(d));
        d.off = L.toff[t]; d.rows = L.trows[t]; d.cols = L.tcols[t];
        d.f0 = d.f1 = 0; d.t0 = -1; d.split = d.cols; d.bias = t & 1;
    }
    const int k1 = L.h1p / 16, k2 = L.h2p / 16, kz = L.zp / 16, ky = L.yp / 16;
    T[0].f0 = L.W1x; T[0].kb0 = GKX; T[0].split = GX; T[0].f1 = L.W1y; T[0].kb1 = ky;
    T[1].f0 = L.b1;
    T[2].f0 = L.W2; T[2].kb0 = k1; T[2].t0 = L.W2T; T[2].tkb = k2; T[2].tcmax = L.h1;
    T[3].f0 = L.b2;
    T[4].f0 = L.Wh; T[4].kb0 = k2; T[4].t0 = L.WhT; T[4].tkb = 2 * kz; T[4].tcmax = L.h2;
    T[5].f0 = L.bh;
    T[6].f0 = L.Wh; T[6].kb0 = k2; T[6].roff = L.zp; T[6].t0 = L.WhT; T[6].tkb = 2 * kz; T[6].tkoff = L.zp; T[6].tcmax = L.h2;
    T[7].f0 = L.bh; T[7].roff = L.zp;
    T[8].f0 = L.D1z; T[8].kb0 = kz; T[8].split = L.z; T[8].f1 = L.D1y; T[8].kb1 = ky; T[8].t0 = L.D1zT; T[8].tkb = k2; T[8].tcmax = L.z;
    T[9].f0 = L.bd1;
    T[10].f0 = L.D2; T[10].kb0 = k2; T[10].t0 = L.D2T; T[10].tkb = k1; T[10].tcmax = L.h2;
    T[11].f0 = L.bd2;
    T[12].f0 = L.D3; T[12].kb0 = k1; T[12].t0 = L.D3T; T[12].tkb = GKX; T[12].tcmax = L.h1;
    T[13].f0 = L.bd3;
    if (L.dec) {                                          // W1y is empty: every column of tensor 0 is x; the label columns of tensor 8 also go to D1yT
        T[0].kb1 = 0;
        T[8].t1 = d1yT_off(L); T[8].tkb1 = k2;
    }
}

static void make_gemms(const GLayout& L, GGemm* G) {
    auto set = [&](int i, int dpre, int nrt, int rows, int wt, int kind, int in_off, int in_w, int y_w) {
        GGemm& m = G[i];
        memset(&m, 0, sizeof(m));
        m.dpre = dpre; m.nrt = nrt; m.rows = rows; m.wt = wt; m.bt = wt + 1; m.in_kind = kind; m.in_off = in_off; m.in_w = in_w; m.y_w = y_w;
        m.cols = in_w + y_w;
    };
    const int y0 = L.dec ? 0 : L.y;                       // DEC: the encoder does not see the labels
    if (L.norm) set(0, L.s_pe1, L.h1p / 16, L.h1, 0, 1, L.s_xn, GX, y0);       // the standardised x from the stash, labels behind it as in decoder layer 1
    else set(0, L.s_pe1, L.h1p / 16, L.h1, 0, 0, 0, GX, y0);
    set(1, L.s_pe2, L.h2p / 16, L.h2, 2, 1, L.s_h1e, L.h1, 0);
    set(2, L.s_ph, L.zp / 16, L.z, 4, 1, L.s_h2e, L.h2, 0);
    set(3, L.s_ph + L.zp, L.zp / 16, L.z, 6, 1, L.s_h2e, L.h2, 0);
    set(4, L.s_pd1, L.h2p / 16, L.h2, 8, 1, L.s_z, L.z, L.y);
    set(5, L.s_pd2, L.h1p / 16, L.h1, 10, 1, L.s_d1, L.h2, 0);
    set(6, L.s_da, GKX, GX, 12, 1, L.s_d2, L.h1, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rows kernel
struct GRowsArgs {
    const float* x; int64_t ldx;
    const float* y; int64_t ldy;
    const float* eps;                 // [B][z]
    const int64_t* row_index; int64_t row_count; int* bad;
    float* ws;                        // the packed copies start the workspace
    float* stash; double* partials;
    float elbo_eps, invB;
    int fwd_only;
    const float* nmean; const float* ndiv;    // NORM: [513] the mean and fl32(std + fl32(norm_eps)) of the standardised encoder input
    // the weighted KL term (plan->kl_weight w, plan->kl_floor): kl_scale = fl32(fl32(w) * invB) -- invB itself at w = 1 --, the scale of the
    // KL parts of d mu and d log_var where the element k = -0.5 (lv - mu^2 - e^lv) is not below kl_floor; they are exact zeros below it
    float kl_scale, kl_floor;
};
// the module modes (dvae_module_generic_forward / _backward): the model's outputs, or the upstream gradients of them (each may be null)
struct GModuleArgs {
    // what the kernel writes row by row: forward r [B][513]; backward (DEC) the label gradient [B][y], null: not asked for.  One mode
    // writes one of them, so they share their place and the arguments of the instantiations without DEC stay where they were
    union { float* out_r; float* out_gy; };
    union { int64_t ld_r; int64_t ld_gy; };
    float* out_mu; float* out_lv; float* out_z;       // [B][z]; out_z may be null
    const float* g_r; int64_t ld_gr;  // [B][513]
    const float* g_mu; const float* g_lv; const float* g_z;       // [B][z]
};
constexpr int ROWS_STEP = 0, ROWS_MODULE_FWD = 1, ROWS_MODULE_BWD = 2;

// NORM (std_norm): encoder layer 1 reads xn = fl32(fl32(x - mean) / div) in the place of x -- the tile holds xn, which also goes to the
// stash block s_xn for the weight gradient of that layer --, and the output layer takes the raw x of its loss terms from the caller's
// memory again.  Everything else is the same code.
// MODE (ROWS_STEP: the train step and its forward-only evaluation, the code it was before the other two existed):
//   ROWS_MODULE_FWD  the forward chain alone -- no stash, no loss sums, no partials -- with the model's outputs written: r = exp(a) as four
//                    consecutive bins of a lane's frame, mu, log_var and z from the reparametrisation phase.  Padded bins, padded latent
//                    columns and frames past B are never written.
//   ROWS_MODULE_BWD  the forward recomputed with the stash writes of a train step, then the same backward phases from upstream gradients
//                    in the place of the ELBO's: da = g_r r; dz = dpre_d1 D1[:, :z] + g_z; d mu = dz + g_mu; d log_var = dz std eps / 2 +
//                    g_lv.  No 1 / B and no KL term: the upstream gradients carry both.  A null pointer is a zero gradient; a frame past
//                    B, a padded bin and a padded latent column contribute exact zeros.  The weight-gradient and reduce kernels read
//                    the stash this leaves as they read a train step's.
// DEC (the module modes on an M2_DEC plan): encoder layer 1 is the x product alone; the label tile is staged as ever and read by decoder
//   layer 1.  In the backward mode the dz phase has ky more row tiles behind its kz: g_y = dpre_d1 D1[:, z:] on D1yT, a lane's four
//   consecutive label columns of its frame stored straight from the accumulator -- no LDS, no further barrier.  The encoder gives g_y
//   nothing, and there is no 1 / B.  A frame past B, a column >= y and the padding of a row are never written; out_gy null: the tiles
//   are not computed.
// KLW (ROWS_STEP only; plan->kl_weight / kl_floor other than 1 / 0): the KL parts of d mu and d log_var carry kl_scale = w / B where the
//   element k = -0.5 (lv - mu^2 - e^lv) is not below kl_floor and are exact zeros below it, and the workgroup's third partial is the sum
//   of max(k, kl_floor).  A template flag and not the two scalars alone: the instantiations without it are the code they were,
//   instruction for instruction (DESIGN 4a': the resource table).
template <bool NORM, int MODE = ROWS_STEP, bool DEC = false, bool KLW = false>
__global__ __launch_bounds__(256) void train_generic_rows_kernel(const GLayout L, const GRowsArgs g, const GModuleArgs mo) {
    static_assert(MODE == ROWS_STEP || !NORM, "the module modes take the encoder input as it is given");
    static_assert(!DEC || MODE != ROWS_STEP, "there is no train step on an M2_DEC plan");
    static_assert(!KLW || MODE == ROWS_STEP, "the module modes' upstream gradients carry the loss");
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    float* X = gsm;                                     // [528][16] x, then d loss / d a
    float* Y = X + GT * GXP;                            // [yp][16]
    float* A = Y + GT * L.yp;                           // [hm][16] h1e, d1, dpre_d1
    float* Bf = A + GT * L.hm;                          // [hm][16] h2e, z, d2, dpre_d2, dpre_e2
    float* C = Bf + GT * L.hm;                          // [3 zp][16] heads; then mu / B | KL part of d log_var | eps std / 2; then d mu | d log_var
    int64_t* srow = reinterpret_cast<int64_t*>(C + GT * 3 * L.zp);     // [16] the frame's row of x / y, -1: past B

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int ky = L.yp >> 4, k1 = L.h1p >> 4, k2 = L.h2p >> 4, kz = L.zp >> 4;
    const float* wp = g.ws;
    const bool bwd = MODE == ROWS_MODULE_BWD || (MODE == ROWS_STEP && !g.fwd_only);
    double sum_is = 0.0, sum_kl = 0.0;
    [[maybe_unused]] double sum_kc = 0.0;               // KLW: the KL elements clamped from below at kl_floor

    for (int64_t tile = blockIdx.x; tile < L.tiles; tile += gridDim.x) {
        const int64_t r0 = tile * GT;
        __syncthreads();                                // the previous tile's readers of srow, X and C are done
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

        // ---- the input tile: a quarter wave reads 16 consecutive inputs of one frame ----
        for (int b = wave; b < GKX; b += 4) {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
                const int k = 16 * b + col, c = 4 * cq + quad;
                const int64_t s = srow[c];
                float xv = (k < GX && s >= 0) ? g.x[s * g.ldx + k] : 0.f;
                if (NORM) {
                    // torch's (x - mean) / div: two correctly rounded operations; padded bins and frames past B stay exact zeros
                    if (k < GX && s >= 0) xv = __fdiv_rn(__fsub_rn(xv, g.nmean[k]), g.ndiv[k]);
                    if (bwd) g.stash[(r0 + c) * (int64_t)L.S + L.s_xn + k] = xv;
                }
                X[k * GT + c] = xv;
            }
        }
        for (int b = wave; b < ky; b += 4) {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
                const int k = 16 * b + col, c = 4 * cq + quad;
                const int64_t s = srow[c];
                Y[k * GT + c] = (k < L.y && s >= 0) ? g.y[s * g.ldy + k] : 0.f;
            }
        }
        __syncthreads();

        // ---- encoder layer 1: h1e = tanh([x | y] W1^T + b1) -> A ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W1x + (int64_t)t * GKX * 256, GKX, X, lane);
            if constexpr (!DEC) acc = tg_gemm(acc, wp + L.W1y + (int64_t)t * ky * 256, ky, Y, lane);
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
        // ---- encoder layer 2: h2e = tanh(h1e W2^T + b2) -> Bf ----
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
        // ---- z = mu + exp(log_var / 2) eps -> Bf; the KL terms; what the backward pass needs of the heads -> C ----
        for (int i = tid; i < GT * L.zp; i += 256) {
            const int c = i & 15, j = i >> 4;
            const bool ok = srow[c] >= 0 && j < L.z;
            const float mu = C[j * GT + c], lv = C[(L.zp + j) * GT + c];
            const float e = ok ? g.eps[(r0 + c) * L.z + j] : 0.f;
            const float sd = expf(0.5f * lv), ev = expf(lv);
            const float zv = mu + sd * e;
            Bf[j * GT + c] = zv;
            if constexpr (MODE == ROWS_STEP) {
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
            } else if constexpr (MODE == ROWS_MODULE_FWD) {
                if (ok) {
                    const int64_t o = (r0 + c) * L.z + j;
                    mo.out_mu[o] = mu; mo.out_lv[o] = lv;
                    if (mo.out_z) mo.out_z[o] = zv;
                }
            } else {                                    // the upstream gradients of mu and log_var in the place of the KL parts
                const int64_t o = (r0 + c) * L.z + j;
                C[j * GT + c] = (ok && mo.g_mu) ? mo.g_mu[o] : 0.f;
                C[(L.zp + j) * GT + c] = (ok && mo.g_lv) ? mo.g_lv[o] : 0.f;
                C[(2 * L.zp + j) * GT + c] = 0.5f * sd * e;
            }
            if (bwd) g.stash[(r0 + c) * (int64_t)L.S + L.s_z + j] = zv;
        }
        __syncthreads();
        // ---- decoder layer 1: d1 = tanh([z | y] D1^T + b) -> A ----
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
        // ---- decoder layer 2: d2 = tanh(d1 D2^T + b) -> Bf ----
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
        // ---- output layer: a = d2 D3^T + b, r = exp(a); Itakura-Saito x / r - log(x + eps) + a - 1; d loss / d a = (1 - x / r) / B -> X ----
        for (int t = wave; t < GKX; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            float xraw[4] = {0.f, 0.f, 0.f, 0.f};
            if (NORM && fok) {                          // requested before the product: four consecutive bins of this lane's frame
                const float* xp = g.x + srow[col] * g.ldx + 16 * t + 4 * quad;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * t + 4 * quad + r < GX) xraw[r] = xp[r];
            }
            f32x4 gr = {0.f, 0.f, 0.f, 0.f};
            if constexpr (MODE == ROWS_MODULE_BWD) {   // requested before the product as well: four consecutive bins of this lane's frame
                if (fok && mo.g_r) {
                    const float* gp = mo.g_r + (r0 + col) * mo.ld_gr + 16 * t + 4 * quad;
                    if (16 * t + 4 * quad + 3 < GX) gr = reinterpret_cast<const G4U*>(gp)->v;
                    else if (16 * t + 4 * quad < GX) gr[0] = gp[0];         // bin 512 (513 = 4 * 128 + 1: a group holds four bins or this one)
                }
            }
            acc = tg_gemm(acc, wp + L.D3 + (int64_t)t * k1 * 256, k1, Bf, lane);
            if constexpr (MODE == ROWS_MODULE_FWD) {
                f32x4 rv;
#pragma unroll
                for (int r = 0; r < 4; ++r) rv[r] = expf(acc[r] + wp[L.bd3 + 16 * t + 4 * quad + r]);
                if (fok) {
                    float* rp = mo.out_r + (r0 + col) * mo.ld_r + 16 * t + 4 * quad;
                    if (16 * t + 4 * quad + 3 < GX) reinterpret_cast<G4U*>(rp)->v = rv;
                    else if (16 * t + 4 * quad < GX) rp[0] = rv[0];
                }
                continue;
            }
            f32x4 da;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const bool ok = fok && row < GX;
                const float a = acc[r] + wp[L.bd3 + row];
                if constexpr (MODE == ROWS_MODULE_BWD) {
                    da[r] = (ok && mo.g_r) ? gr[r] * expf(a) : 0.f;
                } else {
                    const float xv = NORM ? xraw[r] : X[row * GT + col];
                    const float q = xv * expf(-a);
                    if (ok) sum_is += (double)(q - logf(xv + g.elbo_eps) + a - 1.f);
                    da[r] = ok ? (1.f - q) * g.invB : 0.f;
                }
                if (bwd) X[row * GT + col] = da[r];
            }
            st4(L.s_da, t, da);
        }
        if (!bwd) continue;
        __syncthreads();
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
        // ---- d d1 = dpre_d2 D2; dpre_d1 = d d1 (1 - d1^2) -> A ----
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
        // ---- dz = dpre_d1 D1[:, :z]; d mu = dz + mu / B; d log_var = dz eps std / 2 + its KL part -> C rows 0 .. 2 zp - 1 ----
        const int ndz = (DEC && MODE == ROWS_MODULE_BWD && mo.out_gy) ? kz + ky : kz;
        const int64_t D1yT = (L.bd3 + GXP + 63) / 64 * 64;       // d1yT_off(L): behind the last packed copy
        for (int t = wave; t < ndz; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DEC && MODE == ROWS_MODULE_BWD) {
                if (t >= kz) {                          // g_y = dpre_d1 D1[:, z:]: label columns 16 (t - kz) + 4 quad .. + 3 of this lane's frame
                    const int c0 = 16 * (t - kz) + 4 * quad;
                    acc = tg_gemm(acc, wp + D1yT + (int64_t)(t - kz) * k2 * 256, k2, A, lane);
                    if (fok) {
                        float* gp = mo.out_gy + (r0 + col) * mo.ld_gy + c0;
                        if (c0 + 3 < L.y) reinterpret_cast<G4U*>(gp)->v = acc;
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (c0 + r < L.y) gp[r] = acc[r];
                        }
                    }
                    continue;
                }
            }
            float gz[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (MODE == ROWS_MODULE_BWD) {   // the upstream gradient of z: four consecutive columns of this lane's frame
                if (fok && mo.g_z) {
                    const float* zp_ = mo.g_z + (r0 + col) * L.z + 16 * t + 4 * quad;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (16 * t + 4 * quad + r < L.z) gz[r] = zp_[r];
                }
            }
            acc = tg_gemm(acc, wp + L.D1zT + (int64_t)t * k2 * 256, k2, A, lane);
            if constexpr (MODE == ROWS_MODULE_BWD) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += gz[r];
            }
            f32x4 dm, dl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                dm[r] = acc[r] + C[row * GT + col];
                dl[r] = acc[r] * C[(2 * L.zp + row) * GT + col] + C[(L.zp + row) * GT + col];
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
    if constexpr (MODE != ROWS_STEP) return;           // no loss sums, no partials
    // the workgroup's loss sums: waves in order
    sum_is = wave_sum(sum_is); sum_kl = wave_sum(sum_kl);
    if constexpr (KLW) sum_kc = wave_sum(sum_kc);
    __syncthreads();                                    // the last tile's readers of X are done: its first bytes hold the sums
    double (*red)[2] = reinterpret_cast<double (*)[2]>(gsm);
    [[maybe_unused]] double* redk = reinterpret_cast<double*>(gsm) + 8;
    if (lane == 0) {
        red[wave][0] = sum_is; red[wave][1] = sum_kl;
        if constexpr (KLW) redk[wave] = sum_kc;
    }
    __syncthreads();
    if (tid == 0) {
        double* p = g.partials + 4 * (int64_t)blockIdx.x;
        p[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        p[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        if constexpr (KLW) p[2] = ((redk[0] + redk[1]) + redk[2]) + redk[3];     // the clamped KL sum (GApplyArgs: kl_partials)
        else p[2] = 0.0;
        p[3] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
template <bool NORM, int MODE, bool DEC, bool KLW>
static int launch_rows_as(const GLayout& L, const GRowsArgs& g, const GModuleArgs& mo, hipStream_t s) {
    static bool attr_done[64] = {};                     // (one per instantiation: the limit is a property of the kernel)
    if (int rc = raise_lds_limit((const void*)train_generic_rows_kernel<NORM, MODE, DEC, KLW>, "train_generic_rows_kernel", L.lds_bytes, attr_done)) return rc;
    hipLaunchKernelGGL((train_generic_rows_kernel<NORM, MODE, DEC, KLW>), dim3((unsigned)L.rows_grid), dim3(256), (size_t)L.lds_bytes, s, L, g, mo);
    DVAE_LAUNCH_OK("train_generic_rows_kernel");
    return 0;
}

// the M1 / M2 step as train_step_host.hpp reads it
struct MStep {
    using Plan = dvae_train_generic_plan_t;
    using Layout = GLayout;
    static constexpr int NT = M_NT, NG = M_NG;
    static constexpr int ORDER[M_NG] = {0, 6, 4, 1, 5, 2, 3};               // the widest inputs first: their items run longest
    static constexpr bool COUNTS = false, WGRAD_Y = true;

    // dec_ok: the entry point serves the M2_DEC plans of dvae_module_generic_plan too (init, repack, the module modes); the train-step
    // entry points do not
    static int plan_layout(const char* who, const Plan* plan, GLayout& L, bool dec_ok) {
        DVAE_CHECK_ARG(plan, "%s: null plan", who);
        const bool dec = plan->model == DVAE_MODEL_M2_DEC;
        DVAE_CHECK_ARG(!dec || dec_ok, "%s: a plan of model M2_DEC (dvae_module_generic_plan: the module entry points serve it; there is no train step "
                       "on the M2_info body alone -- dvae_train_info_* trains the whole model)", who);
        DVAE_CHECK_ARG((plan->model == DVAE_MODEL_M1 || plan->model == DVAE_MODEL_M2 || dec) && plan->precision == DVAE_PREC_F32 &&
                       dims_ok(plan->y_dim, plan->z_dim, plan->h1, plan->h2) && (plan->model == DVAE_MODEL_M1) == (plan->y_dim == 0) && plan->B >= 1,
                       "%s: not a plan of dvae_train_generic_plan / dvae_module_generic_plan", who);
        DVAE_CHECK_ARG(plan->std_norm == 0 || plan->std_norm == 1, "%s: std_norm %d in the plan (0 or 1)", who, plan->std_norm);
        DVAE_CHECK_ARG(!dec || !plan->std_norm, "%s: std_norm on a plan of model M2_DEC", who);
        DVAE_CHECK_ARG(plan->kl_weight >= 0.0 && isfinite(plan->kl_weight) && plan->kl_floor >= 0.0 && isfinite(plan->kl_floor),
                       "%s: kl_weight %g / kl_floor %g in the plan (finite numbers >= 0; the planner sets 1 and 0)", who, plan->kl_weight, plan->kl_floor);
        L = make_layout(plan->y_dim, plan->z_dim, plan->h1, plan->h2, plan->B, plan->ksplit, plan->std_norm != 0, dec);
        DVAE_CHECK_ARG(L.ws_bytes == plan->workspace_bytes && L.nslices == plan->ksplit && L.n_params == plan->n_params &&
                       L.slice_frames == plan->slice_frames, "%s: the plan was changed after dvae_train_generic_plan", who);
        return 0;
    }

    static int check_inputs(const char* who, const Plan* plan, const void* ws, const StepInputs& in) {
        DVAE_CHECK_ARG(ws && in.x && in.eps, "%s: null pointer", who);
        DVAE_CHECK_ARG(in.ldx >= GX && in.ldx < ((int64_t)1 << 20), "%s: leading dimension of x %lld (at least 513)", who, (long long)in.ldx);
        DVAE_CHECK_ARG((plan->y_dim > 0) == (in.y != nullptr), "%s: y must be given exactly when y_dim > 0 (y_dim %d)", who, plan->y_dim);
        DVAE_CHECK_ARG(!in.y || (in.ldy >= plan->y_dim && in.ldy < ((int64_t)1 << 20)), "%s: leading dimension of y %lld for y_dim %d", who,
                       (long long)in.ldy, plan->y_dim);
        DVAE_CHECK_ARG(!plan->row_index || plan->row_count >= 1, "%s: a gather table needs row_count >= 1 (got %lld)", who, (long long)plan->row_count);
        DVAE_CHECK_ARG(!plan->std_norm || (plan->norm_mean && plan->norm_div && (plan->norm_mean & 3) == 0 && (plan->norm_div & 3) == 0),
                       "%s: a plan with std_norm needs the device tables norm_mean and norm_div (513 floats each)", who);
        return 0;
    }

    static int launch_rows(const Plan* plan, const GLayout& L, char* ws, const StepInputs& in, bool fwd_only, hipStream_t s, int mode = ROWS_STEP,
                           const GModuleArgs* module = nullptr) {
        const bool dec = L.dec != 0;
        DVAE_CHECK_ARG(!dec || mode != ROWS_STEP, "train_generic_rows_kernel: no train step on a plan of model M2_DEC");
        GModuleArgs mo;
        memset(&mo, 0, sizeof(mo));
        if (module) mo = *module;
        GRowsArgs g;
        memset(&g, 0, sizeof(g));
        g.x = in.x; g.ldx = in.ldx; g.y = in.y; g.ldy = in.ldy; g.eps = in.eps;
        g.row_index = (const int64_t*)(uintptr_t)plan->row_index; g.row_count = plan->row_count; g.bad = (int*)(uintptr_t)plan->bad_row_counter;
        g.ws = (float*)ws; g.stash = (float*)(ws + L.o_stash); g.partials = (double*)(ws + L.o_partials);
        g.elbo_eps = in.loss_eps; g.invB = (float)(1.0 / (double)L.B); g.fwd_only = fwd_only ? 1 : 0;
        g.kl_scale = (float)plan->kl_weight * g.invB; g.kl_floor = (float)plan->kl_floor;        // (read by the KLW instantiations)
        if (mode == ROWS_MODULE_FWD) return dec ? launch_rows_as<false, ROWS_MODULE_FWD, true, false>(L, g, mo, s) : launch_rows_as<false, ROWS_MODULE_FWD, false, false>(L, g, mo, s);
        if (mode == ROWS_MODULE_BWD) return dec ? launch_rows_as<false, ROWS_MODULE_BWD, true, false>(L, g, mo, s) : launch_rows_as<false, ROWS_MODULE_BWD, false, false>(L, g, mo, s);
        const bool klw = kl_weighted(plan);
        if (!L.norm) return klw ? launch_rows_as<false, ROWS_STEP, false, true>(L, g, mo, s) : launch_rows_as<false, ROWS_STEP, false, false>(L, g, mo, s);
        g.nmean = (const float*)(uintptr_t)plan->norm_mean; g.ndiv = (const float*)(uintptr_t)plan->norm_div;
        return klw ? launch_rows_as<true, ROWS_STEP, false, true>(L, g, mo, s) : launch_rows_as<true, ROWS_STEP, false, false>(L, g, mo, s);
    }

    static void tensors(const GLayout& L, GTensor* T) { make_tensors(L, T); }
    static void gemms(const GLayout& L, GGemm* G) { make_gemms(L, G); }
    static size_t partials_bytes(const GLayout& L) { return (size_t)L.rows_grid * 4 * sizeof(double); }
    static void extend_apply_args(const Plan*, const GLayout&, ApplyArgs&) {}
    // The weighted KL term of a finalising launch: the finalising workgroup takes the clamped KL sums (slot 2 of the rows kernel's partials),
    // and the running sums go through kl_accum.
    static void extend_table(const Plan* plan, const GLayout& L, char* ws, long long*, GApplyArgs& g) {
        if (!g.finalize || !kl_weighted(plan)) return;
        g.kl_partials = (const double*)(ws + L.o_partials) + 2; g.kl_stride = 4; g.kl_w = (float)plan->kl_weight;
        g.kl_accum = g.a.accum; g.a.accum = nullptr;
    }
};

}  // namespace tg
}  // namespace dvae

using namespace dvae;
using namespace dvae::tg;

static void fill_plan(dvae_train_generic_plan_t* plan, const GLayout& L, int model, int precision, int std_norm) {
    memset(plan, 0, sizeof(*plan));
    plan->std_norm = std_norm;
    plan->kl_weight = 1.0; plan->kl_floor = 0.0;
    plan->model = model; plan->y_dim = L.y; plan->z_dim = L.z; plan->h1 = L.h1; plan->h2 = L.h2; plan->precision = precision;
    plan->ksplit = L.nslices; plan->n_tensors = M_NT; plan->B = L.B; plan->n_params = L.n_params;
    for (int t = 0; t < M_NT; ++t) { plan->tensor_offset[t] = L.toff[t]; plan->tensor_rows[t] = L.trows[t]; plan->tensor_cols[t] = L.tcols[t]; }
    plan->workspace_bytes = L.ws_bytes; plan->grad_offset_bytes = L.o_grads; plan->Bp = L.Bp; plan->rows_grid = L.rows_grid;
    plan->slice_frames = L.slice_frames; plan->wgrad_items = L.n_items; plan->lds_bytes = L.lds_bytes;
}

extern "C" int dvae_train_generic_plan(int model, int y_dim, int z_dim, int h1, int h2, int precision, int64_t B, int ksplit_hint,
                                       dvae_train_generic_plan_t* plan) {
    return dvae_train_generic_plan_norm(model, y_dim, z_dim, h1, h2, precision, B, ksplit_hint, 0, plan);
}

extern "C" int dvae_train_generic_plan_norm(int model, int y_dim, int z_dim, int h1, int h2, int precision, int64_t B, int ksplit_hint,
                                            int std_norm, dvae_train_generic_plan_t* plan) {
    DVAE_CHECK_ARG(plan, "train_generic_plan: null plan");
    DVAE_CHECK_ARG(std_norm == 0 || std_norm == 1, "train_generic_plan: std_norm %d (0: the encoder reads x, 1: the standardised x)", std_norm);
    const char* limits = "the generic train step covers M1 (y_dim 0) and M2 (y_dim 1..513) at x 513, hidden widths 1..512, z_dim 1..128, exact fp32";
    if (model != DVAE_MODEL_M1 && model != DVAE_MODEL_M2) {
        set_error("train_generic_plan: model %d (M2_info and M2_DEC exist at the reference geometry only: dvae_train_plan); %s", model, limits);
        return DVAE_E_UNSUPPORTED;
    }
    if (precision != DVAE_PREC_F32) {
        set_error("train_generic_plan: operand policy %d (the bf16 policies exist at the reference geometry only: dvae_train_plan); %s", precision, limits);
        return DVAE_E_UNSUPPORTED;
    }
    DVAE_CHECK_ARG(dims_ok(y_dim, z_dim, h1, h2), "train_generic_plan: y_dim %d, hidden %d / %d, z_dim %d; %s", y_dim, h1, h2, z_dim, limits);
    DVAE_CHECK_ARG((model == DVAE_MODEL_M1) == (y_dim == 0), "train_generic_plan: model M%d with y_dim %d; %s", model, y_dim, limits);
    DVAE_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 31), "train_generic_plan: %lld frames", (long long)B);
    DVAE_CHECK_ARG(ksplit_hint >= 0 && ksplit_hint <= G_MAX_SLICES, "train_generic_plan: %d frame slices (0 = choose, at most %d)", ksplit_hint, G_MAX_SLICES);
    const GLayout L = make_layout(y_dim, z_dim, h1, h2, B, ksplit_hint, std_norm != 0);
    fill_plan(plan, L, model, precision, std_norm);
    return 0;
}

// the train step's entry points: train_step_host.hpp under this step's description
extern "C" int dvae_train_generic_repack(const dvae_train_generic_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_repack<MStep>("train_generic_repack", plan, params, ws, stream);
}

extern "C" int dvae_train_generic_init(const dvae_train_generic_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_init<MStep>("train_generic_init", plan, params, ws, stream);
}

extern "C" int dvae_train_generic_grads(const dvae_train_generic_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                        const float* eps_noise, float elbo_eps, void* stream) {
    return step_grads<MStep>("train_generic_grads", plan, ws, {x, ldx, y, ldy, eps_noise, elbo_eps}, stream);
}

extern "C" int dvae_train_generic_apply(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr,
                                        double beta1, double beta2, double adam_eps, double grad_scale, float* losses3, void* stream) {
    return step_apply<MStep>("train_generic_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, {losses3, nullptr}, stream);
}

extern "C" int dvae_train_generic_reduce(const dvae_train_generic_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses3,
                                         void* stream) {
    return step_reduce<MStep>("train_generic_reduce", plan, ws, flat, accumulate, weight, {losses3, nullptr}, stream);
}

extern "C" int dvae_train_generic_apply_flat(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat,
                                             int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale, void* stream) {
    return step_apply_flat<MStep>("train_generic_apply_flat", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, nullptr, stream);
}

extern "C" int dvae_train_generic_apply_flat_clipped(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws,
                                                     const float* flat, int step, double lr, double beta1, double beta2, double adam_eps,
                                                     double grad_scale, double max_norm, void* scratch, float* norm2_out,
                                                     int32_t* skipped_counter, void* stream) {
    const GClipHost clip = {grad_scale, max_norm, scratch, norm2_out, skipped_counter};
    return step_apply_flat<MStep>("train_generic_apply_flat_clipped", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, &clip,
                                  stream);
}

extern "C" int dvae_train_generic_step(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                                       const float* y, int64_t ldy, const float* eps_noise, float elbo_eps, int step, double lr, double beta1,
                                       double beta2, double adam_eps, float* losses3, void* stream) {
    return step_step<MStep>("train_generic_step", "train_generic_grads", "train_generic_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, 1.0},
                            ws, {x, ldx, y, ldy, eps_noise, elbo_eps}, {losses3, nullptr}, stream);
}

extern "C" int dvae_train_generic_eval(const dvae_train_generic_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                       const float* eps_noise, float elbo_eps, float* losses3, void* stream) {
    return step_eval<MStep>("train_generic_eval", plan, ws, {x, ldx, y, ldy, eps_noise, elbo_eps}, {losses3, nullptr}, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the whole-model autograd path of the drop-in modules at any covered size (disentangled-vae_amd/module_path.py: GenericModuleEngine)
static int check_module(const char* who, const dvae_train_generic_plan_t* plan, const float* params, const void* ws, const StepInputs& in) {
    DVAE_CHECK_ARG(!plan->std_norm, "%s: a std_norm plan (the module path takes the encoder input as given: normalise x in torch and pass it)", who);
    DVAE_CHECK_ARG(!plan->row_index, "%s: a gather table in the plan (row_index: the module path reads the batch itself)", who);
    DVAE_CHECK_ARG(params, "%s: null pointer", who);
    return MStep::check_inputs(who, plan, ws, in);
}

extern "C" int dvae_module_generic_forward(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                           const float* y, int64_t ldy, const float* eps_noise, float* out_r, int64_t ld_r, float* out_mu,
                                           float* out_lv, float* out_z, int repack, void* stream) {
    GLayout L;
    const StepInputs in = {x, ldx, y, ldy, eps_noise, 0.f};
    if (int rc = MStep::plan_layout("module_generic_forward", plan, L, true)) return rc;
    if (int rc = check_module("module_generic_forward", plan, params, ws, in)) return rc;
    DVAE_CHECK_ARG(out_r && out_mu && out_lv, "module_generic_forward: null pointer (out_z alone may be null)");
    DVAE_CHECK_ARG(ld_r >= GX && ld_r < ((int64_t)1 << 20), "module_generic_forward: ld_r %lld (the leading dimension of out_r: at least 513)", (long long)ld_r);
    hipStream_t s = (hipStream_t)stream;
    if (repack) {                                       // every element of both packed copies from `params`; the padding is dvae_train_generic_init's
        StepUpdate u = {};
        u.params = (float*)params;
        const ApplyArgs a = apply_args<MStep>(plan, L, (char*)ws, u, false, nullptr);
        if (int rc = launch_apply<MStep>(plan, L, a, (char*)ws, false, true, false, nullptr, s)) return rc;
    }
    GModuleArgs mo;
    memset(&mo, 0, sizeof(mo));
    mo.out_r = out_r; mo.ld_r = ld_r; mo.out_mu = out_mu; mo.out_lv = out_lv; mo.out_z = out_z;
    return MStep::launch_rows(plan, L, (char*)ws, in, true, s, ROWS_MODULE_FWD, &mo);
}

static int module_backward(const char* who, const dvae_train_generic_plan_t* plan, const float* params, void* ws, const StepInputs& in,
                           const float* g_r, int64_t ld_gr, const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate,
                           float* g_y, int64_t ld_gy, void* stream) {
    GLayout L;
    if (int rc = MStep::plan_layout(who, plan, L, true)) return rc;
    if (int rc = check_module(who, plan, params, ws, in)) return rc;
    if (int rc = check_reduce_args(who, ws, grad_flat, accumulate, 1.f)) return rc;
    DVAE_CHECK_ARG(!g_r || (ld_gr >= GX && ld_gr < ((int64_t)1 << 20)), "%s: ld_gr %lld (the leading dimension of g_r: at least 513)", who,
                   (long long)ld_gr);
    DVAE_CHECK_ARG(!g_y || L.dec, "%s: g_y on a plan of model %d (the label gradient exists for model M2_DEC alone: dvae_module_generic_plan)", who,
                   plan->model);
    DVAE_CHECK_ARG(!g_y || (ld_gy >= L.y && ld_gy < ((int64_t)1 << 20)), "%s: ld_gy %lld (the leading dimension of g_y: at least y_dim %d)", who,
                   (long long)ld_gy, L.y);
    hipStream_t s = (hipStream_t)stream;
    GModuleArgs mo;
    memset(&mo, 0, sizeof(mo));
    mo.g_r = g_r; mo.ld_gr = ld_gr; mo.g_mu = g_mu; mo.g_lv = g_lv; mo.g_z = g_z;
    mo.out_gy = g_y; mo.ld_gy = ld_gy;
    if (int rc = MStep::launch_rows(plan, L, (char*)ws, in, false, s, ROWS_MODULE_BWD, &mo)) return rc;
    if (int rc = launch_wgrad<MStep>(plan, L, (char*)ws, in, s)) return rc;
    // the slabs in slab order into grad_flat; weight 1: the sum's bits; nothing to finalise, no running sums
    ApplyArgs a = apply_args<MStep>(plan, L, (char*)ws, StepUpdate{}, false, nullptr);
    a.accum = nullptr;
    return launch_reduce<MStep>(plan, L, a, (char*)ws, false, nullptr, grad_flat, accumulate, 1.f, s);
}

extern "C" int dvae_module_generic_backward(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                            const float* y, int64_t ldy, const float* eps_noise, const float* g_r, int64_t ld_gr,
                                            const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate,
                                            void* stream) {
    return module_backward("module_generic_backward", plan, params, ws, {x, ldx, y, ldy, eps_noise, 0.f}, g_r, ld_gr, g_mu, g_lv, g_z, grad_flat,
                           accumulate, nullptr, 0, stream);
}

extern "C" int dvae_module_generic_backward_y(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                              const float* y, int64_t ldy, const float* eps_noise, const float* g_r, int64_t ld_gr,
                                              const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate,
                                              float* g_y, int64_t ld_gy, void* stream) {
    return module_backward("module_generic_backward_y", plan, params, ws, {x, ldx, y, ldy, eps_noise, 0.f}, g_r, ld_gr, g_mu, g_lv, g_z, grad_flat,
                           accumulate, g_y, ld_gy, stream);
}

// Host only.  M1 / M2: dvae_train_generic_plan's plan byte for byte.  M2_DEC: the M2_info body -- tensor 0 [h1, 513], tensor 8 [h2, z + y].
extern "C" int dvae_module_generic_plan(int model, int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint,
                                        dvae_train_generic_plan_t* plan) {
    if (model == DVAE_MODEL_M1 || model == DVAE_MODEL_M2) return dvae_train_generic_plan(model, y_dim, z_dim, h1, h2, DVAE_PREC_F32, B, ksplit_hint, plan);
    DVAE_CHECK_ARG(plan, "module_generic_plan: null plan");
    const char* limits = "the generic module engine covers M1 (y_dim 0), M2 and M2_DEC (the M2_info body: encoder on x alone; y_dim 1..513) at x 513, "
                         "hidden widths 1..512, z_dim 1..128, exact fp32";
    if (model != DVAE_MODEL_M2_DEC) {
        set_error("module_generic_plan: model %d (M2_info as a whole has its own train step, dvae_train_info_plan; its body is model M2_DEC); %s", model, limits);
        return DVAE_E_UNSUPPORTED;
    }
    DVAE_CHECK_ARG(dims_ok(y_dim, z_dim, h1, h2) && y_dim >= 1, "module_generic_plan: model M2_DEC with y_dim %d, hidden %d / %d, z_dim %d; %s", y_dim, h1,
                   h2, z_dim, limits);
    DVAE_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 31), "module_generic_plan: %lld frames", (long long)B);
    DVAE_CHECK_ARG(ksplit_hint >= 0 && ksplit_hint <= G_MAX_SLICES, "module_generic_plan: %d frame slices (0 = choose, at most %d)", ksplit_hint, G_MAX_SLICES);
    const GLayout L = make_layout(y_dim, z_dim, h1, h2, B, ksplit_hint, false, true);
    fill_plan(plan, L, model, DVAE_PREC_F32, 0);
    return 0;
}


// Fused train step for the reference geometry (x 513, h [128,128], z 16, y 0/1/513): see include/dvae_train.h for the three-launch
// structure.  This file is the host side only: plan and workspace layout, the tables the kernels read, the schedule of the
// weight-gradient launch, the per-workspace state and every extern "C" entry point.  The kernels are reached through launchers:
//   rows kernels             train_rows1.hip (4 waves), train_rows2.hip (8 waves), train_rows3.hip     -- rows_common.hpp
//   weight gradients, apply  train_wgrad.hip                                                           -- wgrad_types.hpp
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <map>
#include <algorithm>
#include <tuple>
#include <math.h>
#include <stdlib.h>
#include "fused_tiles.hpp"
#include "rows_common.hpp"
#include "wgrad_types.hpp"
#include "../../include/dvae_train.h"

namespace dvae {
namespace fused {

// ---------------------------------------------------------------------------------------------
// host-side planning
struct Layout {
    // weight-copy buffer (elements of T)
    int64_t W1s, W2s, Wmvs, W3s, W4s, W5s, W5t, W4t, W3zt, Wmvt, W2t, wcopy_elems;
    int64_t Wc1s, Wc2s, Wc2t, Wa1s, Wa1t, Wa2s, Wa2t;                  // M2_info
    int64_t c1T, c2T, dc1T, dc2T, dc3T, a1T, a2T, da1T, da2T, da3T;     // M2_info stash
    bool info;
    int ld1, ld3, yp, ye, yd;
    // stash (rows of Bp elements)
    int64_t xT, yT, h1T, h2T, dh1T, dh2T, dmlvT, zT, d1T, d2T, dd1T, dd2T, daT, stash_rows;
    // workspace byte offsets
    int64_t o_tiles, o_blocks, o_blocks4, o_items4, o_tensors, o_chunks, o_partials, o_flags, o_defer, o_wcopy, o_stash, o_grads, total;
    int ntiles, nblocks, nblocks4;
};
// deferred optimizer step (apply_common.hpp): task table, then the arrival counters (DEFER_SHARDS lines of 128 bytes), then one line with
// the `done` counter (word 0) and the error word (word 1)
constexpr int DEFER_MAX_TASKS = 640;
constexpr int64_t DEFER_O_SHARD = (int64_t)DEFER_MAX_TASKS * (int64_t)sizeof(DeferTask);
constexpr int64_t DEFER_O_DONE = DEFER_O_SHARD + DEFER_SHARDS * 128;
constexpr int64_t DEFER_BYTES = DEFER_O_DONE + 128;

static inline int64_t al(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

static inline int planes_of(int precision) { return precision == DVAE_PREC_BF16X3 ? 2 : 1; }

static int make_layout(const dvae_train_plan_t& p, Layout& L) {
    const int esz = is_bf(p.precision) ? 2 : 4;
    const int np = planes_of(p.precision);
    L.yp = p.y_dim == 0 ? 0 : (p.y_dim + 15) / 16 * 16;
    L.ye = p.model == DVAE_MODEL_M2 ? L.yp : 0;
    L.info = p.model == DVAE_MODEL_M2_INFO;
    L.yd = L.yp;
    // K extents of the weight copies: 16-deep k-steps (x 513 -> 528, labels -> multiple of 16, z 16), or -- rows3 kernel, 32-deep
    // k-steps on 16 x 16 x 32 MFMA tiles -- x -> 544, labels -> multiple of 32, z -> 32
    const bool r3 = p.rows_kernel == 3;
    const int yk = p.y_dim == 0 ? 0 : (r3 ? (p.y_dim + 31) / 32 * 32 : L.yp);
    L.ld1 = (r3 ? 544 : XP) + (L.ye ? yk : 0);
    L.ld3 = (r3 ? 32 : ZD) + (L.yd ? yk : 0);
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += al(n, 128); return r; };
    L.W1s = take((int64_t)HD * L.ld1); L.W2s = take(HD * HD); L.Wmvs = take(32 * HD); L.W3s = take((int64_t)HD * L.ld3);
    L.W4s = take(HD * HD); L.W5s = take((int64_t)NO * HD); L.W5t = take((int64_t)HD * NO); L.W4t = take(HD * HD);
    L.W3zt = take(32 * HD); L.Wmvt = take(HD * 32); L.W2t = take(HD * HD);
    if (L.info) {
        L.Wc1s = take((int64_t)HD * XP); L.Wc2s = take(HD * HD); L.Wc2t = take(HD * HD);
        L.Wa1s = take(HD * ZD); L.Wa1t = take(32 * HD); L.Wa2s = take(HD * HD); L.Wa2t = take(HD * HD);
    }
    L.wcopy_elems = o;
    int64_t r = 0;
    auto rows = [&](int64_t n) { int64_t q = r; r += n; return q; };
    L.xT = rows(NO); L.yT = rows(L.yp ? al(L.yp, 32) : 0); L.h1T = rows(HD); L.h2T = rows(HD); L.dh1T = rows(HD); L.dh2T = rows(HD);
    L.dmlvT = rows(32); L.zT = rows(32); L.d1T = rows(HD); L.d2T = rows(HD); L.dd1T = rows(HD); L.dd2T = rows(HD); L.daT = rows(NO);
    if (L.info) {
        L.c1T = rows(HD); L.c2T = rows(HD); L.dc1T = rows(HD); L.dc2T = rows(HD); L.dc3T = rows(32);
        L.a1T = rows(HD); L.a2T = rows(HD); L.da1T = rows(HD); L.da2T = rows(HD); L.da3T = rows(32);
    }
    rows(32);   // slack
    L.stash_rows = r;
    // 2x2 groups of 32x32 tiles per job: (pairs of A blocks) x (pairs of B blocks)
    const int nty = L.yp ? (int)(al(L.yp, 32) / 32) : 0;
    auto pr = [](int n) { return (n + 1) / 2; };
    L.ntiles = 2 * pr(NT_OUT + (L.ye ? nty : 0)) + 2 * 2 + 1 * 2 + 2 * pr(1 + (L.yd ? nty : 0)) + 2 * 2 + pr(NT_OUT) * 2;
    if (L.info) L.ntiles += 2 * pr(NT_OUT) + 2 * 2 + 1 * 2 + 2 * 1 + 2 * 2 + 1 * 2;   // clf L1, L2, out; aux L1, L2, out
    // 4 x 4 blocks of the workgroup-blocked kernel: ceil(A tiles / 4) x ceil(B tiles / 4) per layer
    auto q4 = [](int n) { return (n + 3) / 4; };
    L.nblocks = q4(4) * q4(NT_OUT + (L.ye ? nty : 0)) + 1 + 1 + q4(4) * q4(1 + (L.yd ? nty : 0)) + 1 + q4(NT_OUT) * 1;
    if (L.info) L.nblocks += q4(NT_OUT) + 1 + 1 + 1 + 1 + 1;
    // blocks of the workgroup k-split kernel: as above, but a block never mixes input-matrix tiles (x, labels) with stash tiles
    L.nblocks4 = q4(4) * (q4(NT_OUT) + (L.ye ? q4(nty) : 0)) + 1 + 1 + q4(4) * (1 + (L.yd ? q4(nty) : 0)) + 1 + q4(NT_OUT) * 1;
    if (L.info) L.nblocks4 += q4(NT_OUT) + 1 + 1 + 1 + 1 + 1;
    int64_t b = 0;
    auto bytes = [&](int64_t n) { int64_t q = b; b += al(n, 256); return q; };
    L.o_tiles = bytes((int64_t)L.ntiles * sizeof(GroupDesc));
    L.o_blocks = bytes((int64_t)L.nblocks * sizeof(BlockDesc));
    L.o_blocks4 = bytes((int64_t)L.nblocks4 * sizeof(Block4));
    L.o_items4 = bytes((int64_t)3 * W4_MAX_ITEMS * sizeof(W4Item));      // table of the one launch, then the two tables of a grouped plan
    L.o_tensors = bytes(DVAE_TRAIN_MAX_TENSORS * sizeof(TensorDesc));
    L.o_chunks = bytes(p.n_params / 64 + 64);
    L.o_partials = bytes(p.rows_grid * 4 * sizeof(double));
    L.o_flags = bytes(1024 + 4 * (p.Bp / TB + 1));            // header of 256 words -- [0]: label-lo-plane epoch (RowsArgs::ylo_epoch), [1], [2], [16..]: the counters of the
                                                              // folded optimizer tail (fold_tail) -- then from byte 1024: ylo_dirty[tile]
    L.o_defer = bytes(DEFER_BYTES);
    L.o_wcopy = bytes(L.wcopy_elems * esz * np);              // PolX3: hi plane, then lo plane
    L.o_stash = bytes(L.stash_rows * p.Bp * esz * np);
    L.o_grads = bytes((int64_t)p.ksplit * p.n_params * sizeof(float));
    L.total = b;
    return 0;
}

static bool g_prof = false;
static unsigned long long* g_dbg = nullptr;   // set by dvae_train_debug_stamps
static double g_ms[4] = {0, 0, 0, 0};
static int64_t g_calls[4] = {0, 0, 0, 0};
struct PendingEv { hipEvent_t a, b; int which; };
static PendingEv g_pending[4096];
static int g_npending = 0;

struct ProfScope {
    hipStream_t s; int which; hipEvent_t a, b; bool on;
    __attribute__((noinline)) ProfScope(hipStream_t s_, int w) : s(s_), which(w), on(g_prof && g_npending < 4096) {      // (one copy, not one per launch site)
        if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
    }
    ~ProfScope() {
        if (on) { (void)hipEventRecord(b, s); g_pending[g_npending++] = PendingEv{a, b, which}; }
    }
};

}  // namespace fused
}  // namespace dvae

using namespace dvae;
using namespace dvae::fused;

static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static long long env_ll(const char* name, long long dflt) { const char* v = getenv(name); return v ? atoll(v) : dflt; }
// weight-gradient kernel form: 4 = workgroup k-split 4 x 4 blocks (default), 2 = 2 x 2 register ring (DVAE_WGRAD=ring),
// 1 = LDS-staged 4 x 4 blocks (DVAE_WGRAD=lds; bf16 policies only).  *set: the variable is there at all
static int wgrad_form_env(bool* set = nullptr) {
    const char* wk = getenv("DVAE_WGRAD");
    if (set) *set = wk != nullptr;
    if (wk && strcmp(wk, "ring") == 0) return 2;
    if (wk && strcmp(wk, "lds") == 0) return 1;
    return 4;
}

static void w4_plan_classes(dvae_train_plan_t* plan, bool grouped);      // (defined behind fill_tables)
constexpr int W4_GROUPED = 0x40000000;      // plan->reserved0: two launches (decoder-side blocks, encoder-side blocks), see w4_build_items

extern "C" int dvae_train_plan(int model, int y_dim, int precision, int64_t B, int ksplit_hint, dvae_train_plan_t* plan) {
    DVAE_CHECK_ARG(plan != nullptr && B > 0, "train_plan: bad argument");
    if (!((model == DVAE_MODEL_M1 && y_dim == 0) || (model == DVAE_MODEL_M2 && (y_dim == 1 || y_dim == 513)) ||
          (model == DVAE_MODEL_M2_INFO && y_dim == 1) || (model == DVAE_MODEL_M2_DEC && y_dim == 1))) {
        set_error("train_plan: fused kernels cover M1 (y 0), M2 (y 1 or 513), M2_info and M2_DEC (y 1) at x 513 / h [128,128] / z 16; got model %d y_dim %d", model, y_dim);
        return DVAE_E_UNSUPPORTED;
    }
    DVAE_CHECK_ARG(precision == DVAE_PREC_F32 || precision == DVAE_PREC_BF16 || precision == DVAE_PREC_BF16X3, "train_plan: unknown precision %d", precision);
    memset(plan, 0, sizeof(*plan));
    plan->model = model; plan->y_dim = y_dim; plan->precision = precision; plan->B = B;
    plan->Bp = al(B, 128);
    const int ye = model == DVAE_MODEL_M2 ? y_dim : 0, yd = y_dim;
    const int rows[26] = {HD, HD, HD, HD, ZD, ZD, ZD, ZD, HD, HD, HD, HD, XD, XD,
                          HD, HD, HD, HD, 1, 1, HD, HD, HD, HD, 1, 1};
    const int cols[26] = {XD + ye, 1, HD, 1, HD, 1, HD, 1, ZD + yd, 1, HD, 1, HD, 1,
                          XD, 1, HD, 1, HD, 1, ZD, 1, HD, 1, HD, 1};
    int64_t off = 0;
    plan->n_tensors = model == DVAE_MODEL_M2_INFO ? 26 : 14;
    for (int i = 0; i < plan->n_tensors; ++i) {
        plan->tensor_offset[i] = off; plan->tensor_rows[i] = rows[i]; plan->tensor_cols[i] = cols[i];
        off += al((int64_t)rows[i] * cols[i], 64);
    }
    plan->n_params = off;
    const int64_t ntiles = (B + TB - 1) / TB;
    // rows kernel generation: the 8-wave chain + helper kernel wherever it exists (M1 / M2 with bf16 or bf16x3 operands: 48 vs 55 us
    // per 8192 frames under bf16x3, 31 vs 33 us under bf16); DVAE_ROWS=1 forces the 4-wave kernel
    int want = env_int("DVAE_ROWS", 2);
    if (want < 1 || want > 3) want = 2;
    plan->rows_kernel = (want == 3 && rows3_supported(precision, model)) ? 3 : ((want >= 2 && rows2_supported(precision, model)) ? 2 : 1);
    if (!kDiagBuild && plan->rows_kernel == 1 && is_bf(precision)) {
        set_error("train_plan: DVAE_ROWS=1 (the 4-wave rows kernel) under the bf16 policies needs the diagnostic build (build.py --diag)");
        return DVAE_E_UNSUPPORTED;
    }
    if (model == DVAE_MODEL_M2_DEC && plan->rows_kernel != 2) {
        set_error("train_plan: M2_DEC exists in the 8-wave rows kernel only (bf16 / bf16x3 operands, DVAE_ROWS unset)");
        return DVAE_E_UNSUPPORTED;
    }
    // workgroups resident at once: the 8-wave kernel holds one per CU; the 4-wave bf16 kernel two.  Beyond that: persistent tile loop
    const int64_t maxg = plan->rows_kernel >= 2 ? 256 : 256 * (precision == DVAE_PREC_BF16 ? 2 : 1);
    plan->rows_grid = ntiles < maxg ? ntiles : maxg;
    int ks = ksplit_hint;
    const bool wg4 = wgrad_form_env() == 4;
    // bf16: 8 slices up to 8192 frames (more slices = more slabs for the apply pass to sum); 12 beyond: 80 groups x 12 = 960
    // single-wave jobs fill the 1024 wave slots in one round (wgrad 164 -> 124 us at 65 536 frames, 2.49 -> 1.80 ms at 2^20).
    // fp32: the MFMA-bound wgrad needs a wave on every SIMD (>= 1024 wave jobs): 16.
    if (ks <= 0 && wg4) {
        // workgroup k-split kernel: one workgroup per (4 x 4 tile block, frame slice) and per CU: as many slices as fill the 256 CUs
        // in one round (M2 y513: 22 blocks x 11), at least 128 frames (two k-steps per wave) each, at most 16 (the apply pass sums them)
        dvae_train_plan_t tmp = *plan;
        tmp.ksplit = 1;
        Layout L0;
        make_layout(tmp, L0);
        ks = 256 / L0.nblocks4;
        // as many slices as fill the CUs; the kernel's XCD-aware index map keeps 8 * (ks / 8) of them on one XCD each (the bf16 policies
        // are bound by the cold read of the stash) and deals the rest out block-wise
        if (ks > plan->Bp / 128) ks = (int)(plan->Bp / 128);
        if (ks > 16) ks = 16;
        if (ks < 1) ks = 1;
    }
    if (ks <= 0) {
        // bf16x3: a wave issues 16 MFMAs per k-step (3 per tile product), ~15.6 us of matrix time per 1024-frame slice on its own SIMD, and
        // 80 groups x 8 slices fill only 640 of the 1024 SIMDs: 12 slices (960 waves) take 3.3 us off the kernel and add 1.7 us of slab sums
        const int cap = precision == DVAE_PREC_BF16X3 ? 12 : (is_bf(precision) ? (plan->Bp > 12288 ? 12 : 8) : 16);
        ks = (int)(plan->Bp / (precision == DVAE_PREC_BF16X3 ? 640 : (is_bf(precision) ? 1024 : 512))); if (ks < 1) ks = 1; if (ks > cap) ks = cap;
    }
    if (ks > 64) ks = 64;
    plan->ksplit = ks;
    plan->reserved0 = 0;
    // Class-sliced schedule of the weight-gradient launch (round 5; w4_class_slices): every block is cut into as many frame slices as ITS
    // cost per k-step asks for, instead of one slice count for all.  Chosen when the library picks the slicing (no hint), for the workgroup
    // k-split kernel; the diagnostic variants whose protocols count `ksplit` arrivals per block (folded / deferred optimizer step) and
    // DVAE_W4_UNIFORM=1 keep the uniform table.  plan->reserved0 = workgroups of that launch (0: uniform slices), ksplit = slabs to sum.
    // Measured (tools/r05/w4_classes_ab.sh, w4_ab2.sh; M2 y 513, 8192 frames, same box, alternating): fp32 operands 60.3 -> 53.2 us (the launch is
    // bound by its matrix work: the model's quantity); bf16x3 25.3 -> 26.6 us and bf16 18.0 -> 19.8 us -- those launches are bound by the
    // 85 MB they pull from the stash (4.3 TB/s), not by the heaviest blocks' MFMAs, and more slices only add slab stores.  So: class-sliced
    // under the fp32 policy, uniform under the bf16 policies (DVAE_W4_CLASSES=1 forces it there, DVAE_W4_UNIFORM=1 switches it off).
    const bool want_classes = getenv("DVAE_W4_CLASSES") != nullptr ? atoi(getenv("DVAE_W4_CLASSES")) != 0 : !is_bf(precision);
    // DVAE_EXCHANGE_GROUPS=2 (opt-in, multi-GPU; read when the plan is made): the weight-gradient pass as TWO launches -- the blocks of the
    // decoder-side tensors (and M2_info's side nets), then those of the encoder -- each cut to fill the CUs by itself, so that the exchange
    // of the first group's gradient can run while the second launch computes (dvae_train_grads_group; Trainer, dp.py).  Always class-sliced.
    const bool want_groups = getenv("DVAE_EXCHANGE_GROUPS") != nullptr && atoi(getenv("DVAE_EXCHANGE_GROUPS")) == 2;
    if ((want_classes || want_groups) && ksplit_hint <= 0 && wg4 && plan->Bp > 128 && getenv("DVAE_W4_UNIFORM") == nullptr &&
        getenv("DVAE_FOLD_APPLY") == nullptr && getenv("DVAE_DEFER_APPLY") == nullptr)
        w4_plan_classes(plan, want_groups);
    Layout L;
    make_layout(*plan, L);
    plan->workspace_bytes = L.total;
    plan->grad_offset_bytes = L.o_grads;
    const double mac = (double)HD * (XD + ye) + HD * HD + 2.0 * ZD * HD + (double)HD * (ZD + yd) + HD * HD + (double)XD * HD;
    const double dxm = (double)HD * HD + 2.0 * ZD * HD + (double)ZD * HD + HD * HD + (double)XD * HD;
    double macx = 0.0, dxx = 0.0;
    if (model == DVAE_MODEL_M2_INFO) {   // classifier fwd once; auxiliary fwd twice in the reference (z and z.detach())
        macx = ((double)HD * XD + HD * HD + HD) + 2.0 * ((double)HD * ZD + HD * HD + HD);
        dxx = ((double)HD * HD + HD) + ((double)HD * HD + HD + (double)ZD * HD);
    }
    plan->flops_per_step = 2.0 * (2.0 * mac + dxm) * (double)B + 2.0 * (2.0 * macx + dxx) * (double)B;
    plan->info_alpha = 0.0; plan->info_beta = 10.0; plan->info_gamma = 1.0;
    plan->min_hbm_bytes_per_step = 4.0 * (XD + y_dim + ZD) * (double)B;
    return 0;
}

static int64_t kper_of(const dvae_train_plan_t* p) {
    const int ks = is_bf(p->precision) ? 16 : 8;
    const int64_t unit = 4 * ks;
    return al((p->Bp + p->ksplit - 1) / p->ksplit, unit);
}

struct ABlock { int64_t row; int mvalid; int tensor; int m0; int bias_tensor; int tensor_hi; int bias_hi; };
struct BBlock { int64_t row; int nvalid; int col; int kind; int scol; int sncols; };   // kind 1 / 2: columns scol.. of the input matrix x / y (sncols wide)

template <typename T>
static void fill_tables(const dvae_train_plan_t* p, const Layout& L, char* ws_dev, GroupDesc* groups, BlockDesc* blocks, Block4* blocks4, TensorDesc* td) {
    const int64_t Bp = p->Bp;
    T* stash = (T*)(ws_dev + L.o_stash);
    auto S = [&](int64_t row) { return (const void*)(stash + row * Bp); };
    int n = 0;
    ABlock ab[64];
    BBlock bb[64];
    int na = 0, nb = 0;
    auto addA = [&](int64_t row0, int M, int tensor, int bias_tensor) {
        for (int m0 = 0; m0 < M; m0 += 32) ab[na++] = ABlock{row0 + m0, M - m0 < 32 ? M - m0 : 32, tensor, m0, bias_tensor, -1, -1};
    };
    auto addB = [&](int64_t row0, int N, int col0, int kind = 0) {
        for (int n0 = 0; n0 < N; n0 += 32) bb[nb++] = BBlock{row0 + n0, N - n0 < 32 ? N - n0 : 32, col0 + n0, kind, n0, N};
    };
    int nblk = 0, nblk4 = 0, layer_id = 0;
    // 2 x 2 group of tiles: A pair starting at block i, B pair starting at block j (all-null when out of range)
    auto make_group = [&](int i, int j) {
        GroupDesc d;
        memset(&d, 0, sizeof(d));
        d.bias_off[0] = d.bias_off[1] = -1;
        if (i >= na || j >= nb) return d;
        for (int ii = 0; ii < 2; ++ii) {
            if (i + ii >= na) continue;
            const ABlock& a = ab[i + ii];
            d.A[ii] = S(a.row);
            d.ldo[ii] = p->tensor_cols[a.tensor];
            d.mvalid[ii] = a.mvalid;
            if (a.bias_tensor >= 0 && j == 0) d.bias_off[ii] = p->tensor_offset[a.bias_tensor] + a.m0;
            for (int jj = 0; jj < 2; ++jj) {
                if (j + jj >= nb) continue;
                d.out_off[ii][jj] = p->tensor_offset[a.tensor] + (int64_t)a.m0 * d.ldo[ii] + bb[j + jj].col;
                if (ii == 0 && a.tensor_hi >= 0) d.out_off_hi[jj] = p->tensor_offset[a.tensor_hi] + bb[j + jj].col;
            }
            if (ii == 0 && a.tensor_hi >= 0) {
                d.split16 = 1;
                d.ldo_hi = p->tensor_cols[a.tensor_hi];
                d.bias_off_hi = p->tensor_offset[a.bias_hi];
            }
        }
        for (int jj = 0; jj < 2; ++jj) {
            if (j + jj >= nb) continue;
            d.Bm[jj] = S(bb[j + jj].row);
            d.nvalid[jj] = bb[j + jj].nvalid;
        }
        return d;
    };
    auto emit = [&]() {
        for (int i = 0; i < na; i += 2)
            for (int j = 0; j < nb; j += 2) groups[n++] = make_group(i, j);
        for (int i0 = 0; i0 < na; i0 += 4)
            for (int j0 = 0; j0 < nb; j0 += 4) {
                BlockDesc b;
                memset(&b, 0, sizeof(b));
                for (int k = 0; k < 4; ++k) {
                    b.At[k] = i0 + k < na ? S(ab[i0 + k].row) : nullptr;
                    b.Bt[k] = j0 + k < nb ? S(bb[j0 + k].row) : nullptr;
                }
                for (int wr = 0; wr < 2; ++wr)
                    for (int wc = 0; wc < 2; ++wc) b.g[wr * 2 + wc] = make_group(i0 + 2 * wr, j0 + 2 * wc);
                blocks[nblk++] = b;
            }
        // blocks of the workgroup k-split kernel: per run of B tiles of one kind (stash / x / labels)
        for (int r0 = 0; r0 < nb;) {
            int r1 = r0;
            while (r1 < nb && bb[r1].kind == bb[r0].kind) ++r1;
            for (int i0 = 0; i0 < na; i0 += 4)
                for (int j0 = r0; j0 < r1; j0 += 4) {
                    Block4 q;
                    memset(&q, 0, sizeof(q));
                    q.layer = layer_id;
                    q.raw = bb[r0].kind; q.rncols = bb[r0].sncols;
                    for (int k = 0; k < 4; ++k) {
                        q.bias_off[k] = -1;
                        if (i0 + k < na) {
                            const ABlock& a = ab[i0 + k];
                            q.At[k] = S(a.row);
                            q.ldo[k] = p->tensor_cols[a.tensor];
                            q.a_off[k] = p->tensor_offset[a.tensor] + (int64_t)a.m0 * q.ldo[k];
                            q.mvalid[k] = a.mvalid;
                            q.wt[k] = a.tensor; q.bt[k] = a.bias_tensor >= 0 ? a.bias_tensor : 0;
                            if (a.bias_tensor >= 0 && j0 == 0) q.bias_off[k] = p->tensor_offset[a.bias_tensor] + a.m0;
                            if (k == 0 && a.tensor_hi >= 0) {
                                q.wt_hi = a.tensor_hi; q.bt_hi = a.bias_hi;
                                q.split16 = 1;
                                q.ldo_hi = p->tensor_cols[a.tensor_hi];
                                q.a_off_hi = p->tensor_offset[a.tensor_hi];
                                q.bias_off_hi = p->tensor_offset[a.bias_hi];
                            }
                        }
                        if (j0 + k < r1) {
                            q.Bt[k] = S(bb[j0 + k].row);
                            q.bcol[k] = bb[j0 + k].col;
                            q.nvalid[k] = bb[j0 + k].nvalid;
                            q.rcol[k] = bb[j0 + k].scol;
                        }
                    }
                    blocks4[nblk4++] = q;
                }
            r0 = r1;
        }
        na = 0; nb = 0;
        ++layer_id;
    };
    const int ye = p->model == DVAE_MODEL_M2 ? p->y_dim : 0, yd = p->y_dim;
    addA(L.dh1T, HD, 0, 1); addB(L.xT, XD, 0, 1); if (ye) addB(L.yT, ye, XD, 2); emit();
    addA(L.dh2T, HD, 2, 3); addB(L.h1T, HD, 0); emit();
    ab[na++] = ABlock{L.dmlvT, 32, 4, 0, 5, 6, 7}; addB(L.h2T, HD, 0); emit();   // one tile: rows 0-15 mu head, 16-31 log_var head
    addA(L.dd1T, HD, 8, 9); addB(L.zT, ZD, 0); if (yd) addB(L.yT, yd, ZD, 2); emit();
    addA(L.dd2T, HD, 10, 11); addB(L.d1T, HD, 0); emit();
    addA(L.daT, XD, 12, 13); addB(L.d2T, HD, 0); emit();
    if (L.info) {   // classifier (tensors 14-19) and auxiliary net (20-25): scripts/training_M2_info_vad.py:141-143
        addA(L.dc1T, HD, 14, 15); addB(L.xT, XD, 0, 1); emit();
        addA(L.dc2T, HD, 16, 17); addB(L.c1T, HD, 0); emit();
        addA(L.dc3T, 1, 18, 19); addB(L.c2T, HD, 0); emit();
        addA(L.da1T, HD, 20, 21); addB(L.zT, ZD, 0); emit();
        addA(L.da2T, HD, 22, 23); addB(L.a1T, HD, 0); emit();
        addA(L.da3T, 1, 24, 25); addB(L.a2T, HD, 0); emit();
    }
    if (n != L.ntiles || nblk != L.nblocks || nblk4 != L.nblocks4) { fprintf(stderr, "dvae: internal group / block count mismatch %d vs %d, %d vs %d, %d vs %d\n", n, L.ntiles, nblk, L.nblocks, nblk4, L.nblocks4); }
    // tensors -> kernel-layout copies
    for (int i = 0; i < p->n_tensors; ++i) {
        TensorDesc t;
        memset(&t, 0, sizeof(t));
        t.off = p->tensor_offset[i]; t.rows = p->tensor_rows[i]; t.cols = p->tensor_cols[i];
        t.sf_off = -1; t.st_off = -1; t.sf_split = 1 << 30;
        td[i] = t;
    }
    td[0].sf_ld = L.ld1; td[2].sf_ld = HD; td[4].sf_ld = HD; td[6].sf_ld = HD; td[8].sf_ld = L.ld3; td[10].sf_ld = HD; td[12].sf_ld = HD;
    td[2].st_ld = HD; td[4].st_ld = 32; td[6].st_ld = 32; td[8].st_ld = HD; td[10].st_ld = HD; td[12].st_ld = NO;
    td[0].sf_off = L.W1s; td[0].sf_nt = 4; td[0].sf_split = XD; td[0].sf_gap = XP - XD;
    // the 8-wave rows kernel under the split-bf16 policy multiplies the x block of layer 1 (and of the M2_info classifier) in split fp16
    const int f16c = (p->precision == DVAE_PREC_BF16X3 && p->rows_kernel >= 2 && PolX3v2::XF16) ? XD : 0;
    td[0].sf_f16_cols = f16c;
    td[2].sf_off = L.W2s; td[2].sf_nt = 4; td[2].st_off = L.W2t; td[2].st_nt = 4; td[2].st_cmax = HD;
    td[4].sf_off = L.Wmvs; td[4].sf_nt = 1; td[4].st_off = L.Wmvt; td[4].st_nt = 4; td[4].st_cmax = HD;
    td[6].sf_off = L.Wmvs; td[6].sf_nt = 1; td[6].sf_roff = 16; td[6].st_off = L.Wmvt; td[6].st_nt = 4; td[6].st_roff = 16; td[6].st_cmax = HD;
    td[8].sf_off = L.W3s; td[8].sf_nt = 4; td[8].st_off = L.W3zt; td[8].st_nt = 1; td[8].st_cmax = ZD;
    td[10].sf_off = L.W4s; td[10].sf_nt = 4; td[10].st_off = L.W4t; td[10].st_nt = 4; td[10].st_cmax = HD;
    td[12].sf_off = L.W5s; td[12].sf_nt = NT_OUT; td[12].st_off = L.W5t; td[12].st_nt = 4; td[12].st_cmax = HD;
    if (p->rows_kernel == 3) {
        // rows3 kernel: 16-row tiles / 32-deep k-steps (apply_types.hpp: kind16); the heads' rows interleaved (rowmap), the backward-z
        // matrix's rows likewise (trowmap)
        for (int i = 0; i < 14; ++i) td[i].kind16 = 1;
        td[0].sf_nt = 8; td[0].sf_gap = 544 - XD;
        td[2].sf_nt = 8; td[2].st_nt = 8;
        td[4].sf_nt = 2; td[4].rowmap = 1; td[4].st_nt = 8;
        td[6].sf_nt = 2; td[6].rowmap = 2; td[6].sf_roff = 0; td[6].st_nt = 8;
        td[8].sf_nt = 8; td[8].sf_split = ZD; td[8].sf_gap = 32 - ZD; td[8].st_nt = 2; td[8].trowmap = 1;
        td[10].sf_nt = 8; td[10].st_nt = 8;
        td[12].sf_nt = NO / 16; td[12].st_nt = 8;
    }
    if (L.info) {
        td[14].sf_off = L.Wc1s; td[14].sf_nt = 4; td[14].sf_ld = XP; td[14].sf_split = XD; td[14].sf_gap = XP - XD; td[14].sf_f16_cols = f16c;
        td[16].sf_off = L.Wc2s; td[16].sf_nt = 4; td[16].sf_ld = HD; td[16].st_off = L.Wc2t; td[16].st_nt = 4; td[16].st_ld = HD; td[16].st_cmax = HD;
        td[20].sf_off = L.Wa1s; td[20].sf_nt = 4; td[20].sf_ld = ZD; td[20].st_off = L.Wa1t; td[20].st_nt = 1; td[20].st_ld = HD; td[20].st_cmax = ZD;
        td[22].sf_off = L.Wa2s; td[22].sf_nt = 4; td[22].sf_ld = HD; td[22].st_off = L.Wa2t; td[22].st_nt = 4; td[22].st_ld = HD; td[22].st_cmax = HD;
    }
}

// folded launches per workspace (the block counters of fold_tail count arrivals across launches); dvae_train_init zeroes the
// workspace and forgets its count
static std::mutex g_fold_mu;
static std::unordered_map<const void*, unsigned> g_fold_seq;
// workgroups of the weight-gradient launch of a workspace (the size of its item table, fixed by dvae_train_init)
struct W4Grids { int g[3]; };      // table 0 (the one launch of an ungrouped plan), tables 1 / 2 (group 0 / 1 of a grouped plan)
static std::unordered_map<const void*, W4Grids> g_w4_grid;
static void w4_grid_put(const void* ws, const W4Grids& grids) { std::lock_guard<std::mutex> lk(g_fold_mu); g_w4_grid[ws] = grids; }
static int w4_grid_get(const void* ws, int table) { std::lock_guard<std::mutex> lk(g_fold_mu); auto it = g_w4_grid.find(ws); return it == g_w4_grid.end() ? -1 : it->second.g[table]; }
static unsigned fold_seq_next(const void* ws) { std::lock_guard<std::mutex> lk(g_fold_mu); return ++g_fold_seq[ws]; }
static void fold_seq_reset(const void* ws) { std::lock_guard<std::mutex> lk(g_fold_mu); g_fold_seq.erase(ws); }

// ---- deferred optimizer step: host-side state per workspace
struct PendingUpdate { float* params; float* m; float* v; int step; double lr, beta1, beta2, adam_eps; int n_slabs; };
struct DeferState { bool pending = false; PendingUpdate u{}; unsigned seq_arrive = 0, seq_done = 0; int ntasks = 0; };
static std::mutex g_defer_mu;
static std::unordered_map<const void*, DeferState> g_defer_state;
static DeferState defer_state_get(const void* ws) { std::lock_guard<std::mutex> lk(g_defer_mu); return g_defer_state[ws]; }
static void defer_state_put(const void* ws, const DeferState& st) { std::lock_guard<std::mutex> lk(g_defer_mu); g_defer_state[ws] = st; }
static void defer_state_reset(const void* ws) { std::lock_guard<std::mutex> lk(g_defer_mu); g_defer_state.erase(ws); }
// dvae_train_step_deferred -> run_grads: run the rows kernel in its deferred form
struct DeferRequest { bool on = false, have = false; PendingUpdate u{}; unsigned seq_arrive = 0, seq_done = 0; float* losses3 = nullptr; };

// tasks of the deferred update (apply_common.hpp: DeferTask): 32 x 32 tiles of every tensor with kernel-layout copies, per column block
// (a tile never straddles the split of the forward copy), and 1024-element chunks of the tensors without copies
static int build_defer_tasks(const dvae_train_plan_t* p, const TensorDesc* td, DeferTask* out, int cap) {
    int n = 0;
    auto put = [&](int t, int r0, int cbeg, int cend, int kind) { if (n < cap) out[n] = DeferTask{t, r0, cbeg, cend, kind, 0, 0, 0}; ++n; };
    for (int t = 0; t < p->n_tensors; ++t) {
        const int rows = p->tensor_rows[t], cols = p->tensor_cols[t];
        if (td[t].sf_off < 0 && td[t].st_off < 0) {
            for (int e0 = 0; e0 < rows * cols; e0 += 1024) put(t, 0, e0, rows * cols, 1);
            continue;
        }
        const int split = td[t].sf_off >= 0 && td[t].sf_split < cols ? td[t].sf_split : cols;
        for (int r0 = 0; r0 < rows; r0 += 32) {
            for (int cb = 0; cb < split; cb += 32) put(t, r0, cb, split, 0);
            for (int cb = split; cb < cols; cb += 32) put(t, r0, cb, cols, 0);
        }
    }
    return n;
}

static ApplyArgs make_apply_args(const dvae_train_plan_t* plan, const Layout& L, float* params, float* m, float* v, char* ws, int n_slabs,
                                 bool adam, int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale, float* losses3) {
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.p = params; a.m = m; a.v = v;
    a.slabs = (const float*)(ws + L.o_grads); a.slab_stride = plan->n_params; a.nslabs = n_slabs;
    a.tensors = (const TensorDesc*)(ws + L.o_tensors); a.ntensors = plan->n_tensors;
    a.chunk_tensor = (const unsigned char*)(ws + L.o_chunks); a.n_params = plan->n_params;
    a.wcopy = ws + L.o_wcopy; a.wpl = L.wcopy_elems;
    if (adam) {
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        a.one_minus_b1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.one_minus_b2 = (float)(1.0 - beta2);
        a.step_size = (float)(lr / bc1); a.bc2_sqrt = (float)sqrt(bc2); a.eps = (float)adam_eps; a.gscale = (float)grad_scale;
    }
    a.partials = (const double*)(ws + L.o_partials); a.npartials = (int)plan->rows_grid; a.B = plan->B; a.losses3 = losses3; a.accum = (double*)(uintptr_t)plan->loss_accum;
    a.info = plan->model == DVAE_MODEL_M2_INFO; a.alpha = (float)plan->info_alpha; a.beta = (float)plan->info_beta; a.gamma = (float)plan->info_gamma;
    return a;
}

static int launch_apply(const dvae_train_plan_t* plan, const Layout& L, float* params, float* m, float* v, char* ws, int n_slabs,
                        bool adam, int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale,
                        float* losses3, hipStream_t s) {
    const ApplyArgs a = make_apply_args(plan, L, params, m, v, ws, n_slabs, adam, step, lr, beta1, beta2, adam_eps, grad_scale, losses3);
    // DVAE_APPLY=units (opt-in; bf16 copies, at most 12 slabs): the unit form of the deferred step as its own launch.  Measured (M2 y513,
    // 8192 frames, bf16x3, same box, alternating): 10.8 against 9.4 us gross for the one-thread-per-parameter kernel below -- a quarter of the
    // instructions and no lone 2-byte stores, but 324 workgroups instead of 1183 on a launch that is one load round trip, one store round
    // trip and its own start-up either way: the flat kernel stays the default.
    const int ntasks = defer_state_get(ws).ntasks;
    const char* ak = getenv("DVAE_APPLY");
#ifdef DVAE_DIAG
    if (adam && is_bf(plan->precision) && n_slabs <= 12 && ntasks > 0 && ntasks <= DEFER_MAX_TASKS && ak && strcmp(ak, "units") == 0)
        return launch_apply_units(plan->precision, a, (const DeferTask*)(ws + L.o_defer), 4 * ntasks, s);
#else
    (void)ntasks; (void)ak;
#endif
    return launch_apply_kernel(plan->precision, adam, a, s);
}

// ---------------------------------------------------------------------------------------------
// Host-side schedule of wgrad4_kernel: the item table (one workgroup = one item) the kernel reads.
//
// Uniform (plan->reserved0 == 0): `ksplit` equal frame slices for every block, workgroup -> (slice, block) by the XCD-aware index map the
// kernel had until round 4 (slice s on XCD s % 8 for 8 * (ksplit / 8) "pure" slices, the rest dealt out block-wise).
//
// Class-sliced (round 5): the blocks of one launch differ by 4x in work per k-step -- 4 x 4 tiles at three MFMAs per product (48 per wave
// and k-step), label-fed 4 x 4 blocks at two (binary labels: one operand plane), 4 x 1 / 1 x 4 edge blocks (12, bound by their operand
// loads) -- and with one slice count for all, the launch lasted as long as its heaviest blocks while a quarter of the CUs had finished
// (M2 y 513, 8192 frames, 10 slices: 13 k-steps x 1536 clocks on the heavy blocks, 42 % of that on the light ones).  Here every block b gets
// s_b slices by water-filling on cost_b x k-steps: the block that would finish last is split further until the CUs are used up.  A block
// writes slabs 0 .. s_b - 1; the slabs it never writes hold the zeros dvae_train_init put there, so the optimizer launch (and the slab
// reduction of the multi-GPU path) keep summing plan->ksplit = max s_b slabs for every parameter, in slab order: still one deterministic sum.
struct W4Sched { std::vector<W4Item> items; int grid = 0; };

static void w4_host_blocks(const dvae_train_plan_t& p, const Layout& L, std::vector<Block4>& out) {
    std::vector<GroupDesc> tiles((size_t)L.ntiles + 8);
    std::vector<BlockDesc> blocks((size_t)L.nblocks + 8);
    out.assign((size_t)L.nblocks4 + 8, Block4{});
    TensorDesc td[DVAE_TRAIN_MAX_TENSORS];
    memset(td, 0, sizeof(td));
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);      // never dereferenced: the descriptors' pointers only say "present"
    if (is_bf(p.precision)) fill_tables<__bf16>(&p, L, base, tiles.data(), blocks.data(), out.data(), td);
    else fill_tables<float>(&p, L, base, tiles.data(), blocks.data(), out.data(), td);
    out.resize((size_t)L.nblocks4);
}

// cost of one 16-frame k-step of block b for one wave, in clocks (a model: matrix-pipe time against operand-fragment pulls at one 1 KB
// fragment per ~70 clocks and wave; the in-lane bias sums where the block carries bias rows)
static double w4_block_cost(const dvae_train_plan_t& p, const Block4& b) {
    int na = 0, nb = 0;
    bool bias = b.split16 && b.bias_off_hi >= 0;
    for (int k = 0; k < 4; ++k) { if (b.At[k]) na = k + 1; if (b.Bt[k]) nb = k + 1; bias = bias || b.bias_off[k] >= 0; }
    const bool x3 = p.precision == DVAE_PREC_BF16X3, bf = is_bf(p.precision);
    const bool one_plane_b = x3 && b.raw == 2 && p.rows_kernel >= 2;      // label tiles: binary labels need no lo plane (two MFMAs per product)
    double mfma, load, fsum;
    // clocks per 1 KB operand fragment and wave: 70 for a lone wave (tools/r03/kstep_bench.hip); W4_KB_CLOCKS overrides (experiments)
    static const double kb_clocks = getenv("DVAE_W4_KB_CLOCKS") ? atof(getenv("DVAE_W4_KB_CLOCKS")) : 70.0;
    if (bf) {
        mfma = (double)na * nb * (x3 ? (one_plane_b ? 2 : 3) : 1) * 32.0;
        load = ((double)na * (x3 ? 2 : 1) + (double)nb * (x3 ? (one_plane_b ? 1 : 2) : 1)) * kb_clocks;
        fsum = bias ? (double)na * (x3 ? 2 : 1) * 16 * 4 * 0.5 : 0.0;
    } else {
        mfma = (double)na * nb * 2 * 4 * 64.0;                            // two 8-frame k-steps of four 32 x 32 x 2 MFMAs per product
        load = (double)(na + nb) * 2 * 70.0;
        fsum = bias ? (double)na * 2 * 8 * 4 * 0.5 : 0.0;
    }
    if (b.raw != 0 && p.B >= 131072 && bf) load *= 2.0;                   // raw fp32 input tiles (large batches): twice the bytes, converted in the loop
    return std::max(mfma, load) + 0.3 * std::min(mfma, load) + fsum;
}

static int64_t w4_kper(const dvae_train_plan_t& p, int slices) {
    const int64_t unit = 4 * (is_bf(p.precision) ? 16 : 8);
    return al((p.Bp + slices - 1) / slices, unit);
}

// s[b] = slices of block b (>= 1), at most `max_items` in all, at most 16 per block (the optimizer launch sums that many slabs), at
// least 128 frames per slice
static inline bool w4_classed(const dvae_train_plan_t& p) { return (p.reserved0 & ~W4_GROUPED) > 0; }
static inline bool w4_grouped(const dvae_train_plan_t& p) { return (p.reserved0 & W4_GROUPED) != 0; }
// gradient slabs a step fills, for the optimizer launch to sum
static int used_slabs(const dvae_train_plan_t* plan) {
    if (w4_classed(*plan)) return plan->ksplit;                          // class-sliced schedule: the largest slice count of any block
    const int64_t kper = kper_of(plan);
    return (int)((plan->Bp + kper - 1) / kper);
}
// group of a block in the two-launch schedule: 0 = launched first (decoder layers 3-5 and, M2_info, the side nets 6-11: tensors 8 and up, the
// upper part of the flat gradient), 1 = the encoder (layers 0-2: tensors 0-7, the lower part)
static inline int w4_group_of(const Block4& b) { return b.layer <= 2 ? 1 : 0; }

// group < 0: every block; otherwise only the blocks of that group take part (the others keep s = 0)
static void w4_class_slices(const dvae_train_plan_t& p, const std::vector<Block4>& blocks, int max_items, std::vector<int>& s, int group = -1) {
    const int n = (int)blocks.size();
    s.assign(n, 1);
    std::vector<double> cost(n);
    for (int b = 0; b < n; ++b) cost[b] = (group < 0 || w4_group_of(blocks[b]) == group) ? w4_block_cost(p, blocks[b]) : 0.0;
    for (int b = 0; b < n; ++b) if (cost[b] == 0.0) s[b] = 0;
    int cap = (int)std::min<int64_t>(16, p.Bp / 128);
    if (cap < 1) cap = 1;
    int total = 0;
    for (int b = 0; b < n; ++b) total += s[b];
    for (;;) {
        int worst = -1;
        double tw = 0.0;
        for (int b = 0; b < n; ++b) { if (s[b] == 0) continue; const double t = cost[b] * (double)w4_kper(p, s[b]); if (t > tw) { tw = t; worst = b; } }
        if (worst < 0) break;
        int s2 = s[worst] + 1;
        while (s2 <= cap && w4_kper(p, s2) >= w4_kper(p, s[worst])) ++s2;       // the next slice count that shortens the slices
        if (s2 > cap || total + (s2 - s[worst]) > max_items) break;            // the block that finishes last cannot be split further
        total += s2 - s[worst];
        s[worst] = s2;
    }
}

static void w4_debug_print(const dvae_train_plan_t& p, const std::vector<Block4>& blocks, const std::vector<int>& s) {
    if (getenv("DVAE_W4_DEBUG") == nullptr) return;                        // DVAE_W4_DEBUG=1: the schedule, block by block (stderr)
    {
        for (int b = 0; b < (int)blocks.size(); ++b) {
            if (s[b] == 0) continue;
            int na = 0, nb = 0;
            for (int k = 0; k < 4; ++k) { if (blocks[b].At[k]) na = k + 1; if (blocks[b].Bt[k]) nb = k + 1; }
            const int64_t kper = w4_kper(p, s[b]);
            fprintf(stderr, "dvae w4: block %2d layer %d %d x %d kind %d bias %d cost %6.0f slices %2d of %lld frames -> %.0f clocks per wave\n", b, blocks[b].layer, na, nb,
                    blocks[b].raw, (int)(blocks[b].bias_off[0] >= 0), w4_block_cost(p, blocks[b]), (int)((p.Bp + kper - 1) / kper), (long long)kper,
                    w4_block_cost(p, blocks[b]) * (double)kper / 64.0);
        }
    }
}

static void w4_plan_classes(dvae_train_plan_t* plan, bool grouped) {
    dvae_train_plan_t tmp = *plan;
    tmp.ksplit = 1;
    Layout L0;
    make_layout(tmp, L0);
    std::vector<Block4> blocks;
    w4_host_blocks(tmp, L0, blocks);
    int nslabs = 1, items_max = 0;
    for (int grp = grouped ? 0 : -1; grp <= (grouped ? 1 : -1); ++grp) {
        std::vector<int> s;
        w4_class_slices(tmp, blocks, 256, s, grp);
        w4_debug_print(tmp, blocks, s);
        int items = 0;
        for (size_t b = 0; b < blocks.size(); ++b) {
            if (s[b] == 0) continue;
            const int64_t kper = w4_kper(tmp, s[b]);
            const int eff = (int)((tmp.Bp + kper - 1) / kper);
            nslabs = std::max(nslabs, eff);
            items += eff;
        }
        items_max = std::max(items_max, items);
    }
    plan->ksplit = nslabs;
    plan->reserved0 = items_max | (grouped ? W4_GROUPED : 0);
}

// group: -1 = the one launch of an ungrouped plan; 0 / 1 = the launches of a grouped plan (w4_group_of)
static void w4_build_items(const dvae_train_plan_t& p, const Layout& L, W4Sched& out, int group = -1) {
    out.items.clear();
    out.grid = 0;
    if (!w4_classed(p)) {
        // uniform slices, the round-2 index map
        const int64_t kper = w4_kper(p, p.ksplit);
        const int ks = (int)((p.Bp + kper - 1) / kper), nblocks = L.nblocks4;
        const int a8 = ks >> 3, r8 = ks & 7, npure = a8 * nblocks, per = (r8 * nblocks + 7) >> 3;
        out.grid = 8 * (a8 * nblocks + per);
        for (int w = 0; w < out.grid; ++w) {
            const int xcd = w & 7, j = w >> 3;
            W4Item it{-1, 0, 0, 0};
            if (j < npure) { it.slice = xcd + 8 * (j / nblocks); it.block = j % nblocks; }
            else {
                const int e = xcd * per + (j - npure);
                if (j - npure < per && e < r8 * nblocks) { it.slice = 8 * a8 + e / nblocks; it.block = e % nblocks; }
            }
            if (it.block >= 0) { it.kbeg = (int64_t)it.slice * kper; it.kend = std::min<int64_t>(it.kbeg + kper, p.Bp); }
            out.items.push_back(it);
        }
        return;
    }
    std::vector<Block4> blocks;
    w4_host_blocks(p, L, blocks);
    dvae_train_plan_t tmp = p;
    std::vector<int> s;
    w4_class_slices(tmp, blocks, 256, s, group);
    struct It { W4Item it; double cost; };
    // items that read the same stash lines -- the blocks of one layer cut the same way, over the same frames -- form a group: one XCD
    std::map<std::tuple<int, int64_t, int>, std::vector<It>> groups;
    for (int b = 0; b < (int)blocks.size(); ++b) {
        if (s[b] == 0) continue;                                          // not in this group's launch
        const int64_t kper = w4_kper(p, s[b]);
        const int eff = (int)((p.Bp + kper - 1) / kper);
        const double c = w4_block_cost(p, blocks[b]);
        for (int i = 0; i < eff; ++i) {
            W4Item it{b, i, (int64_t)i * kper, std::min<int64_t>((int64_t)(i + 1) * kper, p.Bp)};
            groups[std::make_tuple(blocks[b].layer, kper, i)].push_back(It{it, c * (double)(it.kend - it.kbeg)});
        }
    }
    std::vector<std::vector<It>> gl;
    for (auto& kv : groups) gl.push_back(kv.second);
    auto gcost = [](const std::vector<It>& g) { double t = 0; for (const It& i : g) t += i.cost; return t; };
    std::stable_sort(gl.begin(), gl.end(), [&](const std::vector<It>& a, const std::vector<It>& b) { return gcost(a) > gcost(b); });
    std::vector<It> lists[8];
    double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int cap = 32;                                                   // CUs of an XCD: one round of workgroups
    auto lightest = [&](int need) { int best = -1; for (int x = 0; x < 8; ++x) if ((int)lists[x].size() + need <= cap && (best < 0 || load[x] < load[best])) best = x; return best; };
    for (auto& g : gl) {
        int x = lightest((int)g.size());
        if (x >= 0) { for (const It& i : g) { lists[x].push_back(i); load[x] += i.cost; } continue; }
        for (const It& i : g) {                                           // no XCD has room for the whole group: item by item
            x = lightest(1);
            if (x < 0) { x = 0; for (int q = 1; q < 8; ++q) if (lists[q].size() < lists[x].size()) x = q; }      // (more than 256 items: cannot happen by construction)
            lists[x].push_back(i); load[x] += i.cost;
        }
    }
    size_t maxlen = 0;
    for (int x = 0; x < 8; ++x) {
        std::stable_sort(lists[x].begin(), lists[x].end(), [](const It& a, const It& b) { return a.cost > b.cost; });      // longest first
        maxlen = std::max(maxlen, lists[x].size());
    }
    out.grid = (int)(8 * maxlen);
    out.items.assign((size_t)out.grid, W4Item{-1, 0, 0, 0});
    for (int x = 0; x < 8; ++x)
        for (size_t q = 0; q < lists[x].size(); ++q) out.items[q * 8 + x] = lists[x][q].it;
}

extern "C" int dvae_train_repack(const dvae_train_plan_t* plan, const float* params, void* ws, void* stream) {
    DVAE_CHECK_ARG(plan && params && ws, "train_repack: bad argument");
    DVAE_CHECK_ARG(!defer_state_get(ws).pending, "train_repack: an optimizer update is pending on this workspace (dvae_train_step_deferred): call dvae_train_flush BEFORE writing parameters");
    Layout L;
    make_layout(*plan, L);
    return launch_apply(plan, L, const_cast<float*>(params), nullptr, nullptr, (char*)ws, 0, false, 1, 0, 0, 0, 0, 0, nullptr, (hipStream_t)stream);
}

extern "C" int dvae_train_init(const dvae_train_plan_t* plan, const float* params, void* ws, void* stream) {
    DVAE_CHECK_ARG(plan && params && ws, "train_init: bad argument");
    Layout L;
    make_layout(*plan, L);
    DVAE_CHECK_ARG(L.total == plan->workspace_bytes, "train_init: plan does not match this library (workspace %lld vs %lld)",
                   (long long)plan->workspace_bytes, (long long)L.total);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    DVAE_HIP(hipMemsetAsync(w, 0, (size_t)L.total, s));
    fold_seq_reset(ws);
    defer_state_reset(ws);
    GroupDesc* tiles = new GroupDesc[L.ntiles + 8];
    BlockDesc* blocks = new BlockDesc[L.nblocks + 8];
    Block4* blocks4 = new Block4[L.nblocks4 + 8];
    TensorDesc td[DVAE_TRAIN_MAX_TENSORS];
    memset(td, 0, sizeof(td));
    if (is_bf(plan->precision)) fill_tables<__bf16>(plan, L, w, tiles, blocks, blocks4, td);
    else fill_tables<float>(plan, L, w, tiles, blocks, blocks4, td);
    hipError_t e1 = hipMemcpyAsync(w + L.o_tiles, tiles, (size_t)L.ntiles * sizeof(GroupDesc), hipMemcpyHostToDevice, s);
    hipError_t e2 = hipMemcpyAsync(w + L.o_tensors, td, sizeof(td), hipMemcpyHostToDevice, s);
    hipError_t e5 = hipMemcpyAsync(w + L.o_blocks, blocks, (size_t)L.nblocks * sizeof(BlockDesc), hipMemcpyHostToDevice, s);
    hipError_t e6 = hipMemcpyAsync(w + L.o_blocks4, blocks4, (size_t)L.nblocks4 * sizeof(Block4), hipMemcpyHostToDevice, s);
    W4Sched sched[3];                                                     // [0]: the one launch; [1], [2]: the two launches of a grouped plan
    W4Grids grids{{0, 0, 0}};
    hipError_t e8 = hipSuccess;
    for (int t = 0; t < 3; ++t) {
        const bool grouped = w4_grouped(*plan);
        if ((t == 0) == grouped) continue;                                // a plan uses either table 0 or tables 1 and 2
        w4_build_items(*plan, L, sched[t], t - 1);
        DVAE_CHECK_ARG(sched[t].grid > 0 && sched[t].grid <= W4_MAX_ITEMS, "train_init: weight-gradient schedule of %d workgroups does not fit the item table", sched[t].grid);
        grids.g[t] = sched[t].grid;
        const hipError_t e = hipMemcpyAsync(w + L.o_items4 + (int64_t)t * W4_MAX_ITEMS * sizeof(W4Item), sched[t].items.data(), sched[t].items.size() * sizeof(W4Item), hipMemcpyHostToDevice, s);
        if (e8 == hipSuccess) e8 = e;
    }
    const int64_t nchunks = plan->n_params / 64;
    unsigned char* ct = new unsigned char[nchunks + 64];
    memset(ct, 255, (size_t)nchunks + 64);
    for (int t = 0; t < plan->n_tensors; ++t) {
        const int64_t c0 = plan->tensor_offset[t] / 64, ne = (int64_t)plan->tensor_rows[t] * plan->tensor_cols[t];
        for (int64_t c = c0; c < c0 + (ne + 63) / 64; ++c) ct[c] = (unsigned char)t;
    }
    hipError_t e4 = hipMemcpyAsync(w + L.o_chunks, ct, (size_t)nchunks, hipMemcpyHostToDevice, s);
    DeferTask* dt = new DeferTask[DEFER_MAX_TASKS];
    memset(dt, 0, sizeof(DeferTask) * DEFER_MAX_TASKS);
    { DeferState st; st.ntasks = build_defer_tasks(plan, td, dt, DEFER_MAX_TASKS); defer_state_put(ws, st); }
    hipError_t e7 = hipMemcpyAsync(w + L.o_defer, dt, sizeof(DeferTask) * DEFER_MAX_TASKS, hipMemcpyHostToDevice, s);
    hipError_t e3 = hipStreamSynchronize(s);
    delete[] dt;
    delete[] tiles;
    delete[] blocks;
    delete[] blocks4;
    delete[] ct;
    DVAE_HIP(e1); DVAE_HIP(e2); DVAE_HIP(e4); DVAE_HIP(e5); DVAE_HIP(e6); DVAE_HIP(e7); DVAE_HIP(e8); DVAE_HIP(e3);
    w4_grid_put(ws, grids);
    return dvae_train_repack(plan, params, ws, stream);
}

// dvae_train_step -> run_grads: "run the optimizer step in the weight-gradient launch if you can" (done: the answer, it did)
struct FoldRequest { bool want = false, done = false; PendingUpdate u{}; float* losses3 = nullptr; };

static int device_cu_count(int dev) {
    static int cus[64] = {};
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 1;
        cus[dev] = n;
    }
    return cus[dev];
}

// The pending update of a workspace (dvae_train_step_deferred), applied now with apply_kernel: the same slab sums, the same element
// arithmetic as the in-kernel form.  Every entry point that reads parameters, moments, weight copies or gradient slabs calls this first.
extern "C" int dvae_train_flush(const dvae_train_plan_t* plan, void* ws, void* stream) {
    DVAE_CHECK_ARG(plan && ws, "train_flush: bad argument");
    DeferState st = defer_state_get(ws);
    if (!st.pending) return 0;
    Layout L;
    make_layout(*plan, L);
    st.pending = false;
    defer_state_put(ws, st);
    ProfScope ps((hipStream_t)stream, 3);
    return launch_apply(plan, L, st.u.params, st.u.m, st.u.v, (char*)ws, st.u.n_slabs, true, st.u.step, st.u.lr, st.u.beta1, st.u.beta2, st.u.adam_eps,
                        1.0, nullptr /* the step's loss scalars were finalised by its own rows kernel */, (hipStream_t)stream);
}

extern "C" int dvae_train_pending(const void* ws) { return defer_state_get(ws).pending ? 1 : 0; }

// can this plan run the deferred form?  (8-wave rows kernel, M1 / M2 train step; the whole grid resident at once: one workgroup per CU;
// at most two update tasks per chain wave: otherwise the update would take longer in the opening than in its own launch)
static bool defer_possible(const dvae_train_plan_t* plan, const void* ws) {
    if (!(plan->rows_kernel == 2 && rows2_supported(plan->precision, plan->model))) return false;
    if (!(plan->model == DVAE_MODEL_M1 || plan->model == DVAE_MODEL_M2)) return false;
    if (plan->row_index != 0 && plan->row_count <= 0) return false;
    const int dev = current_device();
    const int nt = defer_state_get(ws).ntasks;
    if (nt <= 0 || nt > DEFER_MAX_TASKS) return false;
    if (plan->rows_grid > device_cu_count(dev) || 8 * plan->rows_grid < 4 * nt) return false;      // at most two 8-row units per chain wave
    if (wgrad_form_env() != 4 || plan->Bp <= 128) return false;      // the loss scalars come from an extra workgroup of wgrad4_kernel
    const int64_t kper = kper_of(plan);
    return (plan->Bp + kper - 1) / kper <= 12;
}

extern "C" int dvae_train_can_defer(const dvae_train_plan_t* plan, const void* ws) {
    if (!plan || !ws) return 0;
    // OPT-IN (DVAE_DEFER_APPLY=1): bit-identical and, on the MI355X, not faster -- see DESIGN.md (round 4, item 3) for the ablation
    if (!kDiagBuild || env_int("DVAE_DEFER_APPLY", 0) != 1 || getenv("DVAE_FOLD_APPLY") != nullptr) return 0;      // (the deferred rows kernel exists in -DDVAE_DIAG builds only)
    return defer_possible(plan, ws) ? 1 : 0;
}

// What one gradient pass runs beyond the arguments of dvae_train_grads (the defaults: dvae_train_grads itself); the entry points fill in theirs
struct GradsOptions {
    int mode = 0;                       // rows kernel: 0 the train step, 1 dvae_module_forward (writes out_*), 2 dvae_module_backward (reads g_*)
    float *out_r = nullptr, *out_mu = nullptr, *out_lv = nullptr, *out_z = nullptr;
    const float *g_r = nullptr, *g_mu = nullptr, *g_lv = nullptr, *g_z = nullptr;
    int ld_r = 0, ld_gr = 0;
    bool rows_only = false;             // dvae_train_eval: no weight-gradient launch (mode 1 stops after the rows kernel too)
    long long rng_step = -1;            // dvae_train_step, dvae_train_step_deferred: their `step` argument numbers the noise draw; -1 = plan->rng_step
    int group = -1;                     // dvae_train_grads_group: -1 the whole step, 0 rows + first wgrad launch, 1 second wgrad launch
    DeferRequest defer;                 // dvae_train_step_deferred
    FoldRequest fold;                   // dvae_train_step; fold.done comes back
};

namespace {      // (internal: the constructor is a real function)
// The environment of one gradient pass, read once at the top of run_grads -- per call: tests flip these between calls.
struct StepEnv {
    // DVAE_WGRAD (wgrad_form_env).  =lds selects the workgroup-blocked kernel for the bf16 policies (operands staged once per 4 x 4 block in
    // LDS: half the L2 -> CU operand traffic).  Measured (M2 y513, 8192 frames): 39.3 vs 32.9 us under bf16x3, 25.0 vs 21.4 us under bf16 --
    // SLOWER than the register-ring kernel at every k-split tried, and both kernels take the same time on a stash that is already cache-warm:
    // the weight-gradient pass is bound neither by operand traffic nor by cold reads.  The register-ring kernel stays default.
    bool wgrad_set = false;
    int wgrad_form = wgrad_form_env(&wgrad_set);
    int ablate = env_int("DVAE_ABLATE", 0);
    // DVAE_RAW_INPUTS=1 (opt-in, tested): the weight-gradient kernel takes x and the labels straight from the fp32 input matrices and the
    // rows kernel writes no stash for them (35 MB of writes less in its HBM-bound opening window).  Measured (M2 y513, 8192 frames, bf16x3,
    // same box, alternating): rows 46.0 -> 44.0 us, but the weight-gradient kernel 29.0 -> 34.6 us -- its input-fed blocks convert and
    // transpose 8 KB per k-step and wave through LDS behind a two-deep ring -- so the stash stays the default (step 78.6 vs 81.8 us).
    // Round 4, large batches: from ~1e5 frames on the rows kernel runs many tiles per workgroup and sets the step time (4.7 ns per frame against
    // 2.5 for the weight-gradient kernel, which is HBM-bound there), so the 6.3 KB per frame of input stash it no longer writes pay:
    // B = 262 144: 139.3 -> 143.2 M frames/s, B = 2^20: 137.0 -> 142.8 (x only: 143.3 / 139.1; profiles/r04_bigb_raw.txt).  Chosen
    // automatically from DVAE_RAW_AUTO_B frames on (131 072); DVAE_RAW_INPUTS=0 keeps the stash, =x / =1 force a variant at any size.
    // -1 unset, 0 "0"; else the mask of inputs read raw: 1 "x" (only the x tile; the label stash stays: one plane for binary labels), 3 any other value
    int raw_inputs = -1;
    int64_t raw_auto_b = env_ll("DVAE_RAW_AUTO_B", 131072);
    bool ylo_always = getenv("DVAE_YLO_ALWAYS") != nullptr;
    int wgrad_repeat = std::max(env_int("DVAE_WGRAD_REPEAT", 1), 1);      // diagnostic: re-run the weight-gradient launch on the warm stash
    int gpw = env_int("DVAE_GPW", 2);                                     // diagnostic override: groups (waves) per workgroup of the 2 x 2 kernel, 1..4
    unsigned fold_max_polls = 1u << 20;                                   // DVAE_FOLD_MAX_POLLS
    int defer_diag = env_int("DVAE_DEFER_DIAG", 0);
    long long defer_timeout_ms = std::max(env_ll("DVAE_DEFER_TIMEOUT_MS", 2000), 0ll);      // bound of the arrival wait (the whole grid is resident: it is microseconds)
    StepEnv() {
        if (const char* v = getenv("DVAE_RAW_INPUTS")) raw_inputs = strcmp(v, "0") == 0 ? 0 : (strcmp(v, "x") == 0 ? 1 : 3);
        if (gpw < 1 || gpw > 4) gpw = 2;
        if (const char* v = getenv("DVAE_FOLD_MAX_POLLS")) fold_max_polls = (unsigned)strtoul(v, nullptr, 10);
    }
};
}

// A grouped step is two calls: the launch of group 1 belongs to the rows kernel of the group 0 call on the same workspace and reuses its
// launch id, or its label blocks would misread the epoch word.  The one state that crosses calls, per thread.
static thread_local struct GroupPairing { unsigned last_id = 0; const void* last_ws = nullptr; } g_pairing;

// the rows kernel's arguments from plan, layout and options (all but ylo_skip, which run_grads decides); host arithmetic only
static int fill_rows_args(const dvae_train_plan_t* plan, const Layout& L, const GradsOptions& o, const StepEnv& env, const float* params, char* w,
                          const float* x, int ldx, const float* y, int ldy, const float* eps_noise, float elbo_eps, RowsArgs& a) {
    const int esz = is_bf(plan->precision) ? 2 : 4;
    memset(&a, 0, sizeof(a));
    a.rows = (const int64_t*)(uintptr_t)plan->row_index;
    a.n_rows = plan->row_count; a.bad_rows = (int*)(uintptr_t)plan->bad_row_counter;
    DVAE_CHECK_ARG(a.rows == nullptr || a.n_rows > 0, "train_grads: row_index set but row_count <= 0");
    a.rng_seed = plan->rng_seed; a.rng_step = o.rng_step >= 0 ? (unsigned long long)o.rng_step : plan->rng_step;
    a.x = x; a.y = y; a.eps = eps_noise; a.ldx = ldx; a.ldy = plan->y_dim ? ldy : 0; a.ydim = plan->y_dim;
    a.fastx = (ldx == XD) && (((uintptr_t)x & 15) == 0);
    a.fasty = (plan->y_dim == XD) && (ldy == XD) && (((uintptr_t)y & 15) == 0);
    a.B = plan->B; a.Bp = plan->Bp; a.ntiles = (int)((plan->B + TB - 1) / TB);
    a.invB = (float)(1.0 / (double)plan->B); a.elbo_eps = elbo_eps;
    char* wc = w + L.o_wcopy;
    auto WC = [&](int64_t off) { return (const void*)(wc + off * esz); };
    a.W1s = WC(L.W1s); a.W2s = WC(L.W2s); a.Wmvs = WC(L.Wmvs); a.W3s = WC(L.W3s); a.W4s = WC(L.W4s); a.W5s = WC(L.W5s);
    a.W5t = WC(L.W5t); a.W4t = WC(L.W4t); a.W3zt = WC(L.W3zt); a.Wmvt = WC(L.Wmvt); a.W2t = WC(L.W2t);
    a.b1 = params + plan->tensor_offset[1]; a.b2 = params + plan->tensor_offset[3];
    a.bmu = params + plan->tensor_offset[5]; a.blv = params + plan->tensor_offset[7];
    a.b3 = params + plan->tensor_offset[9]; a.b4 = params + plan->tensor_offset[11]; a.b5 = params + plan->tensor_offset[13];
    a.w5last = params + plan->tensor_offset[12] + (int64_t)(XD - 1) * HD;
    if (L.info) {
        a.Wc1s = WC(L.Wc1s); a.Wc2s = WC(L.Wc2s); a.Wc2t = WC(L.Wc2t); a.Wa1s = WC(L.Wa1s); a.Wa1t = WC(L.Wa1t); a.Wa2s = WC(L.Wa2s); a.Wa2t = WC(L.Wa2t);
        a.bc1 = params + plan->tensor_offset[15]; a.bc2 = params + plan->tensor_offset[17]; a.wc3 = params + plan->tensor_offset[18]; a.bc3 = params + plan->tensor_offset[19];
        a.ba1 = params + plan->tensor_offset[21]; a.ba2 = params + plan->tensor_offset[23]; a.wa3 = params + plan->tensor_offset[24]; a.ba3 = params + plan->tensor_offset[25];
        a.alpha = (float)plan->info_alpha; a.beta = (float)plan->info_beta; a.gamma = (float)plan->info_gamma;
    }
    a.partials = (double*)(w + L.o_partials);
    a.wcopy = wc; a.wcopy_bytes = L.wcopy_elems * esz * planes_of(plan->precision);
    a.spl = L.stash_rows * plan->Bp; a.wpl_bytes = (unsigned)(L.wcopy_elems * esz);
    a.dbg = g_dbg; a.ablate = env.ablate;
    if (o.defer.on) {
        const PendingUpdate& u = o.defer.u;
        a.defer.on = 1; a.defer.have = o.defer.have ? 1 : 0;
        a.defer.diag = env.defer_diag;
        a.defer.a = o.defer.have ? make_apply_args(plan, L, u.params, u.m, u.v, w, u.n_slabs, true, u.step, u.lr, u.beta1, u.beta2, u.adam_eps, 1.0, o.defer.losses3)
                                 : make_apply_args(plan, L, const_cast<float*>(params), nullptr, nullptr, w, 1, false, 1, 0, 0, 0, 0, 0, o.defer.losses3);
        a.defer.tasks = (const DeferTask*)(w + L.o_defer); a.defer.ntasks = defer_state_get(w).ntasks;
        a.defer.shard = (unsigned*)(w + L.o_defer + DEFER_O_SHARD);
        a.defer.done = (unsigned*)(w + L.o_defer + DEFER_O_DONE); a.defer.err = a.defer.done + 1;
        a.defer.seq_arrive = o.defer.seq_arrive; a.defer.seq_done = o.defer.seq_done;
        a.defer.timeout_ticks = (unsigned long long)env.defer_timeout_ms * 100000ull;
    }
    const bool raw_possible = plan->rows_kernel >= 2 && rows2_supported(plan->precision, plan->model) && a.rows == nullptr &&
                              env.wgrad_form == 4 && o.mode != 1;
    const bool raw_auto = env.raw_inputs < 0 && raw_possible && o.mode == 0 && plan->B >= env.raw_auto_b;
    const int raw_mask = !raw_possible ? 0 : (raw_auto ? 3 : std::max(env.raw_inputs, 0));
    a.stash_inputs = 3 & ~raw_mask;
    a.mode = o.mode;
    a.ylo_epoch = (unsigned*)(w + L.o_flags); a.ylo_dirty = (int*)(w + L.o_flags + 1024);
    static std::atomic<unsigned> launch_counter{1};
    if (o.group == 1) {
        DVAE_CHECK_ARG(g_pairing.last_ws == w && g_pairing.last_id != 0, "train_grads_group: group 1 must follow a group 0 call on the same workspace");
        a.launch_id = g_pairing.last_id;
    } else {
        a.launch_id = launch_counter.fetch_add(1, std::memory_order_relaxed);
        if (a.launch_id == 0) a.launch_id = launch_counter.fetch_add(1, std::memory_order_relaxed);      // 0 = the memset value of a fresh workspace
        g_pairing = GroupPairing{a.launch_id, w};
    }
    a.out_r = o.out_r; a.out_mu = o.out_mu; a.out_lv = o.out_lv; a.out_z = o.out_z; a.ld_r = o.ld_r;
    a.g_r = o.g_r; a.g_mu = o.g_mu; a.g_lv = o.g_lv; a.g_z = o.g_z; a.ld_gr = o.ld_gr;
    DVAE_CHECK_ARG(a.mode == 0 || plan->rows_kernel == 2, "rows-kernel modes 1 / 2 exist in the 8-wave kernel only (plan->rows_kernel == 2)");
    char* st = w + L.o_stash;
    auto ST = [&](int64_t row) { return (void*)(st + row * plan->Bp * esz); };
    a.xT = ST(L.xT); a.yT = ST(L.yT); a.h1T = ST(L.h1T); a.h2T = ST(L.h2T); a.dh1T = ST(L.dh1T); a.dh2T = ST(L.dh2T);
    a.dmlvT = ST(L.dmlvT); a.zT = ST(L.zT); a.d1T = ST(L.d1T); a.d2T = ST(L.d2T); a.dd1T = ST(L.dd1T); a.dd2T = ST(L.dd2T); a.daT = ST(L.daT);
    if (L.info) {
        a.c1T = ST(L.c1T); a.c2T = ST(L.c2T); a.dc1T = ST(L.dc1T); a.dc2T = ST(L.dc2T); a.dc3T = ST(L.dc3T);
        a.a1T = ST(L.a1T); a.a2T = ST(L.a2T); a.da1T = ST(L.da1T); a.da2T = ST(L.da2T); a.da3T = ST(L.da3T);
    }
    return 0;
}

static int launch_rows_kernel(const dvae_train_plan_t* plan, const RowsArgs& a, hipStream_t s) {
    const int grid = (int)plan->rows_grid;
    if (plan->rows_kernel == 3 && rows3_supported(plan->precision, plan->model)) return launch_rows3(plan->model, plan->y_dim, a, grid, s);
    if (plan->rows_kernel == 2 && rows2_supported(plan->precision, plan->model)) return launch_rows2(plan->precision, plan->model, plan->y_dim, a, grid, s);
    return launch_rows1(plan->precision, plan->model, plan->y_dim, a, grid, s);
}

// the weight-gradient launch(es) over the stash the rows kernel left, then the optional slab reduction; wg4: the workgroup k-split kernel
static int launch_wgrad_pass(const dvae_train_plan_t* plan, const Layout& L, GradsOptions& o, const StepEnv& env, const RowsArgs& a, bool wg4,
                             char* w, int reduce_slabs, hipStream_t s) {
    const bool x3 = plan->precision == DVAE_PREC_BF16X3;
    const int64_t kper = kper_of(plan);
    const int ks = used_slabs(plan);                                      // slabs the launch fills
    DVAE_CHECK_ARG(ks <= plan->ksplit, "train_grads: internal k-split mismatch");
    DVAE_CHECK_ARG(!w4_classed(*plan) || env.wgrad_form == 4,
                   "train_grads: the plan was made for the workgroup k-split weight-gradient kernel (class-sliced schedule); DVAE_WGRAD changed since");
    float* slabs = (float*)(w + L.o_grads);
    const WgradArgs wa{ks, plan->Bp, a.spl, kper, slabs, plan->n_params};      // (the two uniform-slice kernels)
    for (int rep = 0; rep < env.wgrad_repeat; ++rep) {
        if (wg4) {
            // one launch (table 0), or the launches of a grouped plan: tables 1 and 2, both (group < 0) or the one asked for
            const int tb0 = !w4_grouped(*plan) ? 0 : (o.group == 1 ? 2 : 1), tb1 = !w4_grouped(*plan) ? 0 : (o.group == 0 ? 1 : 2);
            for (int tb = tb0; tb <= tb1; ++tb) {
                ProfScope ps(s, rep == 0 ? 1 : 2);
                const int w4grid = w4_grid_get(w, tb);
                DVAE_CHECK_ARG(w4grid > 0, "train_grads: workspace was not set up by dvae_train_init");
                const dim3 g3((unsigned)w4grid);                                  // one workgroup per item of the host's table (w4_build_items)
                const RawIn ri{a.x, a.y, a.ldx, a.ldy, a.B};
                const int use_raw = 3 & ~a.stash_inputs;
                const Block4* bl = (const Block4*)(w + L.o_blocks4);
                const W4Item* w4items = (const W4Item*)(w + L.o_items4) + (size_t)tb * W4_MAX_ITEMS;
                // the optimizer step in this launch's tail (dvae_train_step asked for it): only when every workgroup of the grid is resident at
                // once -- one per CU, the tail's wait depends on it -- and the block counters fit the flag header
                ApplyArgs fa_apply;
                memset(&fa_apply, 0, sizeof(fa_apply));
                FoldArgs fold{nullptr, 0u, 0u};
                const PendingUpdate& u = o.fold.u;
                if (o.fold.want && !w4_classed(*plan) && env.wgrad_repeat == 1 && a.mode == 0 && ks > 1 && ks <= 16 && L.nblocks4 <= FOLD_MAXB && (int)g3.x <= device_cu_count(current_device())) {
                    fa_apply = make_apply_args(plan, L, u.params, u.m, u.v, w, ks, true, u.step, u.lr, u.beta1, u.beta2, u.adam_eps, 1.0, o.fold.losses3);
                    fold.cnt = (unsigned*)(w + L.o_flags);
                    fold.target = (unsigned)ks * fold_seq_next(w);
                    fold.max_polls = env.fold_max_polls;
                    o.fold.done = true;
                }
                int fin_block = -1;
                const unsigned* fin_err = nullptr;
                dim3 g3l = g3;
                if (a.defer.on) {                                             // + one workgroup that turns the rows kernel's partial sums into the loss scalars
                    fa_apply = a.defer.a;
                    fin_block = (int)g3.x; fin_err = a.defer.err;
                    g3l = dim3(g3.x + 1);
                }
                const Wgrad4Args w4a{bl, w4items, ks, plan->Bp, a.spl, slabs, plan->n_params, ri, use_raw,
                                     a.ylo_skip ? a.ylo_epoch : nullptr, x3 ? a.launch_id : 0u /* the split-bf16 kernel alone reads them */, fa_apply, fold, fin_block, fin_err};
                const int rc = launch_wgrad4(plan->precision, w4a, (int)g3l.x, s);
                if (rc) return rc;
            }
        } else if (is_bf(plan->precision) && env.wgrad_form == 1) {
            ProfScope ps(s, rep == 0 ? 1 : 2);
            const int rc = launch_wgrad_lds(plan->precision, (const BlockDesc*)(w + L.o_blocks), L.nblocks, wa, s);
            if (rc) return rc;
        } else {
            ProfScope ps(s, rep == 0 ? 1 : 2);
            const int rc = launch_wgrad_ring(plan->precision, (const GroupDesc*)(w + L.o_tiles), L.ntiles, wa, env.gpw, s);
            if (rc) return rc;
        }
    }
    if (reduce_slabs && ks > 1) {
        ProfScope ps(s, 2);
        int64_t lo, hi;                                                   // a group's launch reduces its own part of the flat gradient
        dvae_train_group_range(plan, o.group, &lo, &hi, nullptr);
        return launch_slab_reduce(slabs + lo, hi - lo, ks, plan->n_params, s);
    }
    return 0;
}

// The gradient pass behind every entry point below: rows kernel, then the weight-gradient launches.  A pending deferred update is applied
// first -- unless this call IS the deferred step, whose rows kernel applies it in its opening.
static int run_grads(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx, const float* y, int ldy,
                     const float* eps_noise, float elbo_eps, int reduce_slabs, void* stream, GradsOptions& o) {
    DVAE_CHECK_ARG(plan && params && ws && x && ldx >= XD, "train_grads: bad argument");
    DVAE_CHECK_ARG(plan->y_dim == 0 || (y != nullptr && ldy >= plan->y_dim), "train_grads: y missing or ldy < y_dim");
    if (!o.defer.on) { const int frc = dvae_train_flush(plan, ws, stream); if (frc) return frc; }
    const StepEnv env;
    Layout L;
    make_layout(*plan, L);
    hipStream_t s = (hipStream_t)stream;
    RowsArgs a;
    { const int rc = fill_rows_args(plan, L, o, env, params, (char*)ws, x, ldx, y, ldy, eps_noise, elbo_eps, a); if (rc) return rc; }
    // the weight-gradient launch is the workgroup k-split kernel -- but for one 128-frame slice: there the 2 x 2 kernel's short epilogue wins (11.2 vs 12.8 us)
    const bool wg4 = env.wgrad_form == 4 && (plan->Bp > 128 || a.stash_inputs != 3 /* raw inputs */ || env.wgrad_set);
    // label lo plane on demand: 8-wave kernel + the workgroup k-split weight-gradient kernel, split-bf16 operands, labels from the stash
    a.ylo_skip = (plan->precision == DVAE_PREC_BF16X3 && plan->y_dim > 0 && plan->rows_kernel >= 2 && rows2_supported(plan->precision, plan->model) && wg4 &&
                  (a.stash_inputs & 2) && !env.ylo_always) ? 1 : 0;
    DVAE_CHECK_ARG(o.group < 0 || (w4_grouped(*plan) && o.mode == 0 && !o.rows_only), "train_grads_group: the plan was not made for two weight-gradient launches (DVAE_EXCHANGE_GROUPS=2 when the plan is made)");
    if (o.group != 1) {
        ProfScope ps(s, 0);
        const int rc = launch_rows_kernel(plan, a, s);
        if (rc) return rc;
    }
    if (o.rows_only || a.mode == 1) return 0;
    return launch_wgrad_pass(plan, L, o, env, a, wg4, (char*)ws, reduce_slabs, s);
}

extern "C" int dvae_train_grads(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                                const float* y, int ldy, const float* eps_noise, float elbo_eps, int reduce_slabs, void* stream) {
    GradsOptions o;
    return run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, elbo_eps, reduce_slabs, stream, o);
}

// The step's gradient pass in two calls, for a plan made under DVAE_EXCHANGE_GROUPS=2: group 0 = the rows kernel + the weight-gradient launch of
// the decoder-side tensors (flat gradient [tensor_offset[8], n_params)), group 1 = the launch of the encoder's ([0, tensor_offset[8])); the
// caller may start the exchange of group 0's part between the two calls.  dvae_train_grads on such a plan runs both.
extern "C" int dvae_train_grads_group(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx, const float* y, int ldy,
                                      const float* eps_noise, float elbo_eps, int group, int reduce_slabs, void* stream) {
    DVAE_CHECK_ARG(plan && (group == 0 || group == 1), "train_grads_group: group must be 0 or 1");
    DVAE_CHECK_ARG(w4_grouped(*plan), "train_grads_group: the plan was not made for two weight-gradient launches (DVAE_EXCHANGE_GROUPS=2 when the plan is made)");
    GradsOptions o;
    o.group = group;
    return run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, elbo_eps, reduce_slabs, stream, o);
}

// float range [lo, hi) of a group's part of the flat gradient (group < 0: everything); *ngroups = 2 for a plan made for two launches, else 1
extern "C" int dvae_train_group_range(const dvae_train_plan_t* plan, int group, int64_t* lo, int64_t* hi, int* ngroups) {
    DVAE_CHECK_ARG(plan && lo && hi && group >= -1 && group <= 1, "train_group_range: bad argument");
    *lo = 0; *hi = plan->n_params;
    if (group == 0) *lo = plan->tensor_offset[8];
    if (group == 1) *hi = plan->tensor_offset[8];
    if (ngroups) *ngroups = w4_grouped(*plan) ? 2 : 1;
    return 0;
}

extern "C" int dvae_train_apply(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws, int n_slabs,
                                int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale,
                                float* losses3, void* stream) {
    DVAE_CHECK_ARG(plan && params && m && v && ws && step >= 1, "train_apply: bad argument");
    { const int frc = dvae_train_flush(plan, ws, stream); if (frc) return frc; }
    Layout L;
    make_layout(*plan, L);
    if (n_slabs <= 0) n_slabs = used_slabs(plan);
    DVAE_CHECK_ARG(n_slabs <= plan->ksplit, "train_apply: n_slabs %d > plan ksplit %d", n_slabs, plan->ksplit);
    ProfScope ps((hipStream_t)stream, 3);
    return launch_apply(plan, L, params, m, v, (char*)ws, n_slabs, true, step, lr, beta1, beta2, adam_eps, grad_scale, losses3,
                        (hipStream_t)stream);
}

extern "C" int dvae_train_step(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws,
                               const float* x, int ldx, const float* y, int ldy, const float* eps_noise, float elbo_eps,
                               int step, double lr, double beta1, double beta2, double adam_eps, float* losses3, void* stream) {
    DVAE_CHECK_ARG(plan && params && m && v && ws && step >= 1, "train_step: bad argument");
    // DVAE_FOLD_APPLY=1: the optimizer step in the tail of the weight-gradient launch (two launches per step; results bit-identical,
    // tested).  Opt-in, because it is SLOWER on the MI355X (M2 y513, 8192 frames, bf16x3, same box, alternating): the weight-gradient
    // kernel goes 28.7 -> 47.1 us while the separate optimizer launch it replaces costs 9.5 us gross.  Ablation of the 18.4 us tail
    // (FOLD_DIAG builds): arrive + wait for the block's slices 2.6 us; the 13 MB of slab partials + p, m, v as device-coherent loads
    // 8 us; Adam + weight-copy element math and stores 8 us -- the kernel runs ONE wave per SIMD (512 registers of accumulators), so
    // both phases are latency-bound, whereas apply_kernel does the same work at full occupancy in ~6 us behind a ~3 us launch gap.
    // (First attempt with release / acquire fences instead of write-through stores + coherent loads: 75 us -- every fence writes back
    // or invalidates the XCD's whole L2 under the workgroups that are still multiplying.)
    const bool fold_on = kDiagBuild && env_int("DVAE_FOLD_APPLY", 0) != 0;      // read per call (tests flip it); the folded tail exists in -DDVAE_DIAG builds only
    GradsOptions o;
    o.rng_step = step;
    o.fold = FoldRequest{fold_on, false, PendingUpdate{params, m, v, step, lr, beta1, beta2, adam_eps, 0 /* the launch's own slabs */}, losses3};
    const int rc = run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, elbo_eps, 0, stream, o);
    if (rc) return rc;
    if (o.fold.done) return 0;
    return dvae_train_apply(plan, params, m, v, ws, 0, step, lr, beta1, beta2, adam_eps, 1.0, losses3, stream);
}

// Two launches per step: rows(n) applies the update of step n - 1 in its opening and finalises the losses of step n at its end, wgrad(n)
// leaves the gradient slabs of step n; the update of step n stays PENDING until the next deferred step or dvae_train_flush.
extern "C" int dvae_train_step_deferred(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws,
                                        const float* x, int ldx, const float* y, int ldy, const float* eps_noise, float elbo_eps,
                                        int step, double lr, double beta1, double beta2, double adam_eps, float* losses3, void* stream) {
    DVAE_CHECK_ARG(plan && params && m && v && ws && step >= 1 && losses3, "train_step_deferred: bad argument");
    if (!dvae_train_can_defer(plan, ws))
        return dvae_train_step(plan, params, m, v, ws, x, ldx, y, ldy, eps_noise, elbo_eps, step, lr, beta1, beta2, adam_eps, losses3, stream);   // flushes first
    DeferState st = defer_state_get(ws);
    GradsOptions o;
    o.rng_step = step;
    o.defer = DeferRequest{true, st.pending, st.u, st.seq_arrive + (st.pending ? 1u : 0u), st.seq_done + 1u, losses3};
    const int rc = run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, elbo_eps, 0, stream, o);
    if (rc) return rc;
    st.seq_arrive += st.pending ? 1u : 0u; st.seq_done += 1u;
    st.pending = true;
    st.u = PendingUpdate{params, m, v, step, lr, beta1, beta2, adam_eps, used_slabs(plan)};
    defer_state_put(ws, st);
    return 0;
}

/* ---- whole-model autograd path of the drop-in modules (packages/models/models.py) ---- */
extern "C" int dvae_module_forward(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                                   const float* y, int ldy, const float* eps_noise, float* out_r, int ld_r, float* out_mu,
                                   float* out_lv, float* out_z, int repack, void* stream) {
    DVAE_CHECK_ARG(plan && params && ws && x && eps_noise && out_r && out_mu && out_lv && ld_r >= XD, "module_forward: bad argument");
    DVAE_CHECK_ARG(plan->rows_kernel == 2 && plan->row_index == 0, "module_forward: needs the 8-wave rows kernel and no gather table");
    { const int frc = dvae_train_flush(plan, ws, stream); if (frc) return frc; }
    if (repack) { int rc = dvae_train_repack(plan, params, ws, stream); if (rc) return rc; }
    GradsOptions o;
    o.mode = 1; o.out_r = out_r; o.ld_r = ld_r; o.out_mu = out_mu; o.out_lv = out_lv; o.out_z = out_z;
    return run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, 0.f, 0, stream, o);
}

extern "C" int dvae_module_backward(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                                    const float* y, int ldy, const float* eps_noise, const float* g_r, int ld_gr,
                                    const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate,
                                    void* stream) {
    DVAE_CHECK_ARG(plan && params && ws && x && eps_noise && grad_flat, "module_backward: bad argument");
    DVAE_CHECK_ARG(plan->rows_kernel == 2 && plan->row_index == 0, "module_backward: needs the 8-wave rows kernel and no gather table");
    DVAE_CHECK_ARG(g_r == nullptr || ld_gr >= XD, "module_backward: ld_gr < 513");
    GradsOptions o;
    o.mode = 2; o.g_r = g_r; o.ld_gr = ld_gr; o.g_mu = g_mu; o.g_lv = g_lv; o.g_z = g_z;
    const int rc = run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, 0.f, 0, stream, o);
    if (rc) return rc;
    Layout L;
    make_layout(*plan, L);
    const float* slabs = (const float*)((const char*)ws + L.o_grads);
    return launch_slab_sum(slabs, plan->n_params, used_slabs(plan), plan->n_params, grad_flat, accumulate, (hipStream_t)stream);
}

extern "C" int dvae_train_debug_stamps(void* buf) {
    g_dbg = (unsigned long long*)buf;
    return 0;
}

extern "C" int dvae_train_eval(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                               const float* y, int ldy, const float* eps_noise, float elbo_eps, float* losses3, void* stream) {
    DVAE_CHECK_ARG(plan && params && ws && x && losses3, "train_eval: bad argument");
    // forward + loss sums only: the rows kernel also writes the stash, which is simply not consumed
    Layout L;
    make_layout(*plan, L);
    GradsOptions o;
    o.rows_only = true;
    const int rc = run_grads(plan, params, ws, x, ldx, y, ldy, eps_noise, elbo_eps, 0, stream, o);
    if (rc) return rc;
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    char* w = (char*)ws;
    a.partials = (const double*)(w + L.o_partials); a.npartials = (int)plan->rows_grid; a.B = plan->B; a.losses3 = losses3; a.accum = (double*)(uintptr_t)plan->loss_accum;
    a.info = plan->model == DVAE_MODEL_M2_INFO; a.alpha = (float)plan->info_alpha; a.beta = (float)plan->info_beta; a.gamma = (float)plan->info_gamma;
    return launch_apply_losses(a, (hipStream_t)stream);
}

extern "C" int dvae_train_noise(const dvae_train_plan_t* plan, uint64_t step, float* eps_out, void* stream) {
    DVAE_CHECK_ARG(plan && eps_out, "train_noise: null argument");
    return launch_noise((unsigned long long)plan->rng_seed, (unsigned long long)step, plan->B, eps_out, (hipStream_t)stream);
}

extern "C" int dvae_train_profile(int enable) {
    g_prof = enable != 0;
    return 0;
}

extern "C" int dvae_train_profile_read(double ms[4], int64_t calls[4]) {
    hipError_t e = hipDeviceSynchronize();
    for (int i = 0; i < g_npending; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_pending[i].a, g_pending[i].b) == hipSuccess) {
            g_ms[g_pending[i].which] += (double)t;
            g_calls[g_pending[i].which] += 1;
        }
        (void)hipEventDestroy(g_pending[i].a);
        (void)hipEventDestroy(g_pending[i].b);
    }
    g_npending = 0;
    for (int i = 0; i < 4; ++i) { ms[i] = g_ms[i]; calls[i] = g_calls[i]; g_ms[i] = 0; g_calls[i] = 0; }
    DVAE_HIP(e);
    return 0;
}

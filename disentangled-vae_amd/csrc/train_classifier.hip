// The fused train step for the label classifier alone, Classifier([513, [h1, h2], y_dim]) (packages/models/models.py: relu, relu, sigmoid),
// at ANY covered size, exact fp32, three launches per step (include/dvae_train.h: dvae_train_clf_*;
// disentangled-vae_amd/trainer_classifier.py).  The loop body of the reference's sketch scripts/train_audio_net.py: y_hat = model(x),
// binary_cross_entropy (packages/models/utils.py:55-56, eps inside the logs), backward, Adam, the confusion counts of y_hat > 0.5.
// Limits: x 513, h1 / h2 1..512, y_dim 1..513 -- those of mlp_generic.hip, which runs the trained classifier.
//
// The design is train_generic.hip's; the weight-gradient and apply kernels of train_tables.hip serve this step through its tables, and the
// host path around the launches is train_step_host.hpp's (CStep below describes this step to it):
//   * rows kernel (here): 256 threads own a tile of 16 frames; products on v_mfma_f32_16x16x4_f32 from packed copies in fragment order
//     (tg_gemm).  c1 = relu(x W1^T + b1), c2 = relu(c1 W2^T + b2), a = c2 Wo^T + bo, p = 1 / (1 + exp(-a)); the row loss
//     -sum_j [y log(p + eps) + (1 - y) log(1 - p + eps)]; d loss / d p = -(1 / B) (y / (p + eps) - (1 - y) / (1 - p + eps)) with the eps
//     terms kept (oracle/vae_oracle.py: bce_bwd), dpre_o = dp p (1 - p), dpre2 = (dpre_o Wo) [c2 > 0], dpre1 = (dpre2 W2) [c1 > 0]; no d x.
//     LDS as [k][16]: the x tile (the forward pass is done with it after layer 1: dpre_o takes its place), the label tile, two hidden
//     tiles of max(h1p, h2p) rows: 133 KB at 512 / 512 / y 513, sized from the dims at launch.  c1, c2 and the three pre-activation
//     gradients go to the stash.  Frames past B carry zero pre-activation gradients; padded units and labels carry zeros and count for
//     nothing.  The loss sum per workgroup in double, waves in order; the confusion counts (tp, tn, fp, fn: p > 0.5 against y != 0) as
//     integers per workgroup in the same pass.  No float atomics.
//   * weight-gradient kernel: three matrices; layer 1 reads the caller's x (through the gather table when there is one), layers 2 and 3
//     the stash.  One slab per frame slice, summed in slab order by the apply kernel, which also sums the counts in workgroup order.
//   * 64-bit indexing throughout; a gather index outside [0, row_count) is never dereferenced (row 0 instead, counted).
#include <math.h>
#include <vector>
#include "common.hpp"
#include "../../include/dvae_train.h"
#include "train_step_host.hpp"

namespace dvae {
namespace tc {

using namespace dvae::tg;
using fused::ApplyArgs;

constexpr int C_NT = 6, C_NG = 3;

struct CLayout {
    int y, h1, h2, yp, h1p, h2p, hm;
    int64_t W1, W2, Wo, WoT, W2T, b1, b2, bo, wpack_elems;      // packed copies, float offsets from the start of the workspace
    int S, s_c1, s_c2, s_p1, s_p2, s_po;                          // the stash of one frame: layer outputs, then pre-activation gradients
    int64_t o_items, o_partials, o_counts, o_stash, o_grads, ws_bytes;
    int64_t B, Bp, tiles, rows_grid, slice_frames, n_params;
    int nslices, n_items;
    int64_t lds_bytes;
    int64_t toff[C_NT];
    int trows[C_NT], tcols[C_NT];
};

static bool dims_ok(int h1, int h2, int y) { return y >= 1 && y <= GX && h1 >= 1 && h1 <= G_HMAX && h2 >= 1 && h2 <= G_HMAX; }

static void make_gemms(const CLayout& L, GGemm* G) {
    auto set = [&](int i, int dpre, int nrt, int rows, int wt, int kind, int in_off, int in_w) {
        GGemm& m = G[i];
        memset(&m, 0, sizeof(m));
        m.dpre = dpre; m.nrt = nrt; m.rows = rows; m.wt = wt; m.bt = wt + 1; m.in_kind = kind; m.in_off = in_off; m.in_w = in_w; m.y_w = 0;
        m.cols = in_w;
    };
    set(0, L.s_p1, L.h1p / 16, L.h1, 0, 0, 0, GX);
    set(1, L.s_p2, L.h2p / 16, L.h2, 2, 1, L.s_c1, L.h1);
    set(2, L.s_po, L.yp / 16, L.y, 4, 1, L.s_c2, L.h2);
}

static CLayout make_layout(int h1, int h2, int y, int64_t B, int ksplit_hint) {
    CLayout L;
    memset(&L, 0, sizeof(L));
    L.y = y; L.h1 = h1; L.h2 = h2;
    L.yp = up16(y); L.h1p = up16(h1); L.h2p = up16(h2);
    L.hm = L.h1p > L.h2p ? L.h1p : L.h2p;
    // parameters: Classifier.state_dict() order, 256-byte aligned
    const int rows[C_NT] = {h1, h1, h2, h2, y, y};
    const int cols[C_NT] = {GX, 1, h1, 1, h2, 1};
    int64_t o = 0;
    for (int t = 0; t < C_NT; ++t) {
        L.toff[t] = o; L.trows[t] = rows[t]; L.tcols[t] = cols[t];
        o = al64(o + (int64_t)rows[t] * cols[t]);
    }
    L.n_params = o;
    o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o = al64(o + n); return at; };
    L.W1 = take((int64_t)L.h1p * GXP); L.W2 = take((int64_t)L.h2p * L.h1p); L.Wo = take((int64_t)L.yp * L.h2p);
    L.WoT = take((int64_t)L.h2p * L.yp); L.W2T = take((int64_t)L.h1p * L.h2p);
    L.b1 = take(L.h1p); L.b2 = take(L.h2p); L.bo = take(L.yp);
    L.wpack_elems = o;
    int s = 0;
    auto col = [&](int n) { const int at = s; s += n; return at; };
    L.s_c1 = col(L.h1p); L.s_c2 = col(L.h2p); L.s_p1 = col(L.h1p); L.s_p2 = col(L.h2p); L.s_po = col(L.yp);
    L.S = s;
    L.B = B;
    L.tiles = (B + GT - 1) / GT;
    L.Bp = L.tiles * GT;
    L.rows_grid = L.tiles < G_ROWS_GRID ? L.tiles : G_ROWS_GRID;
    GGemm gm[C_NG];
    make_gemms(L, gm);
    int row_tiles = 0;
    for (int i = 0; i < C_NG; ++i) row_tiles += gemm_items(gm[i]);
    choose_slices(B, row_tiles, ksplit_hint, L.slice_frames, L.nslices);
    L.n_items = row_tiles * L.nslices;
    int64_t w = al256(L.wpack_elems * 4);
    L.o_items = w; w = al256(w + (int64_t)L.n_items * sizeof(GItem));
    L.o_partials = w; w = al256(w + L.rows_grid * 4 * sizeof(double));
    L.o_counts = w; w = al256(w + L.rows_grid * 4 * sizeof(long long));
    L.o_stash = w; w = al256(w + L.Bp * (int64_t)L.S * 4);
    L.o_grads = w; w = al256(w + (int64_t)L.nslices * L.n_params * 4);
    L.ws_bytes = w;
    L.lds_bytes = (int64_t)GT * (GXP + L.yp + 2 * L.hm) * 4 + GT * sizeof(int64_t);
    return L;
}

static void make_tensors(const CLayout& L, GTensor* T) {
    for (int t = 0; t < G_NT; ++t) memset(&T[t], 0, sizeof(GTensor));      // (entries past C_NT: no rows, never matched)
    for (int t = 0; t < C_NT; ++t) {
        GTensor& d = T[t];
        d.off = L.toff[t]; d.rows = L.trows[t]; d.cols = L.tcols[t];
        d.t0 = -1; d.split = d.cols; d.bias = t & 1;
    }
    const int k1 = L.h1p / 16, k2 = L.h2p / 16, ky = L.yp / 16;
    T[0].f0 = L.W1; T[0].kb0 = GKX;
    T[1].f0 = L.b1;
    T[2].f0 = L.W2; T[2].kb0 = k1; T[2].t0 = L.W2T; T[2].tkb = k2; T[2].tcmax = L.h1;
    T[3].f0 = L.b2;
    T[4].f0 = L.Wo; T[4].kb0 = k2; T[4].t0 = L.WoT; T[4].tkb = ky; T[4].tcmax = L.h2;
    T[5].f0 = L.bo;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rows kernel
struct CRowsArgs {
    const float* x; int64_t ldx;
    const float* y; int64_t ldy;
    const int64_t* row_index; int64_t row_count; int* bad;
    float* ws;                        // the packed copies start the workspace
    float* stash; double* partials; long long* counts;
    float bce_eps, invB;
    int fwd_only;
};

__global__ __launch_bounds__(256) void train_clf_rows_kernel(const CLayout L, const CRowsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float csm[];
    float* X = csm;                                     // [528][16] x, then d loss / d a (dpre_o) in its first yp rows
    float* Y = X + GT * GXP;                            // [yp][16]
    float* A = Y + GT * L.yp;                           // [hm][16] c1
    float* Bf = A + GT * L.hm;                          // [hm][16] c2, then dpre2
    int64_t* srow = reinterpret_cast<int64_t*>(Bf + GT * L.hm);         // [16] the frame's row of x / y, -1: past B

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int ky = L.yp >> 4, k1 = L.h1p >> 4, k2 = L.h2p >> 4;
    const float* wp = g.ws;
    const bool bwd = !g.fwd_only;
    double sum_bce = 0.0;
    long long n_tp = 0, n_tn = 0, n_fp = 0, n_fn = 0;

    for (int64_t tile = blockIdx.x; tile < L.tiles; tile += gridDim.x) {
        const int64_t r0 = tile * GT;
        __syncthreads();                                // the previous tile's readers of srow, X, A and Bf are done
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

        // ---- the input and label tiles: a quarter wave reads 16 consecutive values of one frame ----
        for (int b = wave; b < GKX; b += 4) {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
                const int k = 16 * b + col, c = 4 * cq + quad;
                const int64_t s = srow[c];
                X[k * GT + c] = (k < GX && s >= 0) ? g.x[s * g.ldx + k] : 0.f;
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

        // ---- layer 1: c1 = relu(x W1^T + b1) -> A ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W1 + (int64_t)t * GKX * 256, GKX, X, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.b1 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                A[row * GT + col] = h[r];
            }
            st4(L.s_c1, t, h);
        }
        __syncthreads();
        // ---- layer 2: c2 = relu(c1 W2^T + b2) -> Bf ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W2 + (int64_t)t * k1 * 256, k1, A, lane);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const float pre = acc[r] + wp[L.b2 + row];
                h[r] = pre > 0.f ? pre : 0.f;
                Bf[row * GT + col] = h[r];
            }
            st4(L.s_c2, t, h);
        }
        __syncthreads();
        // ---- output layer: a = c2 Wo^T + bo, p = sigmoid(a); BCE; counts; dpre_o = d loss / d p * p (1 - p) -> X rows 0 .. yp - 1 ----
        for (int t = wave; t < ky; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.Wo + (int64_t)t * k2 * 256, k2, Bf, lane);
            f32x4 da;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                const bool ok = fok && row < L.y;
                const float a = acc[r] + wp[L.bo + row];
                const float yv = Y[row * GT + col];
                const float p = 1.f / (1.f + expf(-a));
                const float q = 1.f - p;
                if (ok) {
                    sum_bce -= (double)(yv * logf(p + g.bce_eps) + (1.f - yv) * logf(q + g.bce_eps));
                    const bool hat = p > 0.5f, tru = yv != 0.f;
                    n_tp += hat && tru; n_tn += !hat && !tru; n_fp += hat && !tru; n_fn += !hat && tru;
                }
                const float dp = -g.invB * (yv / (p + g.bce_eps) - (1.f - yv) / (q + g.bce_eps));
                da[r] = ok ? dp * p * q : 0.f;
                if (bwd) X[row * GT + col] = da[r];
            }
            st4(L.s_po, t, da);
        }
        if (!bwd) continue;
        __syncthreads();
        // ---- d c2 = dpre_o Wo; dpre2 = d c2 [c2 > 0] -> Bf (c2: this thread's own entry) ----
        for (int t = wave; t < k2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.WoT + (int64_t)t * ky * 256, ky, X, lane);
            f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                d[r] = Bf[row * GT + col] > 0.f ? acc[r] : 0.f;
                Bf[row * GT + col] = d[r];
            }
            st4(L.s_p2, t, d);
        }
        __syncthreads();
        // ---- d c1 = dpre2 W2; dpre1 = d c1 [c1 > 0]: only the stash needs it ----
        for (int t = wave; t < k1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = tg_gemm(acc, wp + L.W2T + (int64_t)t * k2 * 256, k2, Bf, lane);
            f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = A[(16 * t + 4 * quad + r) * GT + col] > 0.f ? acc[r] : 0.f;
            st4(L.s_p1, t, d);
        }
    }
    // the workgroup's loss sum, waves in order, and its counts: the first bytes of X hold them
    sum_bce = wave_sum(sum_bce);
    __syncthreads();                                    // the last tile's readers of X are done
    double* red = reinterpret_cast<double*>(csm);                       // [4]
    long long* cnt = reinterpret_cast<long long*>(csm) + 4;             // [256][4]: 8 KB of the x tile's 33 KB
    if (lane == 0) red[wave] = sum_bce;
    cnt[4 * tid] = n_tp; cnt[4 * tid + 1] = n_tn; cnt[4 * tid + 2] = n_fp; cnt[4 * tid + 3] = n_fn;
    __syncthreads();
    if (tid == 0) {
        double* p = g.partials + 4 * (int64_t)blockIdx.x;
        p[0] = ((red[0] + red[1]) + red[2]) + red[3];
        p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
    }
    if (tid < 4) {
        long long c = 0;
        for (int i = 0; i < 256; ++i) c += cnt[4 * i + tid];
        g.counts[4 * (int64_t)blockIdx.x + tid] = c;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
static const char* LIMITS = "the classifier train step covers Classifier([513, [h1, h2], y_dim]) at x 513, hidden widths 1..512, y_dim 1..513, exact fp32, one GPU";

// the classifier step as train_step_host.hpp reads it
struct CStep {
    using Plan = dvae_train_clf_plan_t;
    using Layout = CLayout;
    static constexpr int NT = C_NT, NG = C_NG;
    static constexpr int ORDER[C_NG] = {0, 1, 2};                           // layer 1 first: 513 input columns
    static constexpr bool COUNTS = true, WGRAD_Y = false;

    static int plan_layout(const char* who, const Plan* plan, CLayout& L, bool) {
        DVAE_CHECK_ARG(plan, "%s: null plan", who);
        DVAE_CHECK_ARG(plan->precision == DVAE_PREC_F32 && dims_ok(plan->h1, plan->h2, plan->y_dim) && plan->B >= 1, "%s: not a plan of dvae_train_clf_plan", who);
        L = make_layout(plan->h1, plan->h2, plan->y_dim, plan->B, plan->ksplit);
        DVAE_CHECK_ARG(L.ws_bytes == plan->workspace_bytes && L.nslices == plan->ksplit && L.n_params == plan->n_params &&
                       L.slice_frames == plan->slice_frames, "%s: the plan was changed after dvae_train_clf_plan", who);
        return 0;
    }

    static int check_inputs(const char* who, const Plan* plan, const void* ws, const StepInputs& in) {
        DVAE_CHECK_ARG(ws && in.x && in.y, "%s: null pointer", who);
        DVAE_CHECK_ARG(in.ldx >= GX && in.ldx < ((int64_t)1 << 20), "%s: leading dimension of x %lld (at least 513)", who, (long long)in.ldx);
        DVAE_CHECK_ARG(in.ldy >= plan->y_dim && in.ldy < ((int64_t)1 << 20), "%s: leading dimension of y %lld for y_dim %d", who, (long long)in.ldy,
                       plan->y_dim);
        DVAE_CHECK_ARG(!plan->row_index || plan->row_count >= 1, "%s: a gather table needs row_count >= 1 (got %lld)", who, (long long)plan->row_count);
        return 0;
    }

    static int launch_rows(const Plan* plan, const CLayout& L, char* ws, const StepInputs& in, bool fwd_only, hipStream_t s) {
        static bool attr_done[64] = {};
        if (int rc = raise_lds_limit((const void*)train_clf_rows_kernel, "train_clf_rows_kernel", L.lds_bytes, attr_done)) return rc;
        CRowsArgs g;
        memset(&g, 0, sizeof(g));
        g.x = in.x; g.ldx = in.ldx; g.y = in.y; g.ldy = in.ldy;
        g.row_index = (const int64_t*)(uintptr_t)plan->row_index; g.row_count = plan->row_count; g.bad = (int*)(uintptr_t)plan->bad_row_counter;
        g.ws = (float*)ws; g.stash = (float*)(ws + L.o_stash); g.partials = (double*)(ws + L.o_partials); g.counts = (long long*)(ws + L.o_counts);
        g.bce_eps = in.loss_eps; g.invB = (float)(1.0 / (double)L.B); g.fwd_only = fwd_only ? 1 : 0;
        hipLaunchKernelGGL(train_clf_rows_kernel, dim3((unsigned)L.rows_grid), dim3(256), (size_t)L.lds_bytes, s, L, g);
        DVAE_LAUNCH_OK("train_clf_rows_kernel");
        return 0;
    }

    static void tensors(const CLayout& L, GTensor* T) { make_tensors(L, T); }
    static void gemms(const CLayout& L, GGemm* G) { make_gemms(L, G); }
    static size_t partials_bytes(const CLayout& L) { return (size_t)(L.o_stash - L.o_partials); }      // loss and count partials
    static void extend_apply_args(const Plan*, const CLayout&, ApplyArgs&) {}
    // a finalising launch sums the confusion counts too
    static void extend_table(const Plan* plan, const CLayout& L, char* ws, long long* counts4, GApplyArgs& g) {
        if (!g.finalize) return;
        g.cnt_partials = (const long long*)(ws + L.o_counts); g.cnt_wgs = (int)L.rows_grid; g.counts4 = counts4;
        g.cnt_accum = (long long*)(uintptr_t)plan->count_accum;
    }
};

}  // namespace tc
}  // namespace dvae

using namespace dvae;
using namespace dvae::tc;

extern "C" int dvae_train_clf_plan(int h1, int h2, int y_dim, int precision, int64_t B, int ksplit_hint, dvae_train_clf_plan_t* plan) {
    DVAE_CHECK_ARG(plan, "train_clf_plan: null plan");
    if (precision != DVAE_PREC_F32) {
        set_error("train_clf_plan: operand policy %d; %s", precision, LIMITS);
        return DVAE_E_UNSUPPORTED;
    }
    if (!dims_ok(h1, h2, y_dim)) {
        set_error("train_clf_plan: hidden %d / %d, y_dim %d; %s", h1, h2, y_dim, LIMITS);
        return DVAE_E_UNSUPPORTED;
    }
    DVAE_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 31), "train_clf_plan: %lld frames", (long long)B);
    DVAE_CHECK_ARG(ksplit_hint >= 0 && ksplit_hint <= G_MAX_SLICES, "train_clf_plan: %d frame slices (0 = choose, at most %d)", ksplit_hint, G_MAX_SLICES);
    const CLayout L = make_layout(h1, h2, y_dim, B, ksplit_hint);
    memset(plan, 0, sizeof(*plan));
    plan->h1 = h1; plan->h2 = h2; plan->y_dim = y_dim; plan->precision = precision;
    plan->ksplit = L.nslices; plan->n_tensors = C_NT; plan->B = B; plan->n_params = L.n_params;
    for (int t = 0; t < C_NT; ++t) { plan->tensor_offset[t] = L.toff[t]; plan->tensor_rows[t] = L.trows[t]; plan->tensor_cols[t] = L.tcols[t]; }
    plan->workspace_bytes = L.ws_bytes; plan->grad_offset_bytes = L.o_grads; plan->Bp = L.Bp; plan->rows_grid = L.rows_grid;
    plan->slice_frames = L.slice_frames; plan->wgrad_items = L.n_items; plan->lds_bytes = L.lds_bytes;
    return 0;
}

// the entry points: train_step_host.hpp under this step's description (no noise: eps null; the loss's eps is bce_eps)
extern "C" int dvae_train_clf_repack(const dvae_train_clf_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_repack<CStep>("train_clf_repack", plan, params, ws, stream);
}

extern "C" int dvae_train_clf_init(const dvae_train_clf_plan_t* plan, const float* params, void* ws, void* stream) {
    return step_init<CStep>("train_clf_init", plan, params, ws, stream);
}

extern "C" int dvae_train_clf_grads(const dvae_train_clf_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                    float bce_eps, void* stream) {
    return step_grads<CStep>("train_clf_grads", plan, ws, {x, ldx, y, ldy, nullptr, bce_eps}, stream);
}

extern "C" int dvae_train_clf_apply(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr,
                                    double beta1, double beta2, double adam_eps, double grad_scale, float* losses3, int64_t* counts4, void* stream) {
    return step_apply<CStep>("train_clf_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, {losses3, (long long*)counts4}, stream);
}

extern "C" int dvae_train_clf_reduce(const dvae_train_clf_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses3,
                                     int64_t* counts4, void* stream) {
    return step_reduce<CStep>("train_clf_reduce", plan, ws, flat, accumulate, weight, {losses3, (long long*)counts4}, stream);
}

extern "C" int dvae_train_clf_apply_flat(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step,
                                         double lr, double beta1, double beta2, double adam_eps, double grad_scale, void* stream) {
    return step_apply_flat<CStep>("train_clf_apply_flat", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, nullptr, stream);
}

extern "C" int dvae_train_clf_apply_flat_clipped(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat,
                                                 int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale,
                                                 double max_norm, void* scratch, float* norm2_out, int32_t* skipped_counter, void* stream) {
    const GClipHost clip = {grad_scale, max_norm, scratch, norm2_out, skipped_counter};
    return step_apply_flat<CStep>("train_clf_apply_flat_clipped", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, grad_scale}, ws, flat, &clip,
                                  stream);
}

extern "C" int dvae_train_clf_step(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                                   const float* y, int64_t ldy, float bce_eps, int step, double lr, double beta1, double beta2, double adam_eps,
                                   float* losses3, int64_t* counts4, void* stream) {
    return step_step<CStep>("train_clf_step", "train_clf_grads", "train_clf_apply", plan, {params, m, v, step, lr, beta1, beta2, adam_eps, 1.0}, ws,
                            {x, ldx, y, ldy, nullptr, bce_eps}, {losses3, (long long*)counts4}, stream);
}

extern "C" int dvae_train_clf_eval(const dvae_train_clf_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                                   float bce_eps, float* losses3, int64_t* counts4, void* stream) {
    return step_eval<CStep>("train_clf_eval", plan, ws, {x, ldx, y, ldy, nullptr, bce_eps}, {losses3, (long long*)counts4}, stream);
}


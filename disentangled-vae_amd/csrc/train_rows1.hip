// rows kernel, first generation, of the fused train step for the reference geometry (x 513, h [128,128], z 16, y 0/1/513): see
// include/dvae_train.h for the three-launch structure and train_fused.hip for the host side.
//
// One 256-thread workgroup = 4 waves per 32-frame tile.  Every layer is computed
// TRANSPOSED: out^T[features x frames] = W[features x K] * in^T[K x frames] on 32x32 MFMA tiles, so
//   * the A operand is the weight matrix in its natural nn.Linear [out][in] order: each lane reads
//     16 contiguous bytes of one weight row straight from L2 into VGPRs (a weight element is used
//     by exactly one wave of the workgroup, so staging it in LDS would buy nothing);
//   * the B operand is the previous layer's activations, kept in LDS as [frame][feature] rows whose
//     stride is an odd number of 16-byte slots (conflict-free ds_read_b128);
//   * in the C tile the lane is the frame and the 16 registers are features, so the tanh / exp /
//     loss epilogues, the [frame][feature] LDS write for the next layer and the coalesced
//     [feature][frame] stash store for the weight-gradient kernel all come out without shuffles;
//   * the four waves split the output features; fp32 copies of the tanh outputs stay in registers
//     for the backward pass of the same tile.
// Two operand policies share the code: exact fp32 (v_mfma_f32_32x32x2_f32, parity mode) and bf16
// operands with fp32 accumulation (v_mfma_f32_32x32x16_bf16, throughput mode).
//
// Also here: noise_kernel, which writes out the reparametrisation noise this path draws in the kernel (dvae_train_noise).
#include <math.h>
#include "fused_tiles.hpp"
#include "rows_common.hpp"
#include "../../include/dvae_train.h"

namespace dvae {
namespace fused {


// x[32 frames][f0 .. f0+127] (fp32) for the loss epilogue: 16 coalesced dwords per thread, addresses clamped
template <typename RowOf>
__device__ __forceinline__ void xt_issue(const float* __restrict__ x, int ldx, RowOf rowof, int f0, float (&xr)[16], int tid) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx >> 7, col = idx & 127;
        int cg = f0 + col; cg = cg < XD ? cg : XD - 1;
        xr[i] = x[rowof(row) * ldx + cg];          // rowof clamps rows past the batch
    }
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void xt_commit(const float (&xr)[16], float* Xt, int ldxt, int64_t b0, int64_t B, int f0, int tid) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx >> 7, col = idx & 127;
        Xt[row * ldxt + col] = (f0 + col < XD && b0 + row < B) ? xr[i] : 0.f;
    }
}

// "Classifier" (packages/models/models.py:41-63): 128-128-1 relu / relu / sigmoid MLP on the current tile, its
// binary_cross_entropy against the frame label (utils.py:55-56) and the unit-scale backward, all on chip.
// Used twice by M2_info (scripts/training_M2_info_vad.py:159-183): classifier on x, auxiliary net on z.
// Each wave owns 32 hidden features; the 1-wide output layer is a VALU dot product reduced through LDS.
struct SideArgs {
    WRef W1, W2, W2t, W1t;          // W1t only when the gradient wrt the input is needed
    unsigned s1, s1t;               // k-step strides of W1 / W1t
    const float *b1, *b2, *w3;      // LDS tables
    float b3;
    float y, invB, eps;
    bool live, need_dx;
    float scale;                    // factor applied to the stashed pre-activation gradients (loss weight)
    void *h1T, *h2T, *d1T, *d2T, *d3T;
    int64_t Bp, b0, spl;
};

template <typename P, int K1STEPS>
__device__ __forceinline__ void side_mlp(__amdgpu_buffer_rsrc_t wrs, const SideArgs& a, const typename P::T* in_row,
                                         typename P::T* Ha, typename P::T* Hb, float* redbuf, int wave, int l31, int h,
                                         unsigned S4, float& bce_frame, float& p_out, f32x16& dx) {
    typedef typename P::T T;
    constexpr int E = P::E, KS = P::KSTEP, LDH = Ld<T>::hh;
    const int fb = 32 * wave;
    const T* const Har = Ha + l31 * LDH + h * E;
    const T* const Hbr = Hb + l31 * LDH + h * E;
    f32x16 acc;
    float bv[16], w3v[16], c1r[16], c2r[16], dv[16];
    // layer 1
    WPre<P, K1STEPS> w1;
    wprefetch<P, K1STEPS>(w1, wrs, a.W1, a.s1);
    zero_acc<P>(acc);
    gemm_block<P, K1STEPS>(acc, w1, wrs, a.W1, in_row, a.s1);
    WPre<P, HD / KS, P::PRE128> w2;
    wprefetch<P, HD / KS>(w2, wrs, a.W2, S4);
    bias16(a.b1, fb, h, bv);
#pragma unroll
    for (int r = 0; r < 16; ++r) c1r[r] = fmaxf(acc[r] + bv[r], 0.f);
    put_lds<P>(c1r, Ha, LDH, fb, l31, h);
    __syncthreads();
    // layer 2 + output dot product
    zero_acc<P>(acc);
    gemm_block<P, HD / KS>(acc, w2, wrs, a.W2, Har, S4, [&]() { stash_tile<P>(Ha, LDH, fb, (T*)a.h1T + (int64_t)wave * 32 * a.Bp, a.spl, a.b0, l31, h); });
    WPre<P, HD / KS, P::PRE128> w2t;
    wprefetch<P, HD / KS>(w2t, wrs, a.W2t, S4);
    bias16(a.b2, fb, h, bv);
    bias16(a.w3, fb, h, w3v);
    float pd = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c2r[r] = fmaxf(acc[r] + bv[r], 0.f); pd = fmaf(w3v[r], c2r[r], pd); }
    put_lds<P>(c2r, Hb, LDH, fb, l31, h);
    pd += __shfl_xor(pd, 32, 64);
    if (h == 0) redbuf[wave * 32 + l31] = pd;
    __syncthreads();
    const float logit = redbuf[l31] + redbuf[32 + l31] + redbuf[64 + l31] + redbuf[96 + l31] + a.b3;
    const float p = 1.f / (1.f + P::exp_(-logit));
    p_out = p;
    const float lp = P::log_(p + a.eps), lq = P::log_(1.f - p + a.eps);
    bce_frame = a.live ? -(a.y * lp + (1.f - a.y) * lq) : 0.f;                              // utils.py:55-56, this frame's term
    const float u = a.live ? -a.invB * (a.y / (p + a.eps) - (1.f - a.y) / (1.f - p + a.eps)) : 0.f;   // d BCE / d p
    const float dpre3 = u * p * (1.f - p);
    stash_tile<P>(Hb, LDH, fb, (T*)a.h2T + (int64_t)wave * 32 * a.Bp, a.spl, a.b0, l31, h);
    if (wave == 0 && h == 0) {       // output pre-activation gradient: feature row 0 of a 32-row stash tile
        T* d3 = (T*)a.d3T + (a.b0 / KS) * (64 * E) + (l31 / E) * 32 * E + (l31 % E);
        const T d3h = P::cvt(dpre3 * a.scale);
        *d3 = d3h;
        if constexpr (P::NP == 2) d3[a.spl] = P::cvt(dpre3 * a.scale - (float)d3h);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dv[r] = c2r[r] > 0.f ? w3v[r] * dpre3 : 0.f;            // dpre2 (unit scale)
    put_lds<P>(dv, Ha, LDH, fb, l31, h);
    __syncthreads();
    // backward through layer 2
    zero_acc<P>(acc);
    gemm_block<P, HD / KS>(acc, w2t, wrs, a.W2t, Har, S4, [&]() { stash_tile<P>(Ha, LDH, fb, (T*)a.d2T + (int64_t)wave * 32 * a.Bp, a.spl, a.b0, l31, h, a.scale); });
    WPre<P, HD / KS> w1t;
    if (a.need_dx && wave == 0) wprefetch<P, HD / KS>(w1t, wrs, a.W1t, a.s1t);
#pragma unroll
    for (int r = 0; r < 16; ++r) dv[r] = c1r[r] > 0.f ? acc[r] : 0.f;                      // dpre1 (unit scale)
    put_lds<P>(dv, Hb, LDH, fb, l31, h);
    __syncthreads();
    zero_acc<P>(dx);
    if (a.need_dx && wave == 0) {
        gemm_block<P, HD / KS>(dx, w1t, wrs, a.W1t, Hbr, a.s1t, [&]() { stash_tile<P>(Hb, LDH, fb, (T*)a.d1T + (int64_t)wave * 32 * a.Bp, a.spl, a.b0, l31, h, a.scale); });
    } else {
        stash_tile<P>(Hb, LDH, fb, (T*)a.d1T + (int64_t)wave * 32 * a.Bp, a.spl, a.b0, l31, h, a.scale);
    }
    __syncthreads();
}

template <typename P, int YP, bool YENC, bool INFO>
__global__ __launch_bounds__(256, 1) void vae_rows_kernel(const RowsArgs g) {
    typedef typename P::T T;
    constexpr int E = P::E;
    constexpr int KS = P::KSTEP;
    constexpr int LDU = Ld<T>::u, LDH = Ld<T>::hh, LDZ = Ld<T>::z, LDX = Ld<T>::xt;
    constexpr int LD1 = XP + (YENC ? YP : 0);           // W1 shadow row length
    constexpr int LD3 = ZD + YP;                        // W3 shadow row length
    constexpr bool Y513 = (YP == XP);                   // IBM labels: y has the same 513-column shape as x
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* U = reinterpret_cast<T*>(smem);
    T* Ha = U + TB * LDU;
    T* Hb = Ha + TB * LDH;
    T* Zb = Hb + TB * LDH;
    float* Xt = reinterpret_cast<float*>(U + P::NP * Ld<T>::act_elems);     // behind the operand plane(s).  XFULL: dense [32][513] fp32 x tile; else [32][129] slice
    float* Bias = Xt + (P::XFULL ? Ld<T>::xf_floats : Ld<T>::xt_floats);
    constexpr int OB1 = 0, OB2 = HD, OBMV = 2 * HD, OB3 = 2 * HD + 32, OB4 = 3 * HD + 32, OB5 = 4 * HD + 32;
    // M2_info tables behind the VAE biases: bc1 bc2 wc3 ba1 ba2 wa3 (128 each), then bc3, ba3
    constexpr int OI = Ld<T>::nbias, OBC1 = OI, OBC2 = OI + HD, OWC3 = OI + 2 * HD, OBA1 = OI + 3 * HD, OBA2 = OI + 4 * HD, OWA3 = OI + 5 * HD, OS3 = OI + 6 * HD;
    __shared__ float red[16];
    __shared__ float red2[128];
    __shared__ int64_t rowsrc[TB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int fb = 32 * wave;                           // this wave's feature block in 128-wide layers
    // fragment-major weight copies: [k-step][row tile][lane][E] (k-step major: the fragments a wave keeps in
    // flight then sit >= 4 KB apart and spread over the L2 channels); this wave's tile = wave in 128-row layers
    constexpr int FB = 64 * E;                          // elements per (tile, k-step) block
    // weight copies through ONE buffer descriptor: per-lane byte offset + wave-uniform (matrix, tile) offset
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.wcopy), 0, (int)g.wcopy_bytes, 0x00020000);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    constexpr unsigned SZ = sizeof(T);
    auto wbase = [&](const void* Wp, int tile, int ld) -> WRef {
        const unsigned m = (unsigned)((const char*)Wp - (const char*)g.wcopy);
        if (WFRAG) return WRef{lane * 16, m + (unsigned)tile * (FB * SZ), g.wpl_bytes};
        return WRef{(int)((l31 * ld + h * E) * SZ), m + (unsigned)(32 * tile * ld) * SZ, g.wpl_bytes};
    };
    // byte strides between k-steps (4-tile, 1-tile and 17-tile matrices), between row tiles of W5s, and the
    // byte offsets of the y k-blocks inside W1 / W3
    constexpr unsigned S4 = (WFRAG ? 4 * FB : 2 * E) * SZ, S1 = (WFRAG ? FB : 2 * E) * SZ, S17 = (WFRAG ? NT_OUT * FB : 2 * E) * SZ;
    constexpr unsigned TSTEP = (WFRAG ? FB : 32 * HD) * SZ;
    constexpr unsigned KB1 = (WFRAG ? (XP / KS) * 4 * FB : XP) * SZ;
    constexpr unsigned KB3 = (WFRAG ? (ZD / KS) * 4 * FB : ZD) * SZ;
    const WRef W1r = wbase(g.W1s, wave_u, LD1);
    const WRef W2r = wbase(g.W2s, wave_u, HD);
    const WRef Wmvr = wbase(g.Wmvs, 0, HD);
    const WRef W3r = wbase(g.W3s, wave_u, LD3);
    const WRef W4r = wbase(g.W4s, wave_u, HD);
    const WRef W5s = wbase(g.W5s, 0, HD);
    const WRef W5tr = wbase(g.W5t, wave_u, NO);
    const WRef W4tr = wbase(g.W4t, wave_u, HD);
    const WRef W3ztr = wbase(g.W3zt, 0, HD);
    const WRef Wmvtr = wbase(g.Wmvt, wave_u, 32);
    const WRef W2tr = wbase(g.W2t, wave_u, HD);
    auto woff = [](WRef r, unsigned bytes) { return WRef{r.voff, r.soff + bytes, r.pl}; };
    const T* const Ur = U + l31 * LDU + h * E;
    const T* const Har = Ha + l31 * LDH + h * E;
    const T* const Hbr = Hb + l31 * LDH + h * E;
    const T* const Zbr = Zb + l31 * LDZ + h * E;

    double tot_rec = 0.0, tot_kl = 0.0, tot_bc = 0.0, tot_ba = 0.0;

    // fp32 bias table -> LDS once (epilogues must not queue global loads behind the weight prefetch).
    // The loads are issued here (clamped addresses instead of branches); the LDS stores wait until the first
    // tile's x loads are in flight, so the kernel's first HBM round trip carries both.
    constexpr int NB = (Ld<T>::nbias + 255) / 256;
    float bvv[NB];
#pragma unroll
    for (int it = 0; it < NB; ++it) {
        int i = tid + 256 * it;
        i = i < Ld<T>::nbias ? i : Ld<T>::nbias - 1;
        const float* src;
        int k;
        if (i < OB2) { src = g.b1; k = i; }
        else if (i < OBMV) { src = g.b2; k = i - OB2; }
        else if (i < OBMV + ZD) { src = g.bmu; k = i - OBMV; }
        else if (i < OB3) { src = g.blv; k = i - OBMV - ZD; }
        else if (i < OB4) { src = g.b3; k = i - OB3; }
        else if (i < OB5) { src = g.b4; k = i - OB4; }
        else if (i < OB5 + NO) { src = g.b5; k = i - OB5; k = k < XD ? k : XD - 1; }
        else { src = g.w5last; k = i - OB5 - NO; }
        bvv[it] = src[k];
    }
    auto store_bias_table = [&]() {
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int i = tid + 256 * it;
            if (i < Ld<T>::nbias) Bias[i] = (i >= OB5 + XD && i < OB5 + NO) ? 0.f : bvv[it];
        }
        if (INFO) {
            for (int i = tid; i < 6 * HD + 2; i += 256) {
                float v;
                const int q = i / HD, k = i - q * HD;
                if (q == 0) v = g.bc1[k]; else if (q == 1) v = g.bc2[k]; else if (q == 2) v = g.wc3[k];
                else if (q == 3) v = g.ba1[k]; else if (q == 4) v = g.ba2[k]; else if (q == 5) v = g.wa3[k];
                else v = k == 0 ? g.bc3[0] : g.ba3[0];
                Bias[OI + i] = v;
            }
        }
    };
    bool bias_pending = true;

    for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * TB;
        const bool live = (b0 + l31) < g.B;             // this lane's frame exists
        const bool full = (b0 + TB) <= g.B;
        float rec_lane = 0.f, kl_lane = 0.f, bce_c = 0.f, bce_a = 0.f;
        float y_l = 0.f;
        // source row of the tile's frame r (clamped to the batch): identity, or through the gather table
        if (g.rows != nullptr) {
            __syncthreads();                                 // previous tile's readers are done with rowsrc
            if (tid < TB) {
                const int64_t bf = b0 + tid;
                const int64_t br = bf < g.B ? bf : g.B - 1;
                int64_t rr = g.rows[br];
                if (rr < 0 || rr >= g.n_rows) { rr = 0; if (g.bad_rows && bf < g.B) atomicAdd(g.bad_rows, 1); }   // never dereference an out-of-range index
                rowsrc[tid] = rr;
            }
            __syncthreads();
        }
        auto rowof = [&](int r) -> int64_t {
            if (g.rows != nullptr) return rowsrc[r];
            const int64_t br = b0 + r;
            return br < g.B ? br : g.B - 1;
        };
        if (INFO) y_l = g.y[rowof(l31) * g.ldy];
        f32x16 dzu;                                      // M2_info: d BCE_aux / d z (unit scale), wave 0
        // per-iteration opaque copy of the thread id: stops the compiler from hoisting the ~70 per-thread
        // staging addresses out of the tile loop (they would live across the whole loop and spill)
        int tl = tid;
        asm volatile("" : "+v"(tl));

        DVAE_STAMP(0);
        if (g.dbg && tid == 0) g.dbg[(size_t)blockIdx.x * 32 + 30] = clock64();
        // reparametrisation noise of this lane's frame (wave 0 owns the latent tile): requested first,
        // long before it is needed
        float ep_r[8];
        if (wave == 0) {
            int64_t br = b0 + l31; br = br < g.B ? br : g.B - 1;
            if (g.eps != nullptr) {
                const f32x4 e0 = *reinterpret_cast<const f32x4*>(g.eps + br * ZD + 4 * h);
                const f32x4 e1 = *reinterpret_cast<const f32x4*>(g.eps + br * ZD + 8 + 4 * h);
#pragma unroll
                for (int jq = 0; jq < 4; ++jq) { ep_r[jq] = live ? e0[jq] : 0.f; ep_r[4 + jq] = live ? e1[jq] : 0.f; }
            } else {                                             // drawn here: no noise tensor, no extra launch
                frame_noise8(g.rng_seed, (unsigned long long)br, g.rng_step, h, ep_r);
#pragma unroll
                for (int jq = 0; jq < 8; ++jq) ep_r[jq] = live ? ep_r[jq] : 0.f;
            }
        }
        // ---------------- encoder layer 1: [x | y] -> h1 ----------------
        WPre<P, XP / KS> w1x;
        wprefetch<P, XP / KS>(w1x, wrs, W1r, S4);
        const bool yfast = Y513 && g.fasty && full;
        f32x4 yv[NQ513];
        if (g.fastx && full) {
            f32x4 xv[NQ513];
            tile513_issue(g.x, rowof, xv, tl);
            if constexpr (Y513 && P::EARLY_Y) {
                if (yfast) tile513_issue(g.y, rowof, yv, tl);      // y tile in flight under the x commit and the x GEMM
            }
            if (bias_pending) { store_bias_table(); bias_pending = false; }
            tile513_commit<P, XP>(xv, U, LDU, tl, P::XFULL ? Xt : nullptr);
        } else {
            if (bias_pending) { store_bias_table(); bias_pending = false; }
            load_rows_to_lds<P>(g.x, g.ldx, XD, XP, b0, g.B, U, LDU, tl, rowof, P::XFULL ? Xt : nullptr);
            if constexpr (Y513 && P::EARLY_Y) {
                if (yfast) tile513_issue(g.y, rowof, yv, tl);
            }
        }
        __syncthreads();
        DVAE_STAMP(1);
        f32x16 acc;
        zero_acc<P>(acc);
        gemm_block<P, XP / KS>(acc, w1x, wrs, W1r, Ur, S4, [&]() {
            if (!(g.ablate & 2)) stash_from_lds<P>(U, LDU, XP, NO, (T*)g.xT, g.spl, g.Bp, b0, tl);
        });
        DVAE_STAMP(2);
        if (INFO) {
            const f32x16 acc_keep = acc;
            SideArgs sa;
            sa.W1 = wbase(g.Wc1s, wave_u, XP); sa.W2 = wbase(g.Wc2s, wave_u, HD); sa.W2t = wbase(g.Wc2t, wave_u, HD); sa.W1t = sa.W2t;
            sa.s1 = S4; sa.s1t = S4; sa.b1 = Bias + OBC1; sa.b2 = Bias + OBC2; sa.w3 = Bias + OWC3; sa.b3 = Bias[OS3];
            sa.y = y_l; sa.invB = g.invB; sa.eps = g.elbo_eps; sa.live = live; sa.need_dx = false; sa.scale = g.alpha;
            sa.h1T = g.c1T; sa.h2T = g.c2T; sa.d1T = g.dc1T; sa.d2T = g.dc2T; sa.d3T = g.dc3T; sa.Bp = g.Bp; sa.b0 = b0; sa.spl = g.spl;
            float pc; f32x16 dxc;
            side_mlp<P, XP / KS>(wrs, sa, Ur, Ha, Hb, red2, wave, l31, h, S4, bce_c, pc, dxc);
            acc = acc_keep;
        }
        WPre<P, HD / KS, P::PRE128> w2;
        WPre<P, (YENC ? YP : 0) / KS> w1y;
        if (YENC) wprefetch<P, (YENC ? YP : 0) / KS>(w1y, wrs, woff(W1r, KB1), S4);
        else wprefetch<P, HD / KS>(w2, wrs, W2r, S4);
        if (YP > 0) {
            __syncthreads();
            if (Y513 && yfast) {
                if constexpr (!P::EARLY_Y) tile513_issue(g.y, rowof, yv, tl);
                tile513_commit<P, XP>(yv, U, LDU, tl);
            } else {
                load_rows_to_lds<P>(g.y, g.ldy, g.ydim, YP, b0, g.B, U, LDU, tl, rowof);
            }
            __syncthreads();
            if (YENC) {
                gemm_block<P, (YENC ? YP : 0) / KS>(acc, w1y, wrs, woff(W1r, KB1), Ur, S4, [&]() {
                    if (!(g.ablate & 2)) stash_from_lds<P>(U, LDU, YP, (YP + 31) / 32 * 32, (T*)g.yT, g.spl, g.Bp, b0, tl);
                });
                wprefetch<P, HD / KS>(w2, wrs, W2r, S4);
            } else {
                if (!(g.ablate & 2)) stash_from_lds<P>(U, LDU, YP, (YP + 31) / 32 * 32, (T*)g.yT, g.spl, g.Bp, b0, tl);
            }
        }
        float h1r[16], bv[16];
        DVAE_STAMP(3);
        bias16(Bias + OB1, fb, h, bv);
#pragma unroll
        for (int r = 0; r < 16; ++r) h1r[r] = P::tanh_(acc[r] + bv[r]);
        put_lds<P>(h1r, Ha, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(4);
        // ---------------- encoder layer 2 ----------------
        zero_acc<P>(acc);
        gemm_block<P, HD / KS>(acc, w2, wrs, W2r, Har, S4, [&]() { DVAE_FSTAMP(16); stash_tile<P>(Ha, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.h1T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); DVAE_FSTAMP(17); });
        DVAE_FSTAMP(18);
        WPre<P, HD / KS, P::PRE128> wmv;
        WPre<P, ZD / KS> w3z;
        if (wave == 0) wprefetch<P, HD / KS>(wmv, wrs, Wmvr, S1);
        wprefetch<P, ZD / KS>(w3z, wrs, W3r, S4);
        float h2r[16];
        bias16(Bias + OB2, fb, h, bv);
#pragma unroll
        for (int r = 0; r < 16; ++r) h2r[r] = P::tanh_(acc[r] + bv[r]);
        DVAE_FSTAMP(19);
        put_lds<P>(h2r, Hb, LDH, fb, l31, h);
        DVAE_FSTAMP(20);
        __syncthreads();

        DVAE_STAMP(5);
        // ---------------- heads + reparametrisation (wave 0): rows 0-15 mu, 16-31 log_var ----------------
        float mu_r[8], lv_r[8], sd_r[8];
        // the label block of decoder layer 1 (33 k-steps) does not depend on z: its first fragments are requested here,
        // a whole phase ahead (three of the four waves idle through the heads anyway)
        WPre<P, (YP > 0 ? YP : KS) / KS, P::PREBIG> w3y;
        if (YP > 0) wprefetch<P, (YP > 0 ? YP : KS) / KS>(w3y, wrs, woff(W3r, KB3), S4);
        if (wave == 0) {
            zero_acc<P>(acc);
            gemm_block<P, HD / KS>(acc, wmv, wrs, Wmvr, Hbr, S1, [&]() { stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.h2T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
            float zv[16];
            bias16(Bias + OBMV, 0, h, bv);                          // rows 0-15 bmu, 16-31 blv
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                mu_r[r] = acc[r] + bv[r];
                lv_r[r] = acc[r + 8] + bv[r + 8];
                sd_r[r] = P::exp_(0.5f * lv_r[r]);                 // models.py:17
                zv[r] = fmaf(sd_r[r], ep_r[r], mu_r[r]);           // models.py:20
                zv[r + 8] = 0.f;
                if (live) kl_lane += lv_r[r] - mu_r[r] * mu_r[r] - P::exp_(lv_r[r]);   // utils.py:75
            }
            // z block of the decoder input: features 0..15 valid, 16..31 zero
            put_lds<P>(zv, Zb, LDZ, 0, l31, h);
        } else {
            stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.h2T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h);
        }
        __syncthreads();

        DVAE_STAMP(6);
        if (INFO) {
            SideArgs sa;
            sa.W1 = wbase(g.Wa1s, wave_u, ZD); sa.W2 = wbase(g.Wa2s, wave_u, HD); sa.W2t = wbase(g.Wa2t, wave_u, HD); sa.W1t = wbase(g.Wa1t, 0, HD);
            sa.s1 = S4; sa.s1t = S1; sa.b1 = Bias + OBA1; sa.b2 = Bias + OBA2; sa.w3 = Bias + OWA3; sa.b3 = Bias[OS3 + 1];
            sa.y = y_l; sa.invB = g.invB; sa.eps = g.elbo_eps; sa.live = live; sa.need_dx = true; sa.scale = g.gamma - g.beta;
            sa.h1T = g.a1T; sa.h2T = g.a2T; sa.d1T = g.da1T; sa.d2T = g.da2T; sa.d3T = g.da3T; sa.Bp = g.Bp; sa.b0 = b0; sa.spl = g.spl;
            float pa;
            if (wave == 0) stash_tile<P>(Zb, LDZ, 0, (T*)g.zT, g.spl, b0, l31, h);
            side_mlp<P, ZD / KS>(wrs, sa, Zbr, Ha, Hb, red2, wave, l31, h, S4, bce_a, pa, dzu);
        }
        // ---------------- decoder layer 1: [z | y] -> d1 ----------------
        zero_acc<P>(acc);
        gemm_block<P, ZD / KS>(acc, w3z, wrs, W3r, Zbr, S4, [&]() { if (!INFO && wave == 0) stash_tile<P>(Zb, LDZ, 0, (T*)g.zT, g.spl, b0, l31, h); });
        WPre<P, HD / KS, P::PRE128> w4;
        if (YP > 0) gemm_block<P, (YP > 0 ? YP : KS) / KS>(acc, w3y, wrs, woff(W3r, KB3), Ur, S4);
        wprefetch<P, HD / KS>(w4, wrs, W4r, S4);
        float d1r[16];
        bias16(Bias + OB3, fb, h, bv);
#pragma unroll
        for (int r = 0; r < 16; ++r) d1r[r] = P::tanh_(acc[r] + bv[r]);
        put_lds<P>(d1r, Ha, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(7);
        // ---------------- decoder layer 2 ----------------
        zero_acc<P>(acc);
        gemm_block<P, HD / KS>(acc, w4, wrs, W4r, Har, S4, [&]() { stash_tile<P>(Ha, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.d1T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
        WPre<P, HD / KS, P::PRE128> w5;
        wprefetch<P, HD / KS>(w5, wrs, woff(W5s, wave_u * TSTEP), S17);
        float xr[16];
        if (!P::XFULL) xt_issue(g.x, g.ldx, rowof, 0, xr, tl);
        float d2r[16];
        bias16(Bias + OB4, fb, h, bv);
#pragma unroll
        for (int r = 0; r < 16; ++r) d2r[r] = P::tanh_(acc[r] + bv[r]);
        put_lds<P>(d2r, Hb, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(8);
        // ---------------- output layer a = W5 d2 + b5, Itakura-Saito terms, da -> U ----------------
        WPre<P, NO / KS> w5t;
        // one 32-feature tile t of the output layer for this wave: GEMM, loss terms, da
        auto out_tile = [&](int t, const float* xsrc, int xld, int xcol0, int xcmax) {
            if (t == 4) DVAE_FSTAMP(21);
            zero_acc<P>(acc);
            const WRef wr = woff(W5s, (unsigned)t * TSTEP);
            gemm_block<P, HD / KS>(acc, w5, wrs, wr, Hbr, S17, [&]() { if (t < 4) stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.d2T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
            if (t == 4) DVAE_FSTAMP(22);
            if (t + 4 < (P::XFULL ? NT_OUT - 1 : NT_OUT)) wprefetch<P, HD / KS>(w5, wrs, woff(wr, 4 * TSTEP), S17);
            else wprefetch<P, NO / KS>(w5t, wrs, W5tr, S4);
            if (t == 4) DVAE_FSTAMP(23);
            float da[16], b5v[16], xs[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {                       // all x reads up front: one LDS wait, not sixteen
                int xc = xcol0 + feat_of(r, h); xc = xc < xcmax ? xc : xcmax;
                xs[r] = xsrc[l31 * xld + xc];
            }
            bias16(Bias + OB5, 32 * t, h, b5v);
            if (t == 4) DVAE_FSTAMP(24);
            const float invB_l = live ? g.invB : 0.f;            // frames past B contribute nothing
            if (t < NT_OUT - 1) {                                // all 32 features of the tile exist
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float a = acc[r] + b5v[r];
                    const float xe = xs[r] * P::exp_(-a);        // x / r,  r = exp(a)  (models.py:122)
                    rec_lane += xe - P::log_(xs[r] + g.elbo_eps) + a - 1.f;   // utils.py:74 (log r = a)
                    da[r] = (1.f - xe) * invB_l;                 // d recon / d a
                }
            } else {                                             // last tile: features >= 513 are padding
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = 32 * t + feat_of(r, h) < XD;
                    const float a = acc[r] + b5v[r];
                    const float xe = xs[r] * P::exp_(-a);
                    const float term = xe - P::log_(xs[r] + g.elbo_eps) + a - 1.f;
                    rec_lane += ok ? term : 0.f;
                    da[r] = ok ? (1.f - xe) * invB_l : 0.f;
                }
            }
            if (t == 4) DVAE_FSTAMP(25);
            put_lds<P>(da, U, LDU, 32 * t, l31, h);
            if (t == 4) DVAE_FSTAMP(26);
        };
        if (P::XFULL) {
            // the fp32 x tile is resident in LDS ([frame][513], odd stride: conflict-free): no barriers here.
            // 16 full tiles = 4 per wave.  The 17th tile holds ONE real feature (bin 512): a whole MFMA tile and
            // epilogue round for it would be a fifth round for wave 0; wave 3 does it as a 128-term dot product instead.
#pragma unroll 1
            for (int t = wave_u; t < NT_OUT - 1; t += 4) out_tile(t, Xt, XD, 32 * t, XD - 1);
            if (wave_u == 3) {
                const float* wl = Bias + OB5 + NO + 64 * h;                 // this half's 64 weights (LDS broadcast reads)
                const T* drow = Hb + l31 * LDH + 64 * h;
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 64 / E; ++c) {
                    const typename P::Frag dv = *reinterpret_cast<const typename P::Frag*>(drow + c * E);
#pragma unroll
                    for (int j = 0; j < E; j += 4) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + c * E + j);
                        s = fmaf((float)dv[j], wv[0], s); s = fmaf((float)dv[j + 1], wv[1], s);
                        s = fmaf((float)dv[j + 2], wv[2], s); s = fmaf((float)dv[j + 3], wv[3], s);
                    }
                }
                s += __shfl_xor(s, 32, 64);
                const float a = s + Bias[OB5 + XD - 1];
                const float xv512 = Xt[l31 * XD + XD - 1];
                const float xe = xv512 * P::exp_(-a);
                if (h == 0) rec_lane += xe - P::log_(xv512 + g.elbo_eps) + a - 1.f;
                const float da512 = live ? (1.f - xe) * g.invB : 0.f;
                // columns 512 .. 543 of this frame's da row: the value, then 31 zeros (16 bf16 = 2 fragments per half)
                typename P::Frag z0, z1;
#pragma unroll
                for (int j = 0; j < E; ++j) { z0[j] = P::cvt(0.f); z1[j] = P::cvt(0.f); }
                if (h == 0) z0[0] = P::cvt(da512);
                T* urow = U + l31 * LDU + (XD - 1) + 16 * h;
                *reinterpret_cast<typename P::Frag*>(urow) = z0;
                *reinterpret_cast<typename P::Frag*>(urow + E) = z1;
            }
            __syncthreads();
        } else {
#pragma unroll 1
            for (int it = 0; it < (NT_OUT + 3) / 4; ++it) {
                xt_commit(xr, Xt, LDX, b0, g.B, 128 * it, tl);
                __syncthreads();
                if (it + 1 < (NT_OUT + 3) / 4) xt_issue(g.x, g.ldx, rowof, 128 * (it + 1), xr, tl);
                const int t = 4 * it + wave_u;
                if (t < NT_OUT) out_tile(t, Xt, LDX, 32 * wave, 127);
                __syncthreads();
            }
        }

        DVAE_STAMP(9);
        // ---------------- backward: d2 <- da ----------------
        zero_acc<P>(acc);
        gemm_block<P, NO / KS>(acc, w5t, wrs, W5tr, Ur, S4, [&]() {
            for (int t = wave; t < NT_OUT; t += 4) stash_tile<P>(U, LDU, 32 * t, (g.ablate & 1) ? nullptr : (T*)g.daT + (int64_t)(t) * 32 * g.Bp, g.spl, b0, l31, h);
        });
        WPre<P, HD / KS, P::PRE128> w4t;
        wprefetch<P, HD / KS>(w4t, wrs, W4tr, S4);
        float dv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = acc[r] * (1.f - d2r[r] * d2r[r]);
        put_lds<P>(dv, Ha, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(10);
        // ---------------- backward: d1 <- dpre_d2 ----------------
        zero_acc<P>(acc);
        gemm_block<P, HD / KS>(acc, w4t, wrs, W4tr, Har, S4, [&]() { stash_tile<P>(Ha, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.dd2T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
        WPre<P, HD / KS, P::PRE128> w3zt;
        WPre<P, 32 / KS> wmvt;
        if (wave == 0) wprefetch<P, HD / KS>(w3zt, wrs, W3ztr, S1);
        wprefetch<P, 32 / KS>(wmvt, wrs, Wmvtr, S4);
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = acc[r] * (1.f - d1r[r] * d1r[r]);
        put_lds<P>(dv, Hb, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(11);
        // ---------------- backward: z <- dpre_d1 (wave 0), then dmu / dlogvar ----------------
        if (wave == 0) {
            zero_acc<P>(acc);
            gemm_block<P, HD / KS>(acc, w3zt, wrs, W3ztr, Hbr, S1, [&]() { stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.dd1T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
            float dml[16];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float dz = INFO ? acc[r] - g.beta * dzu[r] : acc[r];     // enc_loss = ELBO + alpha*clf - beta*BCE(aux(z), y)
                dml[r] = live ? dz + mu_r[r] * g.invB : 0.f;                                                   // dmu
                dml[r + 8] = live ? dz * ep_r[r] * (0.5f * sd_r[r]) - 0.5f * g.invB * (1.f - P::exp_(lv_r[r])) : 0.f;   // dlogvar
            }
            put_lds<P>(dml, Zb, LDZ, 0, l31, h);
        } else {
            stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.dd1T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h);
        }
        __syncthreads();

        DVAE_STAMP(12);
        // ---------------- backward: h2 <- [dmu | dlogvar] ----------------
        zero_acc<P>(acc);
        gemm_block<P, 32 / KS>(acc, wmvt, wrs, Wmvtr, Zbr, S4, [&]() { if (wave == 0) stash_tile<P>(Zb, LDZ, 0, (T*)g.dmlvT, g.spl, b0, l31, h); });
        WPre<P, HD / KS, P::PRE128> w2t;
        wprefetch<P, HD / KS>(w2t, wrs, W2tr, S4);
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = acc[r] * (1.f - h2r[r] * h2r[r]);
        put_lds<P>(dv, Ha, LDH, fb, l31, h);
        __syncthreads();

        DVAE_STAMP(13);
        // ---------------- backward: h1 <- dpre_h2 (inputs are data: stop here) ----------------
        zero_acc<P>(acc);
        gemm_block<P, HD / KS>(acc, w2t, wrs, W2tr, Har, S4, [&]() { stash_tile<P>(Ha, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.dh2T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h); });
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = acc[r] * (1.f - h1r[r] * h1r[r]);
        put_lds<P>(dv, Hb, LDH, fb, l31, h);
        stash_tile<P>(Hb, LDH, fb, (g.ablate & 1) ? nullptr : (T*)g.dh1T + (int64_t)(wave) * 32 * g.Bp, g.spl, b0, l31, h);

        DVAE_STAMP(14);
        // ---------------- per-tile loss sums ----------------
        if (!live) rec_lane = 0.f;
        const float rs = wave_sum(rec_lane), ks = wave_sum(kl_lane);
        if (lane == 0) { red[wave] = rs; red[4 + wave] = ks; }
        if (INFO && wave == 0) {
            const float bcs = wave_sum(h == 0 ? bce_c : 0.f), bas = wave_sum(h == 0 ? bce_a : 0.f);
            if (lane == 0) { red[8] = bcs; red[9] = bas; }
        }
        __syncthreads();
        if (tid == 0) {
            tot_rec += (double)red[0] + (double)red[1] + (double)red[2] + (double)red[3];
            tot_kl += -0.5 * (double)red[4];
            if (INFO) { tot_bc += (double)red[8]; tot_ba += (double)red[9]; }
        }
        __syncthreads();
    }
    DVAE_STAMP(15);
    if (g.dbg && tid == 0) g.dbg[(size_t)blockIdx.x * 32 + 31] = clock64();
    if (tid == 0) {
        g.partials[4 * blockIdx.x] = tot_rec;
        g.partials[4 * blockIdx.x + 1] = tot_kl;
        g.partials[4 * blockIdx.x + 2] = tot_bc;
        g.partials[4 * blockIdx.x + 3] = tot_ba;
    }
}

template <typename P, int YP, bool YENC, bool INFO = false>
static int launch_rows(const RowsArgs& a, int grid, hipStream_t s) {
    const size_t lds = Pl<P>::bytes;
    static bool attr_done[64] = {};                      // per device: the attribute belongs to the device's copy of the code object
    const int dev = current_device();
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)vae_rows_kernel<P, YP, YENC, INFO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute(rows kernel, %zu B LDS): %s", lds, hipGetErrorString(e)); return (int)e; }
        attr_done[dev] = true;
    }
    hipLaunchKernelGGL((vae_rows_kernel<P, YP, YENC, INFO>), dim3(grid), dim3(256), lds, s, a);
    DVAE_LAUNCH_OK("vae_rows_kernel");
    return 0;
}

// model: DVAE_MODEL_M1 / DVAE_MODEL_M2 / DVAE_MODEL_M2_INFO; precision: DVAE_PREC_F32, and the bf16 policies in the diagnostic build
int launch_rows1(int precision, int model, int y_dim, const RowsArgs& a, int grid, hipStream_t s) {
    auto rows4 = [&](auto pol) {      // the 4-wave kernel of one operand policy, in the plan's model variant
        using P = decltype(pol);
        if (model == DVAE_MODEL_M2_INFO) return launch_rows<P, 16, false, true>(a, grid, s);
        if (model != DVAE_MODEL_M2) return launch_rows<P, 0, false>(a, grid, s);
        if (y_dim == 1) return launch_rows<P, 16, true>(a, grid, s);
        return launch_rows<P, 528, true>(a, grid, s);
    };
#ifdef DVAE_DIAG
    return with_policy(precision, rows4);
#else
    if (is_bf(precision)) {
        set_error("train_grads: the 4-wave rows kernel under the bf16 policies exists in the diagnostic build only (build.py --diag)");
        return DVAE_E_UNSUPPORTED;
    }
    return rows4(PolF32{});
#endif
}

// dvae_train_noise: the noise the rows kernels draw for themselves (frame_noise8), written out as a [B][16] tensor
__global__ __launch_bounds__(256) void noise_kernel(unsigned long long seed, unsigned long long step, int64_t B, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one (frame, half) pair per thread
    if (i >= 2 * B) return;
    const int64_t frame = i >> 1; const int h = (int)(i & 1);
    float e[8];
    frame_noise8(seed, (unsigned long long)frame, step, h, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) { out[frame * ZD + 4 * h + j] = e[j]; out[frame * ZD + 8 + 4 * h + j] = e[4 + j]; }
}

int launch_noise(unsigned long long seed, unsigned long long step, int64_t B, float* out, hipStream_t s) {
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, s, seed, step, B, out);
    DVAE_LAUNCH_OK("noise_kernel");
    return 0;
}

}  // namespace fused
}  // namespace dvae

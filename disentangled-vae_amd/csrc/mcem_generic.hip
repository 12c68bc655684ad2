// Metropolis-Hastings chain of the MCEM E-step for a decoder of ANY size with two tanh hidden layers (include/dvae_mcem.h,
// dvae_mcem_plan_dims): [z_dim + y_dim] -> h1 -> h2 -> 513 with z_dim 1..128, h1 / h2 1..512, y_dim 0..513, exact fp32 products.
// The hand-tuned chains (mcem_resident*.hip, mcem.hip) are written for 16 / 128 / 128 and stay the default there; this kernel serves
// every other size, and 16 / 128 / 128 too under a plan made by dvae_mcem_plan_dims.
//
//   * 256 threads own a tile of 16 frames for the whole chain.  Products run on v_mfma_f32_16x16x4_f32: 16 weight rows are the A
//     operand, the tile's 16 frames the B columns; the four waves split a layer's row tiles (wave w: tiles w, w + 4, ...).
//   * Weights are not resident: every pass streams them from a packed copy in fragment order [row tile][k block of 16][lane][4], one
//     16-byte load per lane and four MFMAs (lane l holds row l & 15, inputs 16 b + 4 i + (l >> 4), i = 0..3).  Rows are padded to a
//     multiple of 16 and inputs to a multiple of 16 with zeros, so the loops have runtime trip counts and no tails: a padded hidden
//     unit has zero in-weights and zero bias (tanh 0 = 0) and zero out-weights; a padded output row is computed and dropped.
//   * Activations sit in LDS as [k][16] floats: the B operand of MFMA i of block b is the 64 consecutive floats at (16 b + 4 i) * 16.
//   * The label part of layer 1 (W3[:, z:] y + b3) does not change along a chain: formed once per tile, kept in LDS.
//   * X2 and Vb of the tile are kept in LDS where the activations leave room for them (everything but the largest hidden widths);
//     otherwise they are read from memory in every step.  One code path: a per-lane pointer and a row stride.
//   * The chain keeps, per frame, the current state's likelihood sum and squared norm (the decoder acts frame by frame, so this equals
//     the reference's second decoder pass, as in mcem.hip).  The sum over the 513 bins has a fixed order: every lane adds its bins in
//     ascending order (in double), the 16 lane groups of a frame are added in ascending (wave, quarter) order by one lane per frame,
//     which takes the decision and publishes it through LDS.  Nothing depends on the launch's other frames: a frame's chain gives the
//     same bits alone and as any column of any launch.
//   * The kept samples' variances are a decode pass over Zs behind the chain; the decode job (nit == 0) is that pass alone.
//   * 64-bit indexing throughout.
//   * Not kept: a wave's (tile, block) weight loads as one hand-pipelined stream four deep across tile boundaries -- measured slower
//     (21.7 against 19.4 us per chain step at one utterance, 44.7 against 39.8 at 25; 184 registers against 109): DESIGN section 7.
#include <math.h>
#include <string.h>
#include "mcem_types.hpp"
#include "../../include/dvae_mcem.h"

namespace dvae {
namespace fused {

constexpr int GXD = 513, GNO = 528, GNT_OUT = 33;      // output rows, padded rows, 16-row output tiles
constexpr int GTB = 16;                                 // frames per tile

static inline int up16(int v) { return (v + 15) / 16 * 16; }

// element offsets of the packed copy (floats) and the LDS plan of one launch
struct GenLayout {
    int zp, yp, h1p, h2p;                               // padded sizes (multiples of 16; yp 0 without labels)
    int64_t oW3z, oW3y, oW4, oW5, oB3, oB4, oB5, elems;
    int lds_floats_base;                                // H1, H2, C1, Zcur, Zprop, red, prior, flags
    int lds_floats_xv;                                  // + X2 and Vb of the tile
};

static GenLayout gen_layout(int z, int h1, int h2, int y) {
    GenLayout L;
    L.zp = up16(z); L.yp = y ? up16(y) : 0; L.h1p = up16(h1); L.h2p = up16(h2);
    L.oW3z = 0;
    L.oW3y = L.oW3z + (int64_t)L.h1p * L.zp;
    L.oW4 = L.oW3y + (int64_t)L.h1p * L.yp;
    L.oW5 = L.oW4 + (int64_t)L.h2p * L.h1p;
    L.oB3 = L.oW5 + (int64_t)GNO * L.h2p;
    L.oB4 = L.oB3 + L.h1p;
    L.oB5 = L.oB4 + L.h2p;
    L.elems = L.oB5 + GNO;
    L.lds_floats_base = GTB * (2 * L.h1p + L.h2p + 2 * L.zp) + 2 * 16 * GTB /* red: doubles */ + 16 * GTB + 2 * GTB;
    L.lds_floats_xv = L.lds_floats_base + 2 * GXD * GTB;
    return L;
}

struct GenArgs {
    MhArgs m;
    int zdim, zp, yp, h1p, h2p;
    const float *W3z, *W3y, *W4, *W5, *b3, *b4, *b5;
    int xv_lds;                                         // X2 / Vb of the tile in LDS
};

typedef float g4 __attribute__((ext_vector_type(4)));

// acc += W[row tile t] (16 x 16 kb) * act (16 kb x 16 frames): W in fragment order, act in LDS as [k][16]
__device__ __forceinline__ g4 gen_gemm(g4 acc, const float* __restrict__ wt, int kb, const float* act, int lane) {
    const g4* w = reinterpret_cast<const g4*>(wt) + lane;
    for (int b = 0; b < kb; ++b) {
        const g4 a = w[(int64_t)b * 64];
        const float* bp = act + b * 256 + lane;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bp[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bp[64], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bp[128], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bp[192], acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ float gen_tanh(float v) {
    const float e = __expf(2.f * v);                    // tanh = 1 - 2 / (e^{2v} + 1); saturates cleanly at +-1 (PolF32Deep, mcem.hip)
    return 1.f - __fdividef(2.f, e + 1.f);
}

__global__ __launch_bounds__(256) void mcem_generic_kernel(const GenArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const MhArgs& g = a.m;
    float* H1 = gsm;                                    // [h1p][16]
    float* H2 = H1 + GTB * a.h1p;                       // [h2p][16]
    float* C1 = H2 + GTB * a.h2p;                       // [h1p][16]  label part of layer 1 + b3
    float* Zc = C1 + GTB * a.h1p;                       // [zp][16]   state
    float* Zb = Zc + GTB * a.zp;                        // [zp][16]   proposal (rows >= zdim stay 0)
    double* red = reinterpret_cast<double*>(Zb + GTB * a.zp);      // [16 (wave, quarter)][16 frames]
    float* pri = reinterpret_cast<float*>(red + 16 * GTB);          // [16 (k mod 16)][16 frames]
    int* flag = reinterpret_cast<int*>(pri + 16 * GTB);             // [16 frames] (+ 16 spare)
    float* Xs = reinterpret_cast<float*>(flag + 2 * GTB);           // [513][16], [513][16] when a.xv_lds
    float* Vbs = Xs + GXD * GTB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int kb_z = a.zp >> 4, kb_y = a.yp >> 4, kb_1 = a.h1p >> 4, kb_2 = a.h2p >> 4;
    const int nt1 = a.h1p >> 4, nt2 = a.h2p >> 4;
    const int zdim = a.zdim;
    const int64_t N = g.N;

    for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * GTB;
        const bool live = n0 + col < N;
        const int64_t n = live ? n0 + col : N - 1;      // clamped frame of this lane's column: padding columns repeat the last frame
        const float g_n = g.g ? g.g[n] : 1.f;

        // ---- once per tile: zero the proposal's padding rows, the tile's X2 / Vb, the label part of layer 1 ----
        for (int i = tid; i < GTB * a.zp; i += 256) { Zb[i] = 0.f; Zc[i] = 0.f; }
        if (a.xv_lds && g.nit > 0) {
            for (int i = tid; i < GXD * GTB; i += 256) {
                const int f = i >> 4, c = i & 15;
                const int64_t nn = n0 + c < N ? n0 + c : N - 1;
                Xs[i] = g.X2[(int64_t)f * N + nn];
                Vbs[i] = g.Vb[(int64_t)f * N + nn];
            }
        }
        for (int t = wave; t < nt1; t += 4) {
            g4 acc = {0.f, 0.f, 0.f, 0.f};
            const g4* w = reinterpret_cast<const g4*>(a.W3y + (int64_t)t * kb_y * 256) + lane;
            for (int b = 0; b < kb_y; ++b) {
                const g4 wv = w[(int64_t)b * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 16 * b + 4 * i + quad;
                    const float yv = k < g.ydim ? g.y[(int64_t)k * N + n] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i], yv, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                C1[row * GTB + col] = acc[r] + a.b3[row];
            }
        }
        __syncthreads();

        // one decoder pass over the latents in Zb up to the second hidden layer (H2), all waves
        auto hidden = [&]() {
            for (int t = wave; t < nt1; t += 4) {
                g4 acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = C1[(16 * t + 4 * quad + r) * GTB + col];
                acc = gen_gemm(acc, a.W3z + (int64_t)t * kb_z * 256, kb_z, Zb, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) H1[(16 * t + 4 * quad + r) * GTB + col] = gen_tanh(acc[r]);
            }
            __syncthreads();
            for (int t = wave; t < nt2; t += 4) {
                g4 acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = a.b4[16 * t + 4 * quad + r];
                acc = gen_gemm(acc, a.W4 + (int64_t)t * kb_1 * 256, kb_1, H1, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) H2[(16 * t + 4 * quad + r) * GTB + col] = gen_tanh(acc[r]);
            }
            __syncthreads();
        };
        // output tile t of this wave: pre-activations of bins 16 t + 4 quad + r, frame col
        auto out_tile = [&](int t) {
            g4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = a.b5[16 * t + 4 * quad + r];
            return gen_gemm(acc, a.W5 + (int64_t)t * kb_2 * 256, kb_2, H2, lane);
        };

        if (g.nit > 0) {
            for (int i = tid; i < GTB * zdim; i += 256) {
                const int k = i >> 4, c = i & 15;
                const int64_t nn = n0 + c < N ? n0 + c : N - 1;
                Zc[i] = g.Z0[(int64_t)k * N + nn];
            }
            __syncthreads();
            const float* const xp = a.xv_lds ? Xs + col : g.X2 + n;
            const float* const vp = a.xv_lds ? Vbs + col : g.Vb + n;
            const int64_t xstride = a.xv_lds ? GTB : N;
            double ll_cur = 0.0;                        // lanes tid < 16: the state of frame tid
            float prior_cur = 0.f;
            for (int m = -1; m < g.nit; ++m) {
                // proposal (m = -1: the start itself) and the partial sums of its squared norm, k ascending within each k mod 16
                {
                    const int kq = tid >> 4, c = tid & 15;
                    const int64_t nn = n0 + c < N ? n0 + c : N - 1;
                    float s = 0.f;
                    for (int k = kq; k < zdim; k += 16) {
                        float zv = Zc[k * GTB + c];
                        if (m >= 0) zv = zv + g.sd * g.noise[((int64_t)m * zdim + k) * N + nn];      // mcem.py:244
                        Zb[k * GTB + c] = zv;
                        s += zv * zv;
                    }
                    pri[kq * GTB + c] = s;
                }
                __syncthreads();
                hidden();
                double ll = 0.0;
                for (int t = wave; t < GNT_OUT; t += 4) {
                    const g4 acc = out_tile(t);
                    float s = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * t + 4 * quad + r;
                        const int fc = f < GXD ? f : GXD - 1;
                        const float vx = fmaf(g_n, __expf(acc[r]), vp[fc * xstride]);           // mcem.py:248-249
                        const float term = __logf(vx) + __fdividef(xp[fc * xstride], vx);       // mcem.py:252-253
                        s += f < GXD ? term : 0.f;
                    }
                    ll += (double)s;
                }
                red[(wave * 4 + quad) * GTB + col] = ll;
                __syncthreads();
                if (tid < GTB) {
                    double ll_p = 0.0;
                    float prior_p = 0.f;
#pragma unroll
                    for (int i = 0; i < 16; ++i) { ll_p += red[i * GTB + tid]; prior_p += pri[i * GTB + tid]; }
                    int take = 1;
                    if (m >= 0) {
                        const int64_t nn = n0 + tid < N ? n0 + tid : N - 1;
                        const float acc_prob = (float)(ll_cur - ll_p) + 0.5f * (prior_cur - prior_p);     // mcem.py:252-254
                        take = g.logu[(int64_t)m * N + nn] < acc_prob ? 1 : 0;                             // mcem.py:257
                        if (n0 + tid < N) {
                            if (g.accp) g.accp[(int64_t)m * N + nn] = acc_prob;
                            if (g.accd) g.accd[(int64_t)m * N + nn] = (unsigned char)take;
                        }
                    }
                    if (take) { ll_cur = ll_p; prior_cur = prior_p; }
                    flag[tid] = take;
                }
                __syncthreads();
                if (m >= 0) {
                    for (int i = tid; i < GTB * zdim; i += 256) {
                        if (flag[i & 15]) Zc[i] = Zb[i];
                    }
                    if (m >= g.burnin) {                                                                   // mcem.py:271-273
                        __syncthreads();
                        for (int i = tid; i < GTB * zdim; i += 256) {
                            const int c = i / zdim, k = i - c * zdim;
                            if (n0 + c < N) g.Zs[((n0 + c) * g.R + (m - g.burnin)) * zdim + k] = Zc[k * GTB + c];
                        }
                    }
                }
                __syncthreads();
            }
            if (g.Zlast != nullptr) {
                for (int i = tid; i < GTB * zdim; i += 256) {
                    const int k = i >> 4, c = i & 15;
                    if (n0 + c < N) g.Zlast[(int64_t)k * N + n0 + c] = Zc[i];
                }
            }
        }

        // ---- speech variances of the sampled latents: Vs[r] = decoder([Zs[:, r, :] | y])  (mcem.py:280-290) ----
        if (g.Vs != nullptr) {
            for (int rs = 0; rs < g.R; ++rs) {
                __syncthreads();
                for (int i = tid; i < GTB * zdim; i += 256) {
                    const int c = i / zdim, k = i - c * zdim;
                    const int64_t nn = n0 + c < N ? n0 + c : N - 1;
                    Zb[k * GTB + c] = g.Zs[(nn * g.R + rs) * zdim + k];
                }
                __syncthreads();
                hidden();
                float* const vs_r = g.Vs + (int64_t)rs * GXD * N;
                for (int t = wave; t < GNT_OUT; t += 4) {
                    const g4 acc = out_tile(t);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = 16 * t + 4 * quad + r;
                        if (live && f < GXD) vs_r[(int64_t)f * N + n] = __expf(acc[r]);
                    }
                }
            }
        }
        __syncthreads();
    }
}

// nn.Linear [rows][ld] fp32, columns c0 .. c0 + cols - 1 -> fragment order [row tile][k block][lane][4], zero padded
__global__ void mcem_generic_pack_kernel(const float* __restrict__ src, int rows, int cols, int c0, int ld, float* __restrict__ dst, int nt, int kb) {
    const int64_t total = (int64_t)nt * kb * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i & 3), ln = (int)((i >> 2) & 63);
        const int b = (int)((i >> 8) % kb), t = (int)((i >> 8) / kb);
        const int row = 16 * t + (ln & 15), k = 16 * b + 4 * e + (ln >> 4);
        dst[i] = (row < rows && k < cols) ? src[(int64_t)row * ld + c0 + k] : 0.f;
    }
}

__global__ void mcem_generic_bias_kernel(const float* __restrict__ src, int n, float* __restrict__ dst, int np) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) dst[i] = i < n ? src[i] : 0.f;
}

int64_t generic_weights_bytes(int z, int h1, int h2, int y) {
    return gen_layout(z, h1, h2, y).elems * (int64_t)sizeof(float) + 256;
}

int generic_pack(const dvae_mcem_plan_t* plan, const float* W3, int ld3, const float* b3, const float* W4, int ld4, const float* b4,
                 const float* W5, int ld5, const float* b5, void* weights, hipStream_t s) {
    const int z = plan->z_dim, h1 = plan->h_dim, h2 = plan->h2_dim, y = plan->y_dim;
    const GenLayout L = gen_layout(z, h1, h2, y);
    float* w = (float*)weights;
    auto pack = [&](const float* src, int rows, int cols, int c0, int ld, int64_t off, int rp, int kp) {
        const int64_t total = (int64_t)rp * kp;
        if (total == 0) return;
        hipLaunchKernelGGL(mcem_generic_pack_kernel, dim3((unsigned)((total + 255) / 256 < 512 ? (total + 255) / 256 : 512)), dim3(256), 0, s,
                           src, rows, cols, c0, ld, w + off, rp / 16, kp / 16);
    };
    pack(W3, h1, z, 0, ld3, L.oW3z, L.h1p, L.zp);
    pack(W3, h1, y, z, ld3, L.oW3y, L.h1p, L.yp);
    pack(W4, h2, h1, 0, ld4, L.oW4, L.h2p, L.h1p);
    pack(W5, GXD, h2, 0, ld5, L.oW5, GNO, L.h2p);
    hipLaunchKernelGGL(mcem_generic_bias_kernel, dim3(2), dim3(256), 0, s, b3, h1, w + L.oB3, L.h1p);
    hipLaunchKernelGGL(mcem_generic_bias_kernel, dim3(2), dim3(256), 0, s, b4, h2, w + L.oB4, L.h2p);
    hipLaunchKernelGGL(mcem_generic_bias_kernel, dim3(3), dim3(256), 0, s, b5, GXD, w + L.oB5, GNO);
    DVAE_LAUNCH_OK("mcem_generic_pack");
    return 0;
}

int launch_generic_chain(const dvae_mcem_plan_t* plan, const void* wcopy, const MhArgs& m, hipStream_t s) {
    const GenLayout L = gen_layout(plan->z_dim, plan->h_dim, plan->h2_dim, plan->y_dim);
    GenArgs a;
    memset(&a, 0, sizeof(a));
    a.m = m;
    a.m.ydim = plan->y_dim;
    const int64_t ntiles = (m.N + GTB - 1) / GTB;
    a.m.ntiles = (int)(ntiles < 0x7fffffff ? ntiles : 0x7fffffff);
    a.zdim = plan->z_dim; a.zp = L.zp; a.yp = L.yp; a.h1p = L.h1p; a.h2p = L.h2p;
    const float* w = (const float*)wcopy;
    a.W3z = w + L.oW3z; a.W3y = w + L.oW3y; a.W4 = w + L.oW4; a.W5 = w + L.oW5;
    a.b3 = w + L.oB3; a.b4 = w + L.oB4; a.b5 = w + L.oB5;
    constexpr size_t LDS_MAX = 160 * 1024;
    a.xv_lds = (size_t)L.lds_floats_xv * sizeof(float) <= LDS_MAX ? 1 : 0;
    const size_t lds = (size_t)(a.xv_lds ? L.lds_floats_xv : L.lds_floats_base) * sizeof(float);
    if (lds > LDS_MAX) { set_error("mcem generic chain: %zu B of LDS needed, %zu available", lds, LDS_MAX); return DVAE_E_UNSUPPORTED; }
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)mcem_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute(mcem_generic_kernel, %zu B LDS): %s", LDS_MAX, hipGetErrorString(e)); return (int)e; }
        attr_done = true;
    }
    // one workgroup per tile up to a grid that keeps every CU busy for several rounds; the rest strides
    const int64_t grid = ntiles < 8192 ? ntiles : 8192;
    hipLaunchKernelGGL(mcem_generic_kernel, dim3((unsigned)grid), dim3(256), lds, s, a);
    DVAE_LAUNCH_OK("mcem_generic_kernel");
    return 0;
}

}  // namespace fused
}  // namespace dvae

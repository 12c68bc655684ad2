// The VAE encoder and the classifier over a ragged batch for models of ANY covered size, one launch each (include/dvae.h:
// dvae_encode_generic_batch, dvae_classify_generic_batch; disentangled-vae_amd/encode.py, classify.py: the packs made with generic=True).
// The resident kernels (encode.hip, classify.hip) are written for 513-128-128 and stay the default there; this file serves every
// other size within the limits of dvae_mcem_plan_dims, and 128 / 128 too under a generic pack.
//
//   encoder     [x | y] (513 + y_dim) -> h1 (tanh) -> h2 (tanh) -> {mu z, log_var z}; y_dim 0..513, h1 / h2 1..512, z 1..128
//   classifier  x (513) -> h1 (relu) -> h2 (relu) -> y_dim logits (sigmoid);         y_dim 1..513, h1 / h2 1..512, no batch norm
//
// The design is mcem_generic.hip's, a row MLP instead of a chain:
//   * 256 threads own a tile of 16 frames.  Products run on v_mfma_f32_16x16x4_f32, exact fp32: 16 weight rows are the A operand, the
//     tile's 16 frames the B columns; the four waves split a layer's row tiles (wave w: tiles w, w + 4, ...).
//   * Weights stream from a packed copy in fragment order [row tile][k block of 16][lane][4] (lane l holds row l & 15, inputs
//     16 b + 4 i + (l >> 4), i = 0..3): one 16-byte load per lane and four MFMAs.  Rows and inputs are zero-padded to multiples of 16,
//     so the loops have runtime trip counts and no tails: a padded hidden unit has zero in-weights and zero bias (tanh 0 = relu 0 = 0)
//     and zero out-weights; a padded output row is computed and dropped.  The x block (513 -> 528) and the label block (y_dim -> up16)
//     are padded separately; the sum runs over x first, then y, as torch.cat([x, y], 1) lays them.  The two heads are one output
//     matrix: mu in rows 0 .. z - 1, log_var in rows up16(z) .. up16(z) + z - 1.
//   * Activations sit in LDS as [k][16] floats.  The input tile [528 + up16(y_dim)][16] is staged whole (at most 66 KB; the power
//     formed on the way in from complex frames, spec_power.hpp: the bits of McemBatch.X2; label rows read in place at their stride);
//     H1 and H2 are at most 32 KB each; the output tile (heads <= 256 rows, logits <= 528 rows) reuses the input region: 130 KB at the
//     largest geometry, 33 KB + H1 + H2 at small ones, sized from the dims at launch.
//   * Every output element is one chain over k ascending from 0 (four products per MFMA step), the bias added after it, whatever the
//     frame's place in its tile, the tile's place in the grid and the frames around it: a frame gives the same bits alone, in any
//     batch and from run to run.  Frames outside [frame_off[0], frame_off[U]) or past N are neither read nor written.
//   * tanhf / expf as encode.hip and classify.hip use them (not the chain kernel's fast tanh): the error model of tests/encode_ref.py
//     allows one rounding of |h| per activation.
//   * 64-bit indexing throughout; the column table gets encode_kernel's defensive search.
#include <math.h>
#include "common.hpp"
#include "frame_tiles.hpp"
#include "spec_power.hpp"

namespace dvae {

constexpr int MT = 16;                        // frames per tile
constexpr int MXP = 528, MKX = MXP / 16;      // the x block padded to a multiple of 16, its k blocks
constexpr int M_HMAX = 512, M_ZMAX = 128;     // the limits of dvae_mcem_plan_dims

static inline int mup16(int v) { return (v + 15) / 16 * 16; }

// element offsets of the packed copy (floats) and the LDS plan of one launch
struct MlpLayout {
    int yp, h1p, h2p, outp;                   // padded sizes (multiples of 16; yp 0 without a label block)
    int64_t oW1x, oW1y, oW2, oW3, oB1, oB2, oB3, elems;
    size_t lds_bytes;
};

// y_in: width of the label block of layer 1 (0 for the classifier); outp: padded output rows (2 up16(z) or up16(y_dim))
static MlpLayout mlp_layout(int y_in, int h1, int h2, int outp) {
    MlpLayout L;
    L.yp = y_in ? mup16(y_in) : 0; L.h1p = mup16(h1); L.h2p = mup16(h2); L.outp = outp;
    L.oW1x = 0;
    L.oW1y = L.oW1x + (int64_t)L.h1p * MXP;
    L.oW2 = L.oW1y + (int64_t)L.h1p * L.yp;
    L.oW3 = L.oW2 + (int64_t)L.h2p * L.h1p;
    L.oB1 = L.oW3 + (int64_t)L.outp * L.h2p;
    L.oB2 = L.oB1 + L.h1p;
    L.oB3 = L.oB2 + L.h2p;
    L.elems = L.oB3 + L.outp;
    L.lds_bytes = (size_t)MT * (MXP + L.yp + L.h1p + L.h2p) * sizeof(float) + MT * (sizeof(int64_t) + sizeof(int));
    return L;
}

static bool enc_dims_ok(int y_dim, int h1, int h2, int z) {
    return y_dim >= 0 && y_dim <= CF && h1 >= 1 && h1 <= M_HMAX && h2 >= 1 && h2 <= M_HMAX && z >= 1 && z <= M_ZMAX;
}
static bool clf_dims_ok(int h1, int h2, int y_dim) {
    return y_dim >= 1 && y_dim <= CF && h1 >= 1 && h1 <= M_HMAX && h2 >= 1 && h2 <= M_HMAX;
}

struct MlpArgs {
    const void* src;      // complex64 [N][513] or float32 [N][ld]
    int is_complex;
    int64_t ld, N, lo, hi;                   // frames lo <= r < hi are worked on (0 <= lo <= hi <= N, checked by the host)
    const float* y;       // encoder: label rows [N][ldy] or null
    int64_t ldy;
    int y_in, yp, h1p, h2p, outp;
    const float *W1x, *W1y, *W2, *W3, *b1, *b2, *b3;          // the packed copy
    // encoder
    int z, zp;
    const float* eps;     // [N][z] or null
    float *mu, *log_var, *zs;                // [N][z], each may be null
    float* Z;             // [z][ntot] or null
    int64_t ntot;
    int U;
    const int64_t* tab;   // device [frame prefix (U + 1) | first column (U)], read only when Z is given
    // classifier
    int y_out;
    float *soft, *hard, *logits;             // [N][y_out]; logits may be null
    int64_t tile0, ntiles;
    const float *nmean, *ndiv;               // NORM: [513] mean and fl32(std + fl32(eps)) of the standardised encoder input
};

// acc += W[row tile] (16 x 16 kb) * act (16 kb x 16 frames): W in fragment order, act in LDS as [k][16]
__device__ __forceinline__ f32x4 mlp_gemm(f32x4 acc, const float* __restrict__ wt, int kb, const float* act, int lane) {
    const f32x4* w = reinterpret_cast<const f32x4*>(wt) + lane;
    for (int b = 0; b < kb; ++b) {
        const f32x4 a = w[(int64_t)b * 64];
        const float* bp = act + b * 256 + lane;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bp[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bp[64], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bp[128], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bp[192], acc, 0, 0, 0);
    }
    return acc;
}

template <int CLF>
__device__ __forceinline__ float mlp_act(float v) {
    return CLF ? (v > 0.f ? v : 0.f) : tanhf(v);
}

// CLF = 0: the encoder (tanh, heads, reparametrisation, column output); CLF = 1: the classifier (relu, sigmoid, hard labels)
// NORM (the encoder only): the x block is (p - mean) / div, formed after the power, by the rounding of the train step (train_generic.hip)
template <int CLF, int NORM = 0>
__global__ __launch_bounds__(256) void mlp_generic_kernel(const MlpArgs g) {
    extern __shared__ __attribute__((aligned(16))) float msm[];
    float* In = msm;                                    // [528 + yp][16]; then the output tile [outp][16]
    float* H1 = In + MT * (MXP + g.yp);                 // [h1p][16]
    float* H2 = H1 + MT * g.h1p;                        // [h2p][16]
    int64_t* colof = reinterpret_cast<int64_t*>(H2 + MT * g.h2p);      // [16] the frame's column of Z, -1: none
    int* rowok = reinterpret_cast<int*>(colof + MT);                   // [16]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int kb_y = g.yp >> 4, kb_1 = g.h1p >> 4, kb_2 = g.h2p >> 4;
    const int nt1 = g.h1p >> 4, nt2 = g.h2p >> 4, nt3 = g.outp >> 4;

    for (int64_t tile = g.tile0 + blockIdx.x; tile < g.tile0 + g.ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * MT;
        __syncthreads();                                   // the previous tile's readers of rowok, colof and the output tile are done
        if (tid < MT) {
            const int64_t r = r0 + tid;
            const int ok = (r >= g.lo && r < g.hi && r < g.N) ? 1 : 0;
            rowok[tid] = ok;
            int64_t c = -1;
            if (!CLF && ok && g.Z) {
                // the device copy of the tables the host checked: whatever it holds, the search stays inside its 2 U + 1 entries and
                // a column is used only inside [0, ntot)
                const int64_t* tab = g.tab;
                int a = 0, b = g.U;                        // tab[a] <= r < tab[b] for the table the host saw
                while (b - a > 1) {
                    const int mid = (a + b) >> 1;
                    if (tab[mid] <= r) a = mid; else b = mid;
                }
                const int64_t d = r - tab[a], c0 = tab[g.U + 1 + a];
                if (d >= 0 && d < g.ntot && c0 >= 0 && c0 < g.ntot && c0 + d < g.ntot) c = c0 + d;
            }
            colof[tid] = c;
        }
        __syncthreads();

        // ---- the input tile: a quarter wave reads 16 consecutive inputs of one frame ----
        for (int b = wave; b < MKX; b += 4) {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
                const int k = 16 * b + col, c = 4 * cq + quad;
                float p = 0.f;
                if (k < CF && rowok[c]) {
                    const int64_t at = (r0 + c) * g.ld + k;
                    if (g.is_complex) {
                        const float2 v = ((const float2*)g.src)[at];
                        p = np_power_c64(v.x, v.y);
                    } else {
                        p = ((const float*)g.src)[at];
                    }
                    if (NORM) p = __fdiv_rn(__fsub_rn(p, g.nmean[k]), g.ndiv[k]);
                }
                In[k * MT + c] = p;
            }
        }
        if (!CLF) {
            float* Iny = In + MT * MXP;
            for (int b = wave; b < kb_y; b += 4) {
#pragma unroll
                for (int cq = 0; cq < 4; ++cq) {
                    const int k = 16 * b + col, c = 4 * cq + quad;
                    Iny[k * MT + c] = (k < g.y_in && rowok[c]) ? g.y[(r0 + c) * g.ldy + k] : 0.f;
                }
            }
        }
        __syncthreads();

        // ---- layer 1: h1 = act([x | y] W1^T + b1), x first, then y ----
        for (int t = wave; t < nt1; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mlp_gemm(acc, g.W1x + (int64_t)t * MKX * 256, MKX, In, lane);
            if (!CLF) acc = mlp_gemm(acc, g.W1y + (int64_t)t * kb_y * 256, kb_y, In + MT * MXP, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                H1[row * MT + col] = mlp_act<CLF>(acc[r] + g.b1[row]);
            }
        }
        __syncthreads();
        // ---- layer 2: h2 = act(h1 W2^T + b2) ----
        for (int t = wave; t < nt2; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mlp_gemm(acc, g.W2 + (int64_t)t * kb_1 * 256, kb_1, H1, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                H2[row * MT + col] = mlp_act<CLF>(acc[r] + g.b2[row]);
            }
        }
        __syncthreads();
        // ---- output layer into the input region (its last readers passed two barriers): [mu | log_var] or the logits ----
        float* Out = In;
        for (int t = wave; t < nt3; t += 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mlp_gemm(acc, g.W3 + (int64_t)t * kb_2 * 256, kb_2, H2, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * quad + r;
                Out[row * MT + col] = acc[r] + g.b3[row];
            }
        }
        __syncthreads();

        if (CLF) {
            // rows: element i of the tile's [16][y_out] block, consecutive threads consecutive addresses
            for (int i = tid; i < MT * g.y_out; i += 256) {
                const int c = i / g.y_out, j = i - c * g.y_out;
                if (rowok[c]) {
                    const int64_t at = r0 * g.y_out + i;
                    const float logit = Out[j * MT + c];
                    const float s = 1.f / (1.f + expf(-logit));
                    g.soft[at] = s;
                    g.hard[at] = s > 0.5f ? 1.f : 0.f;
                    if (g.logits) g.logits[at] = logit;
                }
            }
        } else {
            if (g.mu || g.log_var || g.zs) {
                for (int i = tid; i < MT * g.z; i += 256) {
                    const int c = i / g.z, j = i - c * g.z;
                    if (rowok[c]) {
                        const int64_t at = r0 * g.z + i;
                        const float m = Out[j * MT + c], lv = Out[(g.zp + j) * MT + c];
                        if (g.mu) g.mu[at] = m;
                        if (g.log_var) g.log_var[at] = lv;
                        if (g.zs) g.zs[at] = __fadd_rn(m, __fmul_rn(expf(__fmul_rn(0.5f, lv)), g.eps[at]));
                    }
                }
            }
            // columns: consecutive threads consecutive frames (consecutive columns of Z)
            if (g.Z) {
                for (int i = tid; i < MT * g.z; i += 256) {
                    const int64_t c = colof[i & 15];
                    if (c >= 0) g.Z[(int64_t)(i >> 4) * g.ntot + c] = Out[i];
                }
            }
        }
    }
}

// nn.Linear [rows][ld] fp32, columns c0 .. c0 + cols - 1 -> fragment order [row tile][k block][lane][4], zero padded
__global__ void mlp_generic_pack_kernel(const float* __restrict__ src, int rows, int cols, int c0, int64_t ld, float* __restrict__ dst, int nt, int kb) {
    const int64_t total = (int64_t)nt * kb * 256;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i & 3), ln = (int)((i >> 2) & 63);
        const int b = (int)((i >> 8) % kb), t = (int)((i >> 8) / kb);
        const int row = 16 * t + (ln & 15), k = 16 * b + 4 * e + (ln >> 4);
        dst[i] = (row < rows && k < cols) ? src[(int64_t)row * ld + c0 + k] : 0.f;
    }
}

__global__ void mlp_generic_bias_kernel(const float* __restrict__ src, int n, float* __restrict__ dst, int np) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) dst[i] = i < n ? src[i] : 0.f;
}

static void mlp_pack_matrix(const float* src, int rows, int cols, int c0, int64_t ld, float* dst, int rp, int kp, hipStream_t s) {
    const int64_t total = (int64_t)rp * kp;
    if (total == 0) return;
    const int64_t blocks = (total + 255) / 256 < 512 ? (total + 255) / 256 : 512;
    hipLaunchKernelGGL(mlp_generic_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, rows, cols, c0, ld, dst, rp / 16, kp / 16);
}

static void mlp_pack_bias(const float* src, int n, float* dst, int np, hipStream_t s) {
    hipLaunchKernelGGL(mlp_generic_bias_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, src, n, dst, np);
}

static void mlp_weights(MlpArgs& g, const MlpLayout& L, const float* w) {
    g.yp = L.yp; g.h1p = L.h1p; g.h2p = L.h2p; g.outp = L.outp;
    g.W1x = w + L.oW1x; g.W1y = w + L.oW1y; g.W2 = w + L.oW2; g.W3 = w + L.oW3;
    g.b1 = w + L.oB1; g.b2 = w + L.oB2; g.b3 = w + L.oB3;
}

template <int CLF, int NORM = 0>
static int mlp_launch(const char* name, MlpArgs& g, const MlpLayout& L, hipStream_t s) {
    constexpr size_t LDS_MAX = 160 * 1024;
    if (L.lds_bytes > LDS_MAX) { set_error("%s: %zu B of LDS needed, %zu available", name, L.lds_bytes, LDS_MAX); return DVAE_E_UNSUPPORTED; }
    if (L.lds_bytes > 64 * 1024) {                                    // past the default limit of dynamic LDS: raised once per device
        static bool attr_done[64] = {};
        int dev = 0;
        DVAE_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !attr_done[dev]) {
            hipError_t e = hipFuncSetAttribute((const void*)mlp_generic_kernel<CLF, NORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
            if (e != hipSuccess) { set_error("hipFuncSetAttribute(%s, %zu B LDS): %s", name, LDS_MAX, hipGetErrorString(e)); return (int)e; }
            if (dev >= 0 && dev < 64) attr_done[dev] = true;
        }
    }
    g.tile0 = g.lo / MT;
    g.ntiles = cdiv(g.hi, MT) - g.tile0;
    const int64_t blocks = g.ntiles < 2048 ? g.ntiles : 2048;         // the cap of the resident kernels; the rest strides
    hipLaunchKernelGGL((mlp_generic_kernel<CLF, NORM>), dim3((unsigned)blocks), dim3(256), L.lds_bytes, s, g);
    DVAE_LAUNCH_OK(name);
    return 0;
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_encode_generic_weights_floats(int y_dim, int h1, int h2, int z_dim) {
    if (!enc_dims_ok(y_dim, h1, h2, z_dim)) return 0;
    return (size_t)mlp_layout(y_dim, h1, h2, 2 * mup16(z_dim)).elems;
}

extern "C" size_t dvae_classify_generic_weights_floats(int h1, int h2, int y_dim) {
    if (!clf_dims_ok(h1, h2, y_dim)) return 0;
    return (size_t)mlp_layout(0, h1, h2, mup16(y_dim)).elems;
}

extern "C" int dvae_encode_generic_pack(int y_dim, int h1, int h2, int z_dim, const float* W1, int64_t ld1, const float* b1, const float* W2,
                                        int64_t ld2, const float* b2, const float* Wmu, int64_t ldmu, const float* bmu, const float* Wlv,
                                        int64_t ldlv, const float* blv, float* weights, void* stream) {
    DVAE_CHECK_ARG(enc_dims_ok(y_dim, h1, h2, z_dim), "encode_generic_pack: y_dim %d, hidden %d / %d, z_dim %d (the kernel covers y_dim 0..%d, "
                   "hidden widths 1..%d, z_dim 1..%d)", y_dim, h1, h2, z_dim, CF, M_HMAX, M_ZMAX);
    DVAE_CHECK_ARG(W1 && b1 && W2 && b2 && Wmu && bmu && Wlv && blv && weights, "encode_generic_pack: null pointer");
    DVAE_CHECK_ARG(ld1 >= CF + y_dim && ld2 >= h1 && ldmu >= h2 && ldlv >= h2, "encode_generic_pack: leading dimensions %lld, %lld, %lld, %lld for "
                   "rows of %d, %d, %d, %d", (long long)ld1, (long long)ld2, (long long)ldmu, (long long)ldlv, CF + y_dim, h1, h2, h2);
    hipStream_t s = (hipStream_t)stream;
    const int zp = mup16(z_dim);
    const MlpLayout L = mlp_layout(y_dim, h1, h2, 2 * zp);
    mlp_pack_matrix(W1, h1, CF, 0, ld1, weights + L.oW1x, L.h1p, MXP, s);
    mlp_pack_matrix(W1, h1, y_dim, CF, ld1, weights + L.oW1y, L.h1p, L.yp, s);
    mlp_pack_matrix(W2, h2, h1, 0, ld2, weights + L.oW2, L.h2p, L.h1p, s);
    mlp_pack_matrix(Wmu, z_dim, h2, 0, ldmu, weights + L.oW3, zp, L.h2p, s);
    mlp_pack_matrix(Wlv, z_dim, h2, 0, ldlv, weights + L.oW3 + (int64_t)zp * L.h2p, zp, L.h2p, s);
    mlp_pack_bias(b1, h1, weights + L.oB1, L.h1p, s);
    mlp_pack_bias(b2, h2, weights + L.oB2, L.h2p, s);
    mlp_pack_bias(bmu, z_dim, weights + L.oB3, zp, s);
    mlp_pack_bias(blv, z_dim, weights + L.oB3 + zp, zp, s);
    DVAE_LAUNCH_OK("encode_generic_pack");
    return 0;
}

extern "C" int dvae_classify_generic_pack(int h1, int h2, int y_dim, const float* W1, int64_t ld1, const float* b1, const float* W2, int64_t ld2,
                                          const float* b2, const float* W3, int64_t ld3, const float* b3, float* weights, void* stream) {
    DVAE_CHECK_ARG(clf_dims_ok(h1, h2, y_dim), "classify_generic_pack: hidden %d / %d, y_dim %d (the kernel covers hidden widths 1..%d, y_dim 1..%d)",
                   h1, h2, y_dim, M_HMAX, CF);
    DVAE_CHECK_ARG(W1 && b1 && W2 && b2 && W3 && b3 && weights, "classify_generic_pack: null pointer");
    DVAE_CHECK_ARG(ld1 >= CF && ld2 >= h1 && ld3 >= h2, "classify_generic_pack: leading dimensions %lld, %lld, %lld for rows of %d, %d, %d",
                   (long long)ld1, (long long)ld2, (long long)ld3, CF, h1, h2);
    hipStream_t s = (hipStream_t)stream;
    const MlpLayout L = mlp_layout(0, h1, h2, mup16(y_dim));
    mlp_pack_matrix(W1, h1, CF, 0, ld1, weights + L.oW1x, L.h1p, MXP, s);
    mlp_pack_matrix(W2, h2, h1, 0, ld2, weights + L.oW2, L.h2p, L.h1p, s);
    mlp_pack_matrix(W3, y_dim, h2, 0, ld3, weights + L.oW3, L.outp, L.h2p, s);
    mlp_pack_bias(b1, h1, weights + L.oB1, L.h1p, s);
    mlp_pack_bias(b2, h2, weights + L.oB2, L.h2p, s);
    mlp_pack_bias(b3, y_dim, weights + L.oB3, L.outp, s);
    DVAE_LAUNCH_OK("classify_generic_pack");
    return 0;
}

static int encode_generic(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                          const int64_t* frame_off_host, const float* weights, int y_dim, int h1, int h2, int z_dim,
                          const float* eps, float* mu, float* log_var, float* z, float* Z, int64_t ntot,
                          const int64_t* col_host, const int64_t* tables_dev, const float* nmean, const float* ndiv, void* stream) {
    DVAE_CHECK_ARG(src && frame_off_host && weights, "encode_generic_batch: null pointer");
    DVAE_CHECK_ARG(enc_dims_ok(y_dim, h1, h2, z_dim), "encode_generic_batch: y_dim %d, hidden %d / %d, z_dim %d (the kernel covers y_dim 0..%d, "
                   "hidden widths 1..%d, z_dim 1..%d)", y_dim, h1, h2, z_dim, CF, M_HMAX, M_ZMAX);
    DVAE_CHECK_ARG(mu || log_var || z || Z, "encode_generic_batch: no output (mu, log_var, z and Z are all null)");
    DVAE_CHECK_ARG(!z || eps, "encode_generic_batch: z needs eps");
    DVAE_CHECK_ARG((y_dim > 0) == (y != nullptr), "encode_generic_batch: y must be given exactly when y_dim > 0 (y_dim %d)", y_dim);
    DVAE_CHECK_ARG(N > 0 && U > 0, "encode_generic_batch: %lld rows, %d utterances", (long long)N, U);
    DVAE_CHECK_ARG(src_complex == 0 || src_complex == 1, "encode_generic_batch: src_complex %d", src_complex);
    DVAE_CHECK_ARG(src_complex ? ld == CF : ld >= CF, "encode_generic_batch: leading dimension %lld (%s)", (long long)ld,
                   src_complex ? "complex frames are packed: 513" : "at least 513");
    DVAE_CHECK_ARG(!y || (ldy >= y_dim && ldy < ((int64_t)1 << 20)), "encode_generic_batch: label leading dimension %lld for y_dim %d", (long long)ldy, y_dim);
    DVAE_CHECK_ARG(N < ((int64_t)1 << 40) && ld < ((int64_t)1 << 20), "encode_generic_batch: %lld rows of %lld", (long long)N, (long long)ld);
    if (int rc = check_frame_off("encode_generic_batch", frame_off_host, U, N)) return rc;
    if (Z) {
        DVAE_CHECK_ARG(col_host && tables_dev, "encode_generic_batch: the column output needs the column table on the host and both tables on the device");
        DVAE_CHECK_ARG(ntot > 0 && ntot < ((int64_t)1 << 40), "encode_generic_batch: %lld columns", (long long)ntot);
        int64_t end = 0;                                   // the columns of the utterances so far end here
        for (int u = 0; u < U; ++u) {
            const int64_t c = frame_off_host[u + 1] - frame_off_host[u];
            DVAE_CHECK_ARG(col_host[u] >= end, "encode_generic_batch: the column table goes back at utterance %d (column %lld, %lld taken)", u,
                           (long long)col_host[u], (long long)end);
            DVAE_CHECK_ARG(col_host[u] <= ntot - c, "encode_generic_batch: utterance %d (columns [%lld, %lld)) leaves the %lld columns", u,
                           (long long)col_host[u], (long long)(col_host[u] + c), (long long)ntot);
            end = col_host[u] + c;
        }
    }
    MlpArgs g{};
    g.src = src; g.is_complex = src_complex; g.ld = ld; g.N = N;
    g.lo = frame_off_host[0]; g.hi = frame_off_host[U];
    if (g.hi == g.lo) return 0;
    g.y = y; g.ldy = ldy; g.y_in = y_dim;
    g.z = z_dim; g.zp = mup16(z_dim);
    const MlpLayout L = mlp_layout(y_dim, h1, h2, 2 * g.zp);
    mlp_weights(g, L, weights);
    g.eps = eps; g.mu = mu; g.log_var = log_var; g.zs = z;
    g.Z = Z; g.ntot = ntot; g.U = U; g.tab = tables_dev;
    if (nmean) {
        g.nmean = nmean; g.ndiv = ndiv;
        return mlp_launch<0, 1>("encode_generic_norm_kernel", g, L, (hipStream_t)stream);
    }
    return mlp_launch<0>("encode_generic_kernel", g, L, (hipStream_t)stream);
}

extern "C" int dvae_encode_generic_batch(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                                         const int64_t* frame_off_host, const float* weights, int y_dim, int h1, int h2, int z_dim,
                                         const float* eps, float* mu, float* log_var, float* z, float* Z, int64_t ntot,
                                         const int64_t* col_host, const int64_t* tables_dev, void* stream) {
    return encode_generic(src, src_complex, ld, y, ldy, N, U, frame_off_host, weights, y_dim, h1, h2, z_dim, eps, mu, log_var, z, Z, ntot,
                          col_host, tables_dev, nullptr, nullptr, stream);
}

extern "C" int dvae_encode_generic_batch_norm(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                                              const int64_t* frame_off_host, const float* weights, int y_dim, int h1, int h2, int z_dim,
                                              const float* eps, float* mu, float* log_var, float* z, float* Z, int64_t ntot,
                                              const int64_t* col_host, const int64_t* tables_dev, const float* norm_mean,
                                              const float* norm_div, void* stream) {
    DVAE_CHECK_ARG(norm_mean && norm_div, "encode_generic_batch_norm: null norm_mean / norm_div (513 device floats each)");
    return encode_generic(src, src_complex, ld, y, ldy, N, U, frame_off_host, weights, y_dim, h1, h2, z_dim, eps, mu, log_var, z, Z, ntot,
                          col_host, tables_dev, norm_mean, norm_div, stream);
}

extern "C" int dvae_classify_generic_batch(const void* src, int src_complex, int64_t ld, int64_t N, int U, const int64_t* frame_off_host,
                                           const float* weights, int y_dim, int h1, int h2, float* soft, float* hard, float* logits,
                                           void* stream) {
    DVAE_CHECK_ARG(src && frame_off_host && weights && soft && hard, "classify_generic_batch: null pointer");
    DVAE_CHECK_ARG(clf_dims_ok(h1, h2, y_dim), "classify_generic_batch: hidden %d / %d, y_dim %d (the kernel covers hidden widths 1..%d, y_dim 1..%d)",
                   h1, h2, y_dim, M_HMAX, CF);
    DVAE_CHECK_ARG(N > 0 && U > 0, "classify_generic_batch: %lld rows, %d utterances", (long long)N, U);
    DVAE_CHECK_ARG(src_complex == 0 || src_complex == 1, "classify_generic_batch: src_complex %d", src_complex);
    DVAE_CHECK_ARG(src_complex ? ld == CF : ld >= CF, "classify_generic_batch: leading dimension %lld (%s)", (long long)ld,
                   src_complex ? "complex frames are packed: 513" : "at least 513");
    DVAE_CHECK_ARG(N < ((int64_t)1 << 40) && ld < ((int64_t)1 << 20), "classify_generic_batch: %lld rows of %lld", (long long)N, (long long)ld);
    if (int rc = check_frame_off("classify_generic_batch", frame_off_host, U, N)) return rc;
    MlpArgs g{};
    g.src = src; g.is_complex = src_complex; g.ld = ld; g.N = N;
    g.lo = frame_off_host[0]; g.hi = frame_off_host[U];
    if (g.hi == g.lo) return 0;
    g.y_out = y_dim;
    const MlpLayout L = mlp_layout(0, h1, h2, mup16(y_dim));
    mlp_weights(g, L, weights);
    g.soft = soft; g.hard = hard; g.logits = logits;
    return mlp_launch<1>("classify_generic_kernel", g, L, (hipStream_t)stream);
}

// The VAE encoder over a whole ragged batch in one launch (disentangled-vae_amd/encode.py; the reference's `vae.encoder(torch.t(X2))`
// of packages/models/mcem.py:200, 364 and the encoding half of scripts/reconstruct_ntcd_M2.py:231-358, reconstruct_M2_info.py).
//
// dvae_encode_batch: Encoder([513 + y_dim, [128, 128], 16]): [x | y] -> 128 (tanh) -> 128 (tanh) -> {mu 16, log_var 16}, y_dim 0, 1 or
// 513, exact fp32 on v_mfma_f32_32x32x2_f32.  The skeleton is classify.hip's (frame_tiles.hpp): one 256-thread workgroup walks
// 64-frame tiles, grid-strided; layer 1 consumes k in 32-deep slabs, the input slab [64][32] (power squared on the way in from complex
// input, spec_power.hpp; label columns behind bin 512, as torch.cat([x, y], 1) lays them) and the W1 slab [128][32] staged in LDS with
// a register prefetch of the next slab; wave w owns hidden columns 32 w .. 32 w + 31 of all 64 frames; h1, then h2 in its place, stay
// in LDS [64][129], W2 streams through the slab buffer.
//
// The heads are 32 output columns (mu 0..15, log_var 16..31): their weights [32][128] are staged whole in the slab buffer, waves 0 and 1
// take frames 0..31 and 32..63 with one 32 x 32 accumulator each over k = 0..127 (waves 2 and 3 wait: 2 % of the tile's products).
// The results meet in LDS [64][33], from where every thread finishes four (frame, j) pairs: mu, log_var, z = mu + exp(0.5 log_var) eps,
// and the column output Z[j][col] of McemBatch's layout.
//
// Every output element is one chain over k ascending from 0 (layer 1 zero-padded to the slab multiple: 544, 544, 1056), the bias added
// after it, whatever the frame's place in its tile, the tile's place in the grid and the frames around it: a frame gives the same bits
// alone, in any batch and from run to run.  Frames outside [frame_off[0], frame_off[U]) or past N are neither read nor written.
#include "common.hpp"
#include "frame_tiles.hpp"
#include "spec_power.hpp"

namespace dvae {

constexpr int EZ = 16;                       // latent width; the heads are 2 EZ = 32 columns, one MFMA tile

struct EncodeArgs {
    const void* src;      // complex64 [N][513] or float32 [N][ld]
    int is_complex;
    int64_t ld, N, lo, hi;                   // frames lo <= r < hi are encoded (0 <= lo <= hi <= N, checked by the host)
    const float* y;       // [N][ldy] or null
    int64_t ldy;
    int y_dim, K1;                           // K1 = 513 + y_dim
    const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wlv, *blv;
    const float* eps;     // [N][16] or null
    float *mu, *log_var, *z;                 // [N][16], each may be null
    float* Z;             // [16][ntot] or null
    int64_t ntot;
    int U;
    const int64_t* tab;   // device [frame prefix (U + 1) | first column (U)], read only when Z is given
    int64_t tile0, ntiles;
};

// the next layer-1 slab of the input tile: 64 frames x 32 columns of [x | y], thread -> column (tid & 31), frames (tid >> 5) + 8 i
__device__ __forceinline__ void load_input(const EncodeArgs& g, int64_t r0, int kc, int tid, const int* rowok, float (&r)[8]) {
    const int k = kc + (tid & 31), rr = tid >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = rr + 8 * i;
        float p = 0.f;
        if (rowok[row]) {
            if (k < CF) {
                const int64_t at = (r0 + row) * g.ld + k;
                if (g.is_complex) {
                    const float2 v = ((const float2*)g.src)[at];
                    p = np_power_c64(v.x, v.y);
                } else {
                    p = ((const float*)g.src)[at];
                }
            } else if (k < g.K1) {
                p = g.y[(r0 + row) * g.ldy + (k - CF)];
            }
        }
        r[i] = p;
    }
}

__device__ __forceinline__ void store_tanh(float* H, const float* __restrict__ bias, int wave, int l31, int h, const f32x16& acc0, const f32x16& acc1) {
    const int col = wave * 32 + l31;
    const float b = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, h);
        H[row * HLD + col] = tanhf(acc0[r] + b);
        H[(32 + row) * HLD + col] = tanhf(acc1[r] + b);
    }
}

__global__ __launch_bounds__(256) void encode_kernel(const EncodeArgs g) {
    __shared__ float H[CT * HLD];
    __shared__ float As[CT * SLD];             // layer 1's input slab; then the heads' results [64][33]
    __shared__ float Bs[CH * SLD];             // weight slabs [128][33]; then the heads' weights [32][129]
    __shared__ int rowok[CT];
    __shared__ int64_t colof[CT];              // the frame's column of Z, -1: none
    static_assert(2 * EZ * HLD <= CH * SLD, "the heads' weights fit the slab buffer");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;

    for (int64_t tile = g.tile0 + blockIdx.x; tile < g.tile0 + g.ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * CT;
        __syncthreads();                                   // the previous tile's readers of rowok, colof, As and H are done
        if (tid < CT) {
            const int64_t r = r0 + tid;
            const int ok = (r >= g.lo && r < g.hi && r < g.N) ? 1 : 0;
            rowok[tid] = ok;
            int64_t c = -1;
            if (ok && g.Z) {
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

        // ---- layer 1: h1 = tanh([x | y] W1^T + b1), k = 0 .. K1 - 1 in slabs of 32 ----
        f32x16 acc0, acc1;
        zero(acc0); zero(acc1);
        float ra[8], rb[16];
        load_input(g, r0, 0, tid, rowok, ra);
        load_w(g.W1, CH, g.K1, 0, 0, tid, rb);
        for (int kc = 0; kc < g.K1; kc += CK) {
            {
                const int c = tid & 31, rr = tid >> 5;
#pragma unroll
                for (int i = 0; i < 8; ++i) As[(rr + 8 * i) * SLD + c] = ra[i];
            }
            store_w(Bs, tid, rb);
            __syncthreads();
            if (kc + CK < g.K1) {
                load_input(g, r0, kc + CK, tid, rowok, ra);
                load_w(g.W1, CH, g.K1, 0, kc + CK, tid, rb);
            }
            mfma_slab(As, SLD, 0, Bs, wave, l31, h, acc0, acc1);
            __syncthreads();
        }
        store_tanh(H, g.b1, wave, l31, h, acc0, acc1);

        // ---- layer 2: h2 = tanh(h1 W2^T + b2), in h1's place once every wave has read it ----
        zero(acc0); zero(acc1);
        load_w(g.W2, CH, CH, 0, 0, tid, rb);
        for (int kc = 0; kc < CH; kc += CK) {
            store_w(Bs, tid, rb);
            __syncthreads();                               // also orders layer 1's writes of H before the first read
            if (kc + CK < CH) load_w(g.W2, CH, CH, 0, kc + CK, tid, rb);
            mfma_slab(H, HLD, kc, Bs, wave, l31, h, acc0, acc1);
            __syncthreads();
        }
        store_tanh(H, g.b2, wave, l31, h, acc0, acc1);

        // ---- heads: [mu | log_var] = h2 [Wmu; Wlv]^T + [bmu | blv] ----
        for (int i = tid; i < 2 * EZ * CH; i += 256) {     // the last slab's readers passed the loop's closing barrier
            const int n = i >> 7, k = i & (CH - 1);
            Bs[n * HLD + k] = n < EZ ? g.Wmu[n * CH + k] : g.Wlv[(n - EZ) * CH + k];
        }
        __syncthreads();                                   // h2 and the heads' weights are in place
        if (wave < 2) {
            zero(acc0);
            const float* A = H + (32 * wave + l31) * HLD;
            const float* B = Bs + l31 * HLD;
#pragma unroll 8
            for (int kk = 0; kk < CH / 2; ++kk) {
                const int k = 2 * kk + h;
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A[k], B[k], acc0, 0, 0, 0);
            }
            const float b = l31 < EZ ? g.bmu[l31] : g.blv[l31 - EZ];
#pragma unroll
            for (int r = 0; r < 16; ++r) As[(32 * wave + acc_row(r, h)) * SLD + l31] = acc0[r] + b;
        }
        __syncthreads();

        // rows: thread -> frame tid >> 2, components 4 (tid & 3) .. + 3
        {
            const int row = tid >> 2, j0 = 4 * (tid & 3);
            if (rowok[row]) {
                const int64_t at = (r0 + row) * EZ + j0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float m = As[row * SLD + j0 + j], lv = As[row * SLD + EZ + j0 + j];
                    if (g.mu) g.mu[at + j] = m;
                    if (g.log_var) g.log_var[at + j] = lv;
                    if (g.z) g.z[at + j] = __fadd_rn(m, __fmul_rn(expf(__fmul_rn(0.5f, lv)), g.eps[at + j]));
                }
            }
        }
        // columns: thread -> frame tid & 63 (consecutive columns of Z), components tid >> 6 + 4 q
        if (g.Z) {
            const int row = tid & 63;
            const int64_t c = colof[row];
            if (c >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = (tid >> 6) + 4 * q;
                    g.Z[(int64_t)j * g.ntot + c] = As[row * SLD + j];
                }
            }
        }
    }
}

}  // namespace dvae

using namespace dvae;

extern "C" size_t dvae_encode_weights_floats(int y_dim) {
    if (y_dim != 0 && y_dim != 1 && y_dim != CF) return 0;
    return (size_t)CH * (CF + y_dim) + CH + (size_t)CH * CH + CH + 2 * ((size_t)EZ * CH + EZ);
}

extern "C" int dvae_encode_batch(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                                 const int64_t* frame_off_host, const float* weights, int y_dim, const float* eps, float* mu, float* log_var,
                                 float* z, float* Z, int64_t ntot, const int64_t* col_host, const int64_t* tables_dev, void* stream) {
    DVAE_CHECK_ARG(src && frame_off_host && weights, "encode_batch: null pointer");
    DVAE_CHECK_ARG(y_dim == 0 || y_dim == 1 || y_dim == CF, "encode_batch: y_dim %d (the kernel covers 0, 1 and %d)", y_dim, CF);
    DVAE_CHECK_ARG(mu || log_var || z || Z, "encode_batch: no output (mu, log_var, z and Z are all null)");
    DVAE_CHECK_ARG(!z || eps, "encode_batch: z needs eps");
    DVAE_CHECK_ARG((y_dim > 0) == (y != nullptr), "encode_batch: y must be given exactly when y_dim > 0 (y_dim %d)", y_dim);
    DVAE_CHECK_ARG(N > 0 && U > 0, "encode_batch: %lld rows, %d utterances", (long long)N, U);
    DVAE_CHECK_ARG(src_complex == 0 || src_complex == 1, "encode_batch: src_complex %d", src_complex);
    DVAE_CHECK_ARG(src_complex ? ld == CF : ld >= CF, "encode_batch: leading dimension %lld (%s)", (long long)ld,
                   src_complex ? "complex frames are packed: 513" : "at least 513");
    DVAE_CHECK_ARG(!y || (ldy >= y_dim && ldy < ((int64_t)1 << 20)), "encode_batch: label leading dimension %lld for y_dim %d", (long long)ldy, y_dim);
    DVAE_CHECK_ARG(N < ((int64_t)1 << 40) && ld < ((int64_t)1 << 20), "encode_batch: %lld rows of %lld", (long long)N, (long long)ld);
    if (int rc = check_frame_off("encode_batch", frame_off_host, U, N)) return rc;
    if (Z) {
        DVAE_CHECK_ARG(col_host && tables_dev, "encode_batch: the column output needs the column table on the host and both tables on the device");
        DVAE_CHECK_ARG(ntot > 0 && ntot < ((int64_t)1 << 40), "encode_batch: %lld columns", (long long)ntot);
        int64_t end = 0;                                   // the columns of the utterances so far end here
        for (int u = 0; u < U; ++u) {
            const int64_t c = frame_off_host[u + 1] - frame_off_host[u];
            DVAE_CHECK_ARG(col_host[u] >= end, "encode_batch: the column table goes back at utterance %d (column %lld, %lld taken)", u,
                           (long long)col_host[u], (long long)end);
            DVAE_CHECK_ARG(col_host[u] <= ntot - c, "encode_batch: utterance %d (columns [%lld, %lld)) leaves the %lld columns", u,
                           (long long)col_host[u], (long long)(col_host[u] + c), (long long)ntot);
            end = col_host[u] + c;
        }
    }
    EncodeArgs g{};
    g.src = src; g.is_complex = src_complex; g.ld = ld; g.N = N;
    g.lo = frame_off_host[0]; g.hi = frame_off_host[U];
    if (g.hi == g.lo) return 0;
    g.y = y; g.ldy = ldy; g.y_dim = y_dim; g.K1 = CF + y_dim;
    g.W1 = weights;              g.b1 = g.W1 + (size_t)CH * g.K1;
    g.W2 = g.b1 + CH;            g.b2 = g.W2 + (size_t)CH * CH;
    g.Wmu = g.b2 + CH;           g.bmu = g.Wmu + (size_t)EZ * CH;
    g.Wlv = g.bmu + EZ;          g.blv = g.Wlv + (size_t)EZ * CH;
    g.eps = eps; g.mu = mu; g.log_var = log_var; g.z = z;
    g.Z = Z; g.ntot = ntot; g.U = U; g.tab = tables_dev;
    g.tile0 = g.lo / CT;
    g.ntiles = cdiv(g.hi, CT) - g.tile0;
    const int64_t blocks = g.ntiles < 2048 ? g.ntiles : 2048;         // 256 CUs x 2 resident workgroups x 4 rounds; the rest strides
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g);
    DVAE_LAUNCH_OK("encode_kernel");
    return 0;
}

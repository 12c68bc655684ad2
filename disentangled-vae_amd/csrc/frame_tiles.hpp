// The pieces that the frame-tile networks share (classify.hip: the classifier; encode.hip: the VAE encoder): a 256-thread workgroup
// owns a tile of 64 frames, a layer consumes k in 32-deep slabs staged in LDS with a register prefetch of the next one, wave w owns
// output columns 32 w .. 32 w + 31 of all 64 frames as two 32 x 32 accumulators of v_mfma_f32_32x32x2_f32.  Every output element is
// one chain over k ascending, two products per step, whatever the frame's place in the tile.  Also the host check of a frame prefix
// table.
#pragma once
#include "common.hpp"

namespace dvae {

constexpr int CF = 513, CH = 128;            // bins, hidden width
constexpr int CT = 64, CK = 32;              // frames per tile, k per slab
constexpr int HLD = CH + 1, SLD = CK + 1;    // LDS row strides: odd, so the 32 rows an MFMA operand read touches land on distinct banks

// a weight slab: rows n0 .. n0 + 127 of W [nrows][K] (rows past nrows read as zero), columns kc .. kc + 31 (past K as zero)
__device__ __forceinline__ void load_w(const float* __restrict__ W, int nrows, int K, int n0, int kc, int tid, float (&r)[16]) {
    const int k = kc + (tid & 31), rr = tid >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = n0 + rr + 8 * i;
        r[i] = (k < K && n < nrows) ? W[(int64_t)n * K + k] : 0.f;
    }
}

__device__ __forceinline__ void store_w(float* Bs, int tid, const float (&r)[16]) {
    const int c = tid & 31, rr = tid >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) Bs[(rr + 8 * i) * SLD + c] = r[i];
}

// acc0 / acc1 += A[rows 0..31 / 32..63][k0 .. k0 + 31] * Bs[wave's 32 rows][0 .. 31]^T; A has row stride lda, k0 is its first column
__device__ __forceinline__ void mfma_slab(const float* A, int lda, int k0, const float* Bs, int wave, int l31, int h, f32x16& acc0, f32x16& acc1) {
#pragma unroll
    for (int kk = 0; kk < CK / 2; ++kk) {
        const int k = 2 * kk + h;
        const float a0 = A[l31 * lda + k0 + k], a1 = A[(32 + l31) * lda + k0 + k];
        const float b = Bs[(wave * 32 + l31) * SLD + k];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
    }
}

__device__ __forceinline__ void zero(f32x16& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// the frame prefix table of the entry points, on the host: 0 <= off[0] <= off[1] <= ... <= off[U] <= N
static int check_frame_off(const char* op, const int64_t* off, int U, int64_t N) {
    DVAE_CHECK_ARG(off[0] >= 0, "%s: the frame table starts at %lld", op, (long long)off[0]);
    for (int u = 0; u < U; ++u)
        DVAE_CHECK_ARG(off[u + 1] >= off[u], "%s: the frame table decreases at utterance %d (%lld after %lld)", op, u, (long long)off[u + 1],
                       (long long)off[u]);
    DVAE_CHECK_ARG(off[U] <= N, "%s: the frame table ends at %lld of %lld rows", op, (long long)off[U], (long long)N);
    return 0;
}

}  // namespace dvae

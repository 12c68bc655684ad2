// Device-side transform pieces of the STFT / ISTFT kernels (stft_fwd.hip, istft.hip) and of the ESTOI band kernel (estoi.hip): the complex
// type and its arithmetic, the radix-8 butterfly, the in-LDS radix-2 FFT of the generic power-of-two kernels with its tables, and the
// 512-point FFT of one wave that every nfft = 1024 kernel runs -- one body (fft512_passes) behind the two double types the kernels hold
// (Fft512, Fft512L), and the float form (Fft512F).  The kernels and what they compute stand in stft_fwd.hip / istft.hip, the host entries in stft.hip.
#pragma once
#include "common.hpp"

namespace dvae {

template <typename T> struct cx { T x, y; };
typedef cx<double> cd;
typedef cx<float> cf;
template <typename T> __device__ __forceinline__ cx<T> cmul(cx<T> a, cx<T> b) { return cx<T>{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename T> __device__ __forceinline__ cx<T> cadd(cx<T> a, cx<T> b) { return cx<T>{a.x + b.x, a.y + b.y}; }
template <typename T> __device__ __forceinline__ cx<T> csub(cx<T> a, cx<T> b) { return cx<T>{a.x - b.x, a.y - b.y}; }
template <typename T> __device__ __forceinline__ cx<T> cconj(cx<T> a) { return cx<T>{a.x, -a.y}; }
template <typename T> __device__ __forceinline__ cx<T> cmulc(cx<T> a, T wr, T wi) { return cx<T>{a.x * wr - a.y * wi, a.x * wi + a.y * wr}; }

// in-LDS radix-2 DIT FFT of M = 1 << logM points already stored in bit-reversed order.
// tw[k] = exp(-2 pi i k / (2M)), k < M.  inverse != 0 conjugates the twiddles.
__device__ __forceinline__ void fft_lds(cd* z, const cd* tw, int logM, int inverse) {
    const int M = 1 << logM;
    for (int s = 1; s <= logM; ++s) {
        const int half = 1 << (s - 1);
        for (int j = threadIdx.x; j < (M >> 1); j += blockDim.x) {
            const int grp = j >> (s - 1), pos = j & (half - 1);
            const int i0 = (grp << s) + pos, i1 = i0 + half;
            cd w = tw[2 * pos * (M >> s)];
            if (inverse) w.y = -w.y;
            const cd a = z[i0], b = cmul(w, z[i1]);
            z[i0] = cadd(a, b);
            z[i1] = csub(a, b);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void stage_tables(cd* tw, double* win, const double* window, int nfft) {
    const int M = nfft >> 1;
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        double s, c;
        sincospi(-2.0 * (double)k / (double)nfft, &s, &c);
        tw[k] = cd{c, s};
    }
    for (int i = threadIdx.x; i < nfft; i += blockDim.x) win[i] = window[i];
}

// in-place 8-point DFT (forward), natural-order output
template <typename T>
__device__ __forceinline__ void dft8(cx<T> (&a)[8]) {
    typedef cx<T> C;
    constexpr T H = (T)0.70710678118654752440;
    C b[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { b[i] = cadd(a[i], a[i + 4]); }
    { const C d = csub(a[0], a[4]); b[4] = d; }
    { const C d = csub(a[1], a[5]); b[5] = C{(d.x + d.y) * H, (d.y - d.x) * H}; }        // * (1 - i)/sqrt2
    { const C d = csub(a[2], a[6]); b[6] = C{d.y, -d.x}; }                               // * -i
    { const C d = csub(a[3], a[7]); b[7] = C{(d.y - d.x) * H, -(d.x + d.y) * H}; }       // * (-1 - i)/sqrt2
    C c[8];
#pragma unroll
    for (int q = 0; q < 8; q += 4) {
        c[q] = cadd(b[q], b[q + 2]); c[q + 1] = cadd(b[q + 1], b[q + 3]);
        c[q + 2] = csub(b[q], b[q + 2]);
        const C d = csub(b[q + 1], b[q + 3]); c[q + 3] = C{d.y, -d.x};                   // * -i
    }
    a[0] = cadd(c[0], c[1]); a[4] = csub(c[0], c[1]); a[2] = cadd(c[2], c[3]); a[6] = csub(c[2], c[3]);
    a[1] = cadd(c[4], c[5]); a[5] = csub(c[4], c[5]); a[3] = cadd(c[6], c[7]); a[7] = csub(c[6], c[7]);
}

__device__ __forceinline__ int padidx(int i) { return i + (i >> 3); }     // one slot of padding per 8: strides 8 and 64 both conflict-free

// 512-point complex forward FFT of one wave, double: v[r] = x[lane + 64 r] in, X[lane + 64 r] out (both natural order), three radix-8
// Stockham passes with 8 points per lane in registers; lanes exchange data through re / im, the wave's private padded LDS buffers
// (512 + 64 doubles each), between passes (no workgroup barrier: a wave's LDS accesses are ordered).  tw1(r) = exp(-2 pi i r (lane & 7) / 64),
// the pass-1 twiddle, from wherever the caller keeps it; t2r / t2i[r] = exp(-2 pi i r lane / 512).
template <typename TW1>
__device__ __forceinline__ void fft512_passes(cd (&v)[8], double* re, double* im, TW1 tw1, const double (&t2r)[8], const double (&t2i)[8], int lane) {
    // pass 0 (Ns = 1): no twiddles; outputs to index lane*8 + r
    dft8(v);
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int i = padidx(lane * 8 + r); re[i] = v[r].x; im[i] = v[r].y; }
    __builtin_amdgcn_wave_barrier();
    // pass 1 (Ns = 8)
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int i = padidx(lane + 64 * r); v[r] = cd{re[i], im[i]}; }
#pragma unroll
    for (int r = 1; r < 8; ++r) { const cd t = tw1(r); v[r] = cmulc(v[r], t.x, t.y); }
    dft8(v);
    __builtin_amdgcn_wave_barrier();
    {
        const int j0 = (lane >> 3) * 64 + (lane & 7);
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int i = padidx(j0 + 8 * r); re[i] = v[r].x; im[i] = v[r].y; }
    }
    __builtin_amdgcn_wave_barrier();
    // pass 2 (Ns = 64): outputs X[lane + 64 r] stay in registers
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int i = padidx(lane + 64 * r); v[r] = cd{re[i], im[i]}; }
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmulc(v[r], t2r[r], t2i[r]);
    dft8(v);
}

// every twiddle in registers
struct Fft512 {
    double t1r[8], t1i[8], t2r[8], t2i[8];
    __device__ __forceinline__ void init(int lane) {
#pragma unroll
        for (int r = 1; r < 8; ++r) {
            sincospi(-2.0 * (double)(r * (lane & 7)) / 64.0, &t1i[r], &t1r[r]);      // pass 1 (Ns = 8): exp(-2 pi i r k / 64), k = lane & 7
            sincospi(-2.0 * (double)(r * lane) / 512.0, &t2i[r], &t2r[r]);           // pass 2 (Ns = 64): exp(-2 pi i r lane / 512)
        }
    }
    __device__ __forceinline__ void run(cd (&v)[8], double* re, double* im, int lane) const {
        fft512_passes(v, re, im, [&](int r) { return cd{t1r[r], t1i[r]}; }, t2r, t2i, lane);
    }
};

// The same transform with the pass-1 twiddles read from an LDS table t1l[(lane & 7) * 8 + r] = exp(-2 pi i r (lane & 7) / 64) (they depend on
// lane & 7 only): 28 registers less per wave (three waves per SIMD: stft1024_walk_kernel, OCC3)
struct Fft512L {
    double t2r[8], t2i[8];
    __device__ __forceinline__ void init(int lane) {
#pragma unroll
        for (int r = 1; r < 8; ++r) sincospi(-2.0 * (double)(r * lane) / 512.0, &t2i[r], &t2r[r]);
    }
    __device__ __forceinline__ void run(cd (&v)[8], double* re, double* im, int lane, const double2* t1l) const {
        fft512_passes(v, re, im, [&](int r) { const double2 t = t1l[(lane & 7) * 8 + r]; return cd{t.x, t.y}; }, t2r, t2i, lane);
    }
};

// The float transform of the fp32-arithmetic walks; z: the wave's exchange buffer of 512 + 64 (re, im) slots, one 8-byte slot per point,
// padded like the double buffers.  The same three passes WRITTEN OUT: run through fft512_passes (with the exchange as a parameter) the
// float kernels compile to other instructions and register counts than these.
struct Fft512F {
    float t1r[8], t1i[8], t2r[8], t2i[8];
    __device__ __forceinline__ void init(int lane) {
#pragma unroll
        for (int r = 1; r < 8; ++r) {
            double sn, cs;
            sincospi(-2.0 * (double)(r * (lane & 7)) / 64.0, &sn, &cs); t1r[r] = (float)cs; t1i[r] = (float)sn;
            sincospi(-2.0 * (double)(r * lane) / 512.0, &sn, &cs); t2r[r] = (float)cs; t2i[r] = (float)sn;
        }
    }
    __device__ __forceinline__ void run(cf (&v)[8], cf* z, int lane) const {
        dft8(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) z[padidx(lane * 8 + r)] = v[r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = z[padidx(lane + 64 * r)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmulc(v[r], t1r[r], t1i[r]);
        dft8(v);
        __builtin_amdgcn_wave_barrier();
        {
            const int j0 = (lane >> 3) * 64 + (lane & 7);
#pragma unroll
            for (int r = 0; r < 8; ++r) z[padidx(j0 + 8 * r)] = v[r];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = z[padidx(lane + 64 * r)];
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmulc(v[r], t2r[r], t2i[r]);
        dft8(v);
    }
};

}  // namespace dvae

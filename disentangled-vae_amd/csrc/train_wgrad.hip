// Weight-gradient and optimizer kernels of the fused train step (include/dvae_train.h: launches two and three; train_fused.hip has the
// host side, wgrad_types.hpp the tables it fills and the launchers it calls).
//
// wgrad kernel: dW tile[32 out x 32 in] = sum over frames of dPre^T * In, both operands read from
// the [feature][frame] stash with 16-byte loads (frame = MFMA k index), 4 tiles per workgroup,
// the frame axis cut into `ksplit` slabs that the apply kernel sums in a fixed order
// (deterministic: no atomics anywhere).  Bias gradients ride along as one extra MFMA against a
// constant-one fragment.
#include <type_traits>
#include "fused_tiles.hpp"
#include "rows_common.hpp"
#include "apply_common.hpp"
#include "wgrad_types.hpp"
#include "../../include/dvae_train.h"

namespace dvae {
namespace fused {

// ---------------------------------------------------------------------------------------------
// One wave = one 2x2 group of 32x32 MFMA tiles (64 output features x 64 input features of one
// layer): per k-step it loads 2 + 2 operand fragments and issues 4 MFMAs, halving the bytes per
// FLOP of a single-tile wave.  Missing halves (odd tile counts, 16-row heads) are null.
template <typename P, bool A1, bool B1>
__device__ __forceinline__ void wgrad_body(const GroupDesc& d, int64_t kbeg, int64_t kend, int64_t Bp, int64_t spl, float* __restrict__ slab,
                                           int l31, int h) {
    typedef typename P::T T;
    typedef typename P::Frag Frag;
    constexpr int E = P::E, KS = P::KSTEP, NP = P::NP;
    const int lane = h * 32 + l31;
    constexpr int FB = 64 * E;                              // elements per (feature tile, k-step) block
    const T* a0p = (const T*)d.A[0] + lane * E;
    const T* a1p = A1 ? (const T*)d.A[1] + lane * E : a0p;
    const T* b0p = (const T*)d.Bm[0] + lane * E;
    const T* b1p = B1 ? (const T*)d.Bm[1] + lane * E : b0p;
    const bool bias0 = d.bias_off[0] >= 0, bias1 = A1 && d.bias_off[1] >= 0;
    f32x16 c00, c01, c10, c11, cb0, cb1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { c00[i] = 0.f; c01[i] = 0.f; c10[i] = 0.f; c11[i] = 0.f; cb0[i] = 0.f; cb1[i] = 0.f; }
    const Frag one = P::ones();
    const int64_t sbeg = kbeg / KS, send = kend / KS;       // k-steps of this frame slice
    // The stash was written once by the previous kernel: these are cold HBM/MALL reads (~2 us round trip).
    // A ring of RD k-steps per operand keeps 4 * RD (x planes) 1-KB loads in flight per wave; the slot an MFMA group has
    // consumed is re-requested RD steps ahead (clamped on the last lap: a harmless reload, no branch).
    constexpr int RD = P::WRING;
    Frag a0[RD][NP], a1[RD][NP], b0[RD][NP], b1[RD][NP];
    auto ldp = [&](Frag (&f)[NP], const T* p, int64_t sk) {
        f[0] = *reinterpret_cast<const Frag*>(p + sk * FB);
        if constexpr (NP == 2) f[1] = *reinterpret_cast<const Frag*>(p + spl + sk * FB);
    };
#pragma unroll
    for (int i = 0; i < RD; ++i) {
        int64_t sk = sbeg + i; sk = sk < send ? sk : send - 1;
        ldp(a0[i], a0p, sk);
        ldp(b0[i], b0p, sk);
        if (A1) ldp(a1[i], a1p, sk);
        if (B1) ldp(b1[i], b1p, sk);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
    for (int64_t sk = sbeg; sk < send; sk += RD) {
#pragma unroll
        for (int i = 0; i < RD; ++i) {
            if (sk + i < send) {                            // wave-uniform: slices are multiples of RD steps except the tail
                mmap<P>(c00, a0[i], b0[i]);
                if (B1) mmap<P>(c01, a0[i], b1[i]);
                if (A1) mmap<P>(c10, a1[i], b0[i]);
                if (A1 && B1) mmap<P>(c11, a1[i], b1[i]);
                if (bias0) { P::mma(cb0, a0[i][0], one); if constexpr (NP == 2) P::mma(cb0, a0[i][1], one); }
                if (A1) { if (bias1) { P::mma(cb1, a1[i][0], one); if constexpr (NP == 2) P::mma(cb1, a1[i][1], one); } }
            }
            int64_t sn = sk + RD + i; sn = sn < send ? sn : send - 1;
            ldp(a0[i], a0p, sn);
            ldp(b0[i], b0p, sn);
            if (A1) ldp(a1[i], a1p, sn);
            if (B1) ldp(b1[i], b1p, sn);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = feat_of(r, h);
        if (row < d.mvalid[0]) {
            const bool hi = d.split16 && row >= 16;
            const int rr = hi ? row - 16 : row;
            const int ldo = hi ? d.ldo_hi : d.ldo[0];
            if (l31 < d.nvalid[0]) slab[(hi ? d.out_off_hi[0] : d.out_off[0][0]) + (int64_t)rr * ldo + l31] = c00[r];
            if (B1) { if (l31 < d.nvalid[1]) slab[(hi ? d.out_off_hi[1] : d.out_off[0][1]) + (int64_t)rr * ldo + l31] = c01[r]; }
            if (bias0 && l31 == 0) slab[(hi ? d.bias_off_hi : d.bias_off[0]) + rr] = cb0[r];
        }
        if (A1) {
            if (row < d.mvalid[1]) {
                if (l31 < d.nvalid[0]) slab[d.out_off[1][0] + (int64_t)row * d.ldo[1] + l31] = c10[r];
                if (B1) { if (l31 < d.nvalid[1]) slab[d.out_off[1][1] + (int64_t)row * d.ldo[1] + l31] = c11[r]; }
                if (bias1 && l31 == 0) slab[d.bias_off[1] + row] = cb1[r];
            }
        }
    }
}

// grid.x = workgroups * ksplit with the k-slice as the FAST index: consecutive workgroups (dealt
// round-robin to the 8 XCDs) work on different frame slices, so each XCD's L2 mostly holds one
// slice of the stash.  blockDim.x / 64 groups per workgroup.
#ifndef DVAE_WGRAD_OCC
#define DVAE_WGRAD_OCC 1
#endif
template <typename P>
__global__ __launch_bounds__(256, DVAE_WGRAD_OCC) void wgrad_kernel(const GroupDesc* __restrict__ groups, int ngroups, int ksplit, int64_t Bp,
                                                    int64_t spl, int64_t kper, float* __restrict__ slabs, int64_t slab_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int slice = blockIdx.x % ksplit, wg = blockIdx.x / ksplit;
    const int gi = wg * (blockDim.x >> 6) + wave;
    if (gi >= ngroups) return;
    const GroupDesc d = groups[gi];
    const int64_t kbeg = (int64_t)slice * kper;
    int64_t kend = kbeg + kper;
    if (kend > Bp) kend = Bp;
    float* slab = slabs + (int64_t)slice * slab_stride;
    const bool a1 = d.A[1] != nullptr, b1 = d.Bm[1] != nullptr;
    if (a1 && b1) wgrad_body<P, true, true>(d, kbeg, kend, Bp, spl, slab, l31, h);
    else if (a1) wgrad_body<P, true, false>(d, kbeg, kend, Bp, spl, slab, l31, h);
    else if (b1) wgrad_body<P, false, true>(d, kbeg, kend, Bp, spl, slab, l31, h);
    else wgrad_body<P, false, false>(d, kbeg, kend, Bp, spl, slab, l31, h);
}
// ---------------------------------------------------------------------------------------------
// Weight gradients, workgroup-blocked: one 256-thread workgroup owns a 4 x 4 block of 32 x 32 tiles (128 output x 128 input
// features of one layer), wave (wr, wc) the 2 x 2 group {2wr, 2wr+1} x {2wc, 2wc+1} of it.  The block's 4 + 4 operand tiles
// are staged ONCE per k-step in LDS and shared by the four waves: the fragment-major stash tile of one k-step is 1 KB in
// exactly the lane-linear order a direct-to-LDS load writes (LDS address = wave-uniform base + lane * 16), so a fragment
// costs one `global_load_lds_dwordx4` and no registers.  A ring of NSTG stages x 2 k-steps keeps (NSTG - 1) stages in flight
// across one raw workgroup barrier per stage (counted vmcnt, never 0: cdna_hip_programming.md "Pipelining across barriers").
// Against the register-ring kernel above (every wave loads its own 2 + 2 fragments: each stash line crosses L2 -> CU 3.7
// times) the operand traffic halves and the in-flight bytes no longer cost registers.
#ifdef DVAE_DIAG
template <typename P> struct WgLds {
    static constexpr int KPS = 2;                                   // k-steps per stage
    static constexpr int NSTG = 4;
    static constexpr int FRAG = 1024;                               // bytes of one (tile, plane, k-step) fragment block
    static constexpr int STAGE = 8 * P::NP * KPS * FRAG;
    static constexpr int BYTES = NSTG * STAGE;
    static constexpr int LOADS = 2 * P::NP * KPS;                   // direct-to-LDS loads per wave and stage (one A slot + one B slot)
};

template <typename P>
__global__ __launch_bounds__(256, 1) void wgrad_lds_kernel(const BlockDesc* __restrict__ blocks, int nblocks, int ksplit, int64_t Bp,
                                                           int64_t spl, int64_t kper, float* __restrict__ slabs, int64_t slab_stride) {
    typedef typename P::T T;
    typedef typename P::Frag Frag;
    typedef WgLds<P> W;
    constexpr int E = P::E, KS = P::KSTEP, NP = P::NP, KPS = W::KPS, NSTG = W::NSTG;
    constexpr int FB = 64 * E;
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int slice = blockIdx.x % ksplit, bi = blockIdx.x / ksplit;
    if (bi >= nblocks) return;
    const BlockDesc& bd = blocks[bi];
    const GroupDesc d = bd.g[wave];
    const int64_t kbeg = (int64_t)slice * kper;
    int64_t kend = kbeg + kper;
    if (kend > Bp) kend = Bp;
    const int64_t sbeg = kbeg / KS, send = kend / KS;                 // k-steps of this frame slice
    const int nst = (int)((send - sbeg + KPS - 1) / KPS);             // stages
    float* slab = slabs + (int64_t)slice * slab_stride;
    // this wave stages tile slots `wave` (an A tile) and 4 + `wave` (a B tile); absent tiles reload the block's first A tile so
    // that every wave issues the same number of loads per stage (the vmcnt counts below are immediates)
    const T* src[2];
    src[0] = (const T*)(bd.At[wave] ? bd.At[wave] : bd.At[0]);
    src[1] = (const T*)(bd.Bt[wave] ? bd.Bt[wave] : bd.At[0]);
    auto issue = [&](int st) {                                        // stage st -> ring slot st % NSTG
        char* base = wsm + (st % NSTG) * W::STAGE;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                for (int kk = 0; kk < KPS; ++kk) {
                    int64_t sk = sbeg + (int64_t)st * KPS + kk; sk = sk < send ? sk : send - 1;   // past the slice: a harmless reload into a free slot
                    const T* gp = src[q] + pl * spl + sk * FB + lane * E;
                    char* lp = base + (((q * 4 + wave) * NP + pl) * KPS + kk) * W::FRAG;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)lp, 16, 0, 0);
                }
    };
    f32x16 c00, c01, c10, c11, cb0, cb1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { c00[i] = 0.f; c01[i] = 0.f; c10[i] = 0.f; c11[i] = 0.f; cb0[i] = 0.f; cb1[i] = 0.f; }
    const bool have = d.A[0] != nullptr;
    const bool A1 = d.A[1] != nullptr, B1 = d.Bm[1] != nullptr;
    const bool bias0 = have && d.bias_off[0] >= 0, bias1 = A1 && d.bias_off[1] >= 0;
    const Frag one = P::ones();
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int st = 0; st < NSTG - 1; ++st) issue(st);
    for (int st = 0; st < nst; ++st) {
        // stage st has landed for this wave's loads once at most (NSTG - 2) later stages are outstanding; the barrier extends that
        // to every wave's loads and says that everybody has finished reading stage st - 1, whose slot the next issue overwrites
        if constexpr (W::LOADS * (NSTG - 2) == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if constexpr (W::LOADS * (NSTG - 2) == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        issue(st + NSTG - 1);
        const char* base = wsm + (st % NSTG) * W::STAGE;
#pragma unroll
        for (int kk = 0; kk < KPS; ++kk) {
            if (sbeg + (int64_t)st * KPS + kk >= send) break;         // wave-uniform tail
            auto frag = [&](int slot, int pl) -> Frag {
                return *reinterpret_cast<const Frag*>(base + ((slot * NP + pl) * KPS + kk) * W::FRAG + lane * 16);
            };
            Frag a0[NP], a1[NP], b0[NP], b1[NP];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) { a0[pl] = frag(2 * wr, pl); a1[pl] = frag(2 * wr + 1, pl); b0[pl] = frag(4 + 2 * wc, pl); b1[pl] = frag(5 + 2 * wc, pl); }
            if (have) {
                mmap<P>(c00, a0, b0);
                if (B1) mmap<P>(c01, a0, b1);
                if (A1) mmap<P>(c10, a1, b0);
                if (A1 && B1) mmap<P>(c11, a1, b1);
                if (bias0) { P::mma(cb0, a0[0], one); if constexpr (NP == 2) P::mma(cb0, a0[1], one); }
                if (bias1) { P::mma(cb1, a1[0], one); if constexpr (NP == 2) P::mma(cb1, a1[1], one); }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the clamped tail loads must land before the LDS is released
    if (!have) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = feat_of(r, h);
        if (row < d.mvalid[0]) {
            const bool hi = d.split16 && row >= 16;
            const int rr = hi ? row - 16 : row;
            const int ldo = hi ? d.ldo_hi : d.ldo[0];
            if (l31 < d.nvalid[0]) slab[(hi ? d.out_off_hi[0] : d.out_off[0][0]) + (int64_t)rr * ldo + l31] = c00[r];
            if (B1) { if (l31 < d.nvalid[1]) slab[(hi ? d.out_off_hi[1] : d.out_off[0][1]) + (int64_t)rr * ldo + l31] = c01[r]; }
            if (bias0 && l31 == 0) slab[(hi ? d.bias_off_hi : d.bias_off[0]) + rr] = cb0[r];
        }
        if (A1) {
            if (row < d.mvalid[1]) {
                if (l31 < d.nvalid[0]) slab[d.out_off[1][0] + (int64_t)row * d.ldo[1] + l31] = c10[r];
                if (B1) { if (l31 < d.nvalid[1]) slab[d.out_off[1][1] + (int64_t)row * d.ldo[1] + l31] = c11[r]; }
                if (bias1 && l31 == 0) slab[d.bias_off[1] + row] = cb1[r];
            }
        }
    }
}
#endif  // DVAE_DIAG
// ---------------------------------------------------------------------------------------------
// Weight gradients, third form (default): one 256-thread workgroup = one 4 x 4 block of 32 x 32 tiles (128 output x 128 input
// features of a layer) x one frame slice, ONE workgroup per CU.  EVERY wave owns the whole 4 x 4 block (256 accumulator
// registers: the kernel runs at one wave per SIMD and has 512) on a QUARTER of the slice's frames: per k-step a wave loads 4 + 4
// operand fragments and issues 16 tile products, so a byte pulled into the CU feeds twice the MFMAs of the 2 x 2 register-ring
// kernel above (the measured bound there: ~55 GB/s of operand fragments per CU, 335 MB per launch, at 2.6 x the MFMA time).
// The four partial blocks meet in LDS as a reduce-scatter in a fixed order (deterministic): wave w finishes and stores A row w.  Bias gradients are in-lane sums of the A fragments (a frame
// sum needs no MFMA: one fp32 register per A tile instead of a 16-register accumulator against a constant-one operand).
template <int I, int N, typename F>
__device__ __forceinline__ void static_for_w(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for_w<I + 1, N>(f); }
}

// gradient-slab stores of the workgroup k-split kernel as buffer stores with cache-policy bits (W4_SLAB_AUX: gfx950 buffer aux, 0 = plain,
// 16 = sc1 = write-through -- the slabs are read by the apply kernel: 73.1 -> 72.9 us per step, same box, alternating; non-temporal
// loads of the once-read B fragments, also tried: 26.8 -> 31.6 us for the kernel)
#ifndef W4_SLAB_AUX
#define W4_SLAB_AUX 16
#endif
// the ragged-tile and bias stores of the slabs: write-through like the full-tile buffer stores (the folded optimizer tail reads the
// slabs of other workgroups of the same launch and relies on every slab store being one)
__device__ __forceinline__ void slab_store(float* p, float v) {
#if W4_SLAB_AUX
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
template <typename P> struct Wg4 {
#ifndef DVAE_W4RING_X3
#define DVAE_W4RING_X3 2      // round 5, same box, alternating, three rounds: 25.6 us (2) against 27.2 (3) by hipEvent -- 32 instead of 48 KB per wave in flight
#endif
#ifndef DVAE_W4RING
#define DVAE_W4RING 4
#endif
    static constexpr int RD = P::NP == 2 ? DVAE_W4RING_X3 : DVAE_W4RING;      // k-steps of operand fragments in flight per wave
    static constexpr size_t BYTES = (size_t)(8 * 16) * 64 * 16 + 12 * 64 * 4;           // 8 exchange slots of one A row (4 tiles x 16 registers x 64 lanes x 4 B) + the bias sums
};

// NA x NB = tiles of the block this instantiation computes (absent tiles alias tile 0 and are masked at the store: their
// descriptors carry mvalid / nvalid 0).  Compile-time shapes keep every operand load unconditional: a load under a run-time
// branch makes hipcc's wait-count pass fall back to vmcnt(0) in front of the first MFMA of every k-step (the ring then holds one).
// BLO = false: the B tiles (labels) have no lo plane in this launch -- it is neither read nor multiplied
// BIAS = false: no A tile of the block carries bias rows (only a layer's first B column does): no frame sums of the A fragments
template <typename P, int NA, int NB, int RAW, bool BLO = true, bool BIAS = true>
__device__ __forceinline__ void wgrad4_body(const Block4& bd, const Block4* __restrict__ bdg, char* wsm, int slice, int64_t Bp, int64_t spl, int64_t kbeg, int64_t kend_,
                                            float* __restrict__ slabs, int64_t slab_stride, int lane, int wave, const RawIn& ri) {
    typedef typename P::T T;
    typedef typename P::Frag Frag;
    typedef Wg4<P> W;
    typedef const __attribute__((address_space(1))) char* gptr;
    typedef const __attribute__((address_space(1))) Frag* gfrag;
    // RAW: 0 = B tiles from the stash; 1 = from the fp32 input matrix by dword loads (any shape); 2 = from the input matrix through
    // this wave's LDS staging rows (four full tiles): 16 frames x 128 columns per k-step arrive as eight 1 KB row loads, are split
    // into (hi, lo) bf16, written as [frame][column] rows and read back transposed (ds_read_b64_tr_b16) into MFMA fragments.
    // Mode 1 needs 32 loads per k-step and overruns the 6-bit vmcnt (at most 63 loads in flight: 1.5 k-steps); mode 2 needs 16.
    constexpr int E = P::E, KS = P::KSTEP, NP = P::NP, RD = RAW == 2 ? 2 : W::RD;
    constexpr int64_t FBB = 64 * 16;                                     // bytes of one (feature tile, k-step) fragment block
    constexpr int SLD = 128 + 8, SPL = 16 * SLD;                         // staging rows: elements per frame row (odd number of 16-byte slots), per plane
    const int l31 = lane & 31, h = lane >> 5;
    // this wave's quarter of the slice's k-steps
    int64_t kend = kend_;
    if (kend > Bp) kend = Bp;
    const int64_t s0 = kbeg / KS, s1 = kend / KS;
    const int64_t nq = (s1 - s0 + 3) / 4;
    int64_t sbeg = s0 + (int64_t)wave * nq, send = sbeg + nq;
    if (send > s1) send = s1;
    if (sbeg > send) sbeg = send;
    gptr ap[NA], bp[NB];
    // NA == 4: wave w holds the A tiles rotated by w (local row i = A tile (i + w) % 4), so that "the row this wave finishes and
    // stores" is local row 0 for every wave and the reduce-scatter below is ONE instruction stream with compile-time register indices
    const int rot = NA == 4 ? wave : 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) { const void* q = NA == 4 ? bdg->At[(k + rot) & 3] : bd.At[k]; ap[k] = (gptr)(uintptr_t)(q ? q : bd.At[0]); }   // dynamic index: from the global copy (a scalar load), not a private-memory copy of bd
#pragma unroll
    for (int k = 0; k < NB; ++k) bp[k] = (gptr)(uintptr_t)(bd.Bt[k] ? bd.Bt[k] : bd.Bt[0]);
    const int64_t plb = spl * (int64_t)sizeof(T);                          // bytes between the hi and lo planes
    const unsigned loff = (unsigned)lane * 16u;
    // Stash-fed bodies (RAW == 0): the operand stream as buffer loads, the form of the rows kernel's weight stream (wstream.hpp) -- one
    // resource per operand matrix and plane in SGPRs, ONE per-lane offset (lane * 16) shared by every fragment, tile + k-step as the scalar
    // offset: no 64-bit VGPR address per fragment.  An operand matrix = the block's present tiles, contiguous stash rows (fill_tables lays a
    // block's tiles out in ascending rows, tile 0 first): the resource starts at tile 0 and its record count ends with the highest tile, so every
    // request -- the clamped reloads of the last k-step included -- is inside it by construction; nothing relies on the range check.
    constexpr bool BUF = RAW == 0;
    const unsigned tileb = (unsigned)(32 * Bp * (int64_t)sizeof(T));       // bytes of one tile's rows (launch_wgrad4 bounds Bp)
    __amdgpu_buffer_rsrc_t ars[NP], brs[NP];
    unsigned aoff[NA], boff[NB];
    if constexpr (BUF) {
        const gptr a0 = (gptr)(uintptr_t)bd.At[0], b0 = (gptr)(uintptr_t)bd.Bt[0];      // tile 0: the lowest rows
        unsigned am = 0, bm = 0;
#pragma unroll
        for (int k = 0; k < NA; ++k) { aoff[k] = (unsigned)(ap[k] - a0); am = aoff[k] > am ? aoff[k] : am; }
#pragma unroll
        for (int k = 0; k < NB; ++k) { boff[k] = (unsigned)(bp[k] - b0); bm = boff[k] > bm ? boff[k] : bm; }
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            ars[pl] = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(a0 + pl * plb), 0, __builtin_amdgcn_readfirstlane((int)(am + tileb)), 0x00020000);   // (hipcc takes the maximum with a vector instruction)
            brs[pl] = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(b0 + pl * plb), 0, __builtin_amdgcn_readfirstlane((int)(bm + tileb)), 0x00020000);
        }
    }
    f32x16 c[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) c[i][j][r] = 0.f;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    Frag a[RD][NA][NP], b[RAW == 1 ? 1 : (RAW == 2 ? 1 : RD)][RAW == 1 ? 1 : NB][NP];   // RAW == 2: b[0] = the fragments of the k-step being multiplied
    // RAW: the B fragments come from the fp32 input matrix itself -- lane (feature l31, frame half h) of tile j needs E consecutive
    // frames of ONE column: E dword loads, each wave-instruction two 128-byte row segments; split into (hi, lo) when consumed.
    // Frames past the batch repeat its last row (their dPre operand is zero), pad columns repeat the last column (never stored).
    float braw[RAW == 1 ? RD : 1][RAW == 1 ? NB : 1][E];
    f32x4 rawq[RAW == 2 ? RD : 1][RAW == 2 ? 8 : 1];                        // RAW == 2: row 2u + (lane >> 5), columns 4 (lane & 31) .. + 3 of the k-step's block
    typedef const __attribute__((address_space(1))) float* gflt;
    const gflt rsrc = (gflt)(uintptr_t)(RAW ? (bd.raw == 1 ? ri.x : ri.y) : nullptr);
    const int rld = RAW ? (bd.raw == 1 ? ri.ldx : ri.ldy) : 0;
    int rcolv[RAW == 1 ? NB : 1];
    if constexpr (RAW == 1) {
#pragma unroll
        for (int k = 0; k < NB; ++k) { const int cc = bd.rcol[k] + l31; rcolv[k] = cc < bd.rncols ? cc : bd.rncols - 1; }
    }
    T* const stg = reinterpret_cast<T*>(wsm) + wave * (SPL * NP);          // RAW == 2: this wave's staging rows
    const int rcol4 = RAW == 2 ? bd.rcol[0] + 4 * l31 : 0;
    auto load = [&](auto sc, int64_t sk) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
        const int64_t o = sk * FBB;
        const unsigned so = (unsigned)o;                                     // BUF: the k-step as the loads' scalar offset
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if constexpr (BUF) {
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) a[s][k][pl] = __builtin_bit_cast(Frag, __builtin_amdgcn_raw_buffer_load_b128(ars[pl], (int)loff, (int)(aoff[k] + so), 0));
            } else {
                a[s][k][0] = *(gfrag)(ap[k] + o + loff);
                if constexpr (NP == 2) a[s][k][1] = *(gfrag)(ap[k] + plb + o + loff);
            }
        }
        if constexpr (RAW == 1) {
            const int64_t f0 = sk * KS + h * E;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                int64_t fr = f0 + e; fr = fr < ri.B ? fr : ri.B - 1;
                const gflt rowp = rsrc + fr * rld;
#pragma unroll
                for (int k = 0; k < NB; ++k) braw[s][k][e] = rowp[rcolv[k]];
            }
        } else if constexpr (RAW == 2) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int64_t fr = sk * KS + 2 * u + h; fr = fr < ri.B ? fr : ri.B - 1;
                rawq[s][u] = reinterpret_cast<const __attribute__((address_space(1))) F4U*>(rsrc + fr * rld + rcol4)->v;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                b[s][k][0] = __builtin_bit_cast(Frag, __builtin_amdgcn_raw_buffer_load_b128(brs[0], (int)loff, (int)(boff[k] + so), 0));
                if constexpr (NP == 2 && BLO) b[s][k][1] = __builtin_bit_cast(Frag, __builtin_amdgcn_raw_buffer_load_b128(brs[NP - 1], (int)loff, (int)(boff[k] + so), 0));
            }
        }
    };
    auto fsum = [&](const Frag& f) __attribute__((always_inline)) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < E; ++q) t += (float)f[q];
        return t;
    };
    // RAW == 2: stage s of the raw ring -> (hi, lo) rows in LDS -> transposed fragments b[0][j]
    auto prepare = [&](auto sc) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
        if constexpr (RAW == 2) {
            typedef typename P::Pack4 Pack4;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                Pack4 ph, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ph[e] = P::cvt(rawq[s][u][e]); pl[e] = P::cvt(rawq[s][u][e] - (float)ph[e]); }
                T* const rowp = stg + (2 * u + h) * SLD + 4 * l31;
                *reinterpret_cast<Pack4*>(rowp) = ph;
                if constexpr (NP == 2) *reinterpret_cast<Pack4*>(rowp + SPL) = pl;
            }
            const int i16 = l31 & 15, q = i16 >> 2, pp = i16 & 3, cg = l31 >> 4;
            typedef short s16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int pln = 0; pln < NP; ++pln) {
                    const T* bpj = stg + pln * SPL + q * SLD + 32 * j + 16 * cg + 4 * pp;
                    const s16x4 r0 = lds_tr16(bpj + (8 * h) * SLD), r1 = lds_tr16(bpj + (8 * h + 4) * SLD);
                    const s16x8 raw8 = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
                    b[0][j][pln] = __builtin_bit_cast(Frag, raw8);
                }
        }
    };
    // timing ablations of the main loop (tools/r05/ab_libs.sh on variants built by tools/r05/mkvariant.sh; results are wrong under any of them): W4_NOMFMA = loads + bias sums only,
    // W4_NOFSUM = no bias sums, W4_NOLOAD = the ring is never refilled (MFMAs on the prologue's fragments), W4_NOEPI = no reduce-scatter / stores
    auto compute = [&](auto sc) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
#ifdef W4_NOMFMA
        if constexpr (RAW == 0) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                bs[i] += fsum(a[s][i][0]);
                if constexpr (NP == 2) bs[i] += fsum(a[s][i][1]);
#pragma unroll
                for (int j = 0; j < NB; ++j) { c[i][j][0] += (float)b[s][j][0][0]; if constexpr (NP == 2 && BLO) c[i][j][1] += (float)b[s][j][1][0]; }
            }
            return;
        }
#endif
        if constexpr (RAW == 2) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
#pragma unroll
                for (int j = 0; j < NB; ++j) mmap<P>(c[i][j], a[s][i], b[0][j]);
                if constexpr (BIAS) {
                    bs[i] += fsum(a[s][i][0]);
                    if constexpr (NP == 2) bs[i] += fsum(a[s][i][1]);
                }
            }
        } else if constexpr (RAW == 1) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                Frag bj[NP];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    bj[0][e] = P::cvt(braw[s][j][e]);
                    if constexpr (NP == 2) bj[1][e] = P::cvt(braw[s][j][e] - (float)bj[0][e]);
                }
#pragma unroll
                for (int i = 0; i < NA; ++i) mmap<P>(c[i][j], a[s][i], bj);
            }
            if constexpr (BIAS) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    bs[i] += fsum(a[s][i][0]);
                    if constexpr (NP == 2) bs[i] += fsum(a[s][i][1]);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
#pragma unroll
                for (int j = 0; j < NB; ++j) mmap<P>(c[i][j], a[s][i], b[s][j], BLO);
#ifndef W4_NOFSUM
                if constexpr (BIAS) {
                    bs[i] += fsum(a[s][i][0]);                           // bias gradient: frame sum of the A fragment (VALU in the MFMAs' shadow)
                    if constexpr (NP == 2) bs[i] += fsum(a[s][i][1]);
                }
#endif
            }
        }
    };
    // No branch around the loop (an empty range runs zero laps; its clamped prologue loads re-read the slice's last k-step): a
    // conditional region here makes every accumulator a phi of (zero, loop result) and costs a 256-register copy.
    {
        int64_t slast = (send > s0 ? send : s0 + 1) - 1;
        if (slast > Bp / KS - 1) slast = Bp / KS - 1;                     // a slice that starts at the batch's end: still a k-step of the matrix
        static_for_w<0, RD>([&](auto sc) {
            int64_t sk = sbeg + decltype(sc)::value; sk = sk < slast ? sk : slast;
            load(sc, sk);
        });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RAW == 2) prepare(std::integral_constant<int, 0>{});
#pragma unroll 1
        for (int64_t sk = sbeg; sk < send; sk += RD) {
            static_for_w<0, RD>([&](auto sc) {
                constexpr int s = decltype(sc)::value;
                if (sk + s < send) compute(sc);                         // wave-uniform
                int64_t sn = sk + RD + s; sn = sn < slast ? sn : slast;     // last lap: a harmless reload, no branch around a load
                if constexpr (RAW == 2) {
                    // the MFMAs of this k-step are in the pipe (their operands are read): stage the NEXT k-step's B tiles in their shadow
                    // -- its raw values are consumed before this slot's reload below overwrites the ring
                    prepare(std::integral_constant<int, (s + 1) % RD>{});
                }
#ifndef W4_NOLOAD
                load(sc, sn);
#else
                (void)sn;
#endif
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        if constexpr (RAW == 2) __syncthreads();                        // every wave is done with its staging rows: the reduce-scatter below reuses the LDS
    }
    // ---- the four partial blocks meet in LDS: a reduce-scatter in a fixed order (deterministic).  Wave w ends up with A tile row
    // w of the block (its local row 0) and stores it: a single wave storing 8 tiles with per-element address arithmetic took
    // 17 us (issue-bound), more than the main loop.
#ifdef W4_NOEPI
    {
        float t = bs[0] + bs[1] + bs[2] + bs[3];
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += c[i][j][r];
        if (t == 123.456f) slabs[0] = t;
        return;
    }
#endif
    constexpr int ROWQ = 4 * 4 * 64;                                      // f32x4 quads of one A row (4 tiles x 16 registers x 64 lanes)
    f32x4* const lds = reinterpret_cast<f32x4*>(wsm);
    float* const lbias = reinterpret_cast<float*>(lds + 8 * ROWQ);        // [dest wave][source order][lane]
    auto put_row = [&](auto ic, int slot) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                lds[slot * ROWQ + (j * 4 + q) * 64 + lane] = f32x4{c[i][j][4 * q], c[i][j][4 * q + 1], c[i][j][4 * q + 2], c[i][j][4 * q + 3]};
    };
    auto add_row0 = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = lds[slot * ROWQ + (j * 4 + q) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) c[0][j][4 * q + e] += v[e];
            }
    };
    typedef std::integral_constant<int, 0> I0; typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2; typedef std::integral_constant<int, 3> I3;
    if constexpr (NA == 1) {
        // one A row: waves 1-3 hand it to wave 0
        if (wave != 0) { put_row(I0{}, wave); lbias[wave * 64 + lane] = bs[0]; }
        __syncthreads();
        if (wave != 0) return;
        add_row0(1); add_row0(2); add_row0(3);
        bs[0] += lbias[64 + lane]; bs[0] += lbias[128 + lane]; bs[0] += lbias[192 + lane];
    } else {
        // round A: local rows 1, 2 go to waves (w + 1) % 4, (w + 2) % 4 (slot = 2 * destination + source order); round B: local row 3
        const int d1 = (wave + 1) & 3, d2 = (wave + 2) & 3, d3 = (wave + 3) & 3;
        put_row(I1{}, 2 * d1); put_row(I2{}, 2 * d2 + 1);
        lbias[(3 * d1 + 0) * 64 + lane] = bs[1]; lbias[(3 * d2 + 1) * 64 + lane] = bs[2]; lbias[(3 * d3 + 2) * 64 + lane] = bs[3];
        __syncthreads();
        add_row0(2 * wave); add_row0(2 * wave + 1);                         // from wave (w - 1) % 4, then from wave (w - 2) % 4
        __syncthreads();
        put_row(I3{}, d3);
        __syncthreads();
        add_row0(wave);                                                   // from wave (w - 3) % 4
        bs[0] += lbias[(3 * wave + 0) * 64 + lane]; bs[0] += lbias[(3 * wave + 1) * 64 + lane]; bs[0] += lbias[(3 * wave + 2) * 64 + lane];
    }
    // ---- store local row 0 = A tile `rot` of the block (descriptor fields of that tile: wave-uniform scalar loads)
    float* const slab = slabs + (int64_t)slice * slab_stride;
    const int mv = bdg->mvalid[rot], ldo = bdg->ldo[rot];
    const int64_t a_off = bdg->a_off[rot], bias_off = bdg->bias_off[rot];
    const bool split = rot == 0 && bd.split16;
    if (mv == 32 && !split) {
        // full tile rows: one exec region per tile, scalar row address + a per-lane 32-bit offset.  (Round 3 tried 16-byte stores -- the
        // tile turned through this wave's LDS slot so that a lane holds four consecutive columns, 4 stores of 1 KB per tile instead of
        // 16 of 256 B: 28.1 us against 27.2 us for the kernel, same box, alternating.  The dword form stays.)
        const unsigned lo = (unsigned)(4 * h * ldo + l31);
#if W4_SLAB_AUX
        const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(slab + a_off, 0, 0x7fffffff, 0x00020000);   // this A row's 32 tensor rows
#endif
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (l31 < bd.nvalid[j]) {
                float* const t0 = slab + a_off + bd.bcol[j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
#if W4_SLAB_AUX
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c[0][j][r]), srs, (int)(4u * lo), (int)(4u * (unsigned)(bd.bcol[j] + ((r & 3) + 8 * (r >> 2)) * ldo)), W4_SLAB_AUX);
#else
                    float* const rowp = t0 + (int64_t)((r & 3) + 8 * (r >> 2)) * ldo;     // wave-uniform
                    rowp[lo] = c[0][j][r];
#endif
                }
                (void)t0;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = feat_of(r, h);
                if (row < mv && l31 < bd.nvalid[j]) {
                    const bool hi = split && row >= 16;
                    const int rr = hi ? row - 16 : row;
                    const int ld = hi ? bd.ldo_hi : ldo;
                    slab_store(&slab[(hi ? bd.a_off_hi : a_off) + (int64_t)rr * ld + bd.bcol[j] + l31], c[0][j][r]);
                }
            }
        }
    }
    const float tot = bs[0] + __shfl_xor(bs[0], 32, 64);                  // the two frame halves of feature row l31
    if (h == 0 && l31 < mv && bias_off >= 0) {
        const bool hi = split && l31 >= 16;
        slab_store(&slab[hi ? bd.bias_off_hi + (l31 - 16) : bias_off + l31], tot);
    }
}
// ---------------------------------------------------------------------------------------------
// ---- the optimizer step folded into the tail of the weight-gradient kernel (a train step = two launches).
// Every (slice, block) workgroup, once its partial block is in its slab, arrives at the block's counter and waits until all `ksplit`
// slices of the block have arrived (the grid is one round of workgroups, all resident: the host folds only when the grid fits the CUs;
// the wait is bounded and raises the error word instead of hanging).  Then the ksplit * 4 waves share the block's parameters: a wave
// takes whole tensor rows (row u of the block's 128, u = wave id, + ksplit * 4, ...; units 128-131: the bias rows), a lane two elements
// of a row; each element = the slab sum in slab order (the very additions of apply_kernel), Adam, the weight-copy refresh.  Workgroup 0
// also turns the rows kernel's partial sums into the loss scalars.
// Counters (unsigned words of the flag header): [2] error (sticky), [16 + b] arrivals of block b -- never reset: launch number n of a
// workspace (counted by the host, fold_seq) waits for ksplit * n.  One fire-and-forget atomic and the polling loads are all the
// synchronisation a workgroup pays (returning atomics cost a device-scope round trip each: 2 us on the critical path).
#ifdef DVAE_DIAG
template <typename T, int NP>
__device__ __forceinline__ void fold_tail(const ApplyArgs& g, const FoldArgs& fa, const Block4& bd, const Block4* __restrict__ bdg, int bi, int slice,
                                          int ks, int lane, int wave, char* wsm) {
    int* const flag = reinterpret_cast<int*>(wsm);                     // the reduce-scatter is over: the exchange slots are free
    // This wave's slab stores are complete, i.e. visible device-wide: they are write-through (sc1) stores, so waiting for them is
    // enough.  (A release fence writes back the XCD's whole L2 and the matching acquire invalidates it -- 960 times per launch: the
    // kernel took 75 us instead of 28.)
#if W4_SLAB_AUX
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(fa.cnt + 16 + bi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned polls = 0;
        int ok = 1;
        while ((int)(__hip_atomic_load(fa.cnt + 16 + bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - fa.target) < 0) {
            __builtin_amdgcn_s_sleep(1);
            if (++polls > fa.max_polls) { ok = 0; break; }
        }
        if (!ok) __hip_atomic_store(fa.cnt + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag[0] = ok;
    }
    __syncthreads();
    const int ok = flag[0];
#if !W4_SLAB_AUX
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
#ifndef FOLD_DIAG
#define FOLD_DIAG 0      // timing diagnostics (wrong results): 1 = wait only, 2 = wait + loads + stores of p only, 3 = no loss scalars
#endif
    if (ok && FOLD_DIAG != 1) {
        int nb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (bd.Bt[k] != nullptr) nb = k + 1;
        const int gw = slice * 4 + wave, nw = ks * 4;
        constexpr int UB = 4;                                          // units per batch: their loads are all in flight together
        for (int u0 = gw; u0 < 132; u0 += UB * nw) {
            int64_t idx[UB][2];
            float pi[UB][2], mo[UB][2], vo[UB][2], gi[UB][2];
            int tq[UB][2];                                             // wave-uniform: a unit is a row of ONE tensor (two for the heads' bias unit: one per q)
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                const int u = u0 + b * nw;                             // wave-uniform
                idx[b][0] = idx[b][1] = -1;
                tq[b][0] = tq[b][1] = 0;
                if (u < 128) {
                    const int rot = u >> 5, rr = u & 31;
                    if (rr < bdg->mvalid[rot]) {
                        const bool hi = rot == 0 && bd.split16 && rr >= 16;
                        const int64_t base = hi ? bd.a_off_hi + (int64_t)(rr - 16) * bd.ldo_hi : bdg->a_off[rot] + (int64_t)rr * bdg->ldo[rot];
                        tq[b][0] = tq[b][1] = hi ? bd.wt_hi : bdg->wt[rot];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int j = (lane >> 5) + 2 * q, l = lane & 31;     // columns lane and lane + 64 of the block's 128
                            if (j < nb && l < bdg->nvalid[j]) idx[b][q] = base + bdg->bcol[j] + l;
                        }
                    }
                } else if (u < 132) {
                    const int rot = u - 128;
                    const int64_t bo = bdg->bias_off[rot];
                    const int mv = bdg->mvalid[rot];
                    if (bo >= 0) {
                        const bool split = rot == 0 && bd.split16;
                        tq[b][0] = bdg->bt[rot]; tq[b][1] = bd.bt_hi;
                        if (lane < (split ? 16 : 32) && lane < mv) idx[b][0] = bo + lane;
                        if (split && lane >= 16 && lane < 32 && lane < mv) idx[b][1] = bd.bias_off_hi + (lane - 16);
                    }
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int64_t i = idx[b][q] >= 0 ? idx[b][q] : 0;  // masked lanes read element 0 (no branch around the loads)
                    pi[b][q] = g.p[i]; mo[b][q] = g.m[i]; vo[b][q] = g.v[i];
                    gi[b][q] = slab_sum_at<W4_SLAB_AUX != 0>(g, i);               // the other slices' slabs, not this XCD's stale L2 lines
                }
            }
#pragma unroll
            for (int b = 0; b < UB; ++b)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const TensorDesc& d = g.tensors[tq[b][q]];                     // uniform address: scalar loads
                    if (FOLD_DIAG == 2) { if (idx[b][q] >= 0) g.p[idx[b][q]] = pi[b][q] + mo[b][q] + vo[b][q] + gi[b][q]; continue; }
                    if (idx[b][q] >= 0) apply_element<T, true, NP>(g, idx[b][q], d, pi[b][q], mo[b][q], vo[b][q], gi[b][q]);
                }
        }
    }
    if (blockIdx.x == 0 && g.losses3 != nullptr && FOLD_DIAG == 0) {   // workgroup 0 (always a participant): loss scalars
        __syncthreads();
        finalize_losses(g, reinterpret_cast<double (*)[4]>(wsm + 64));
        // a wait that ran out (error word set, sticky): parameters were not all updated -- the loss says so
        if (threadIdx.x == 0 && __hip_atomic_load(fa.cnt + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) g.losses3[0] = __builtin_nanf("");
    }
    if (!ok && threadIdx.x == 0 && g.losses3 != nullptr) g.losses3[0] = __builtin_nanf("");
}
#endif  // DVAE_DIAG

template <typename P>
__global__ __launch_bounds__(256, 1) void wgrad4_kernel(const Block4* __restrict__ blocks, const W4Item* __restrict__ items, int ksplit, int64_t Bp,
                                                        int64_t spl, float* __restrict__ slabs, int64_t slab_stride,
                                                        const RawIn ri, int use_raw, const unsigned* __restrict__ ylo_epoch, unsigned launch_id,
                                                        const ApplyArgs fold_apply, const FoldArgs fold, int fin_block, const unsigned* fin_err) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // deferred optimizer step (apply_common.hpp): the step's loss scalars no longer come from an optimizer launch -- ONE extra workgroup of
    // this launch (it follows the rows kernel, whose partial sums are complete) reduces them, on a CU the weight-gradient blocks leave free
    if (fin_block >= 0 && (int)blockIdx.x == fin_block) {
        finalize_losses(fold_apply, reinterpret_cast<double (*)[4]>(wsm));
        if (threadIdx.x == 0 && fin_err != nullptr && __hip_atomic_load(fin_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
            fold_apply.losses3[0] = __builtin_nanf("");              // a bounded wait of the rows kernel ran out: the update was not complete
        return;
    }
    // Workgroup -> (block, slice, frames): the host's item table (w4_build_items).  Workgroup i runs on XCD i % 8 (speed only): the table
    // keeps the items that read the same stash lines -- the blocks of a layer over the same frames -- on one XCD, and cuts every block into
    // as many slices as its cost per k-step asks for, so that all workgroups of the one round finish together.
    const W4Item it = items[blockIdx.x];
    if (it.block < 0) return;
    const int slice = it.slice, bi = it.block;
    const Block4 bd = blocks[bi];                                       // by value: wave-uniform, lives in SGPRs (a reference would be re-read after every slab store)
    int na = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (bd.At[k] != nullptr) na = k + 1; if (bd.Bt[k] != nullptr) nb = k + 1; }
    // (BIAS = false bodies -- no frame sums of the A fragments in blocks that carry no bias rows -- exist as a template parameter and are NOT
    // instantiated: built in round 5, the kernel with them took 34.3 us against 25.3 without, same box, alternating (their loops are
    // tighter, 158 against 394 instructions per two k-steps, but hipcc spills 250 - 650 registers around them; tools/r05/w4_ab2.sh))
#define W4_GO_(NA_, NB_, RAW_, BLO_) wgrad4_body<P, NA_, NB_, RAW_, BLO_, true>(bd, blocks + bi, wsm, slice, Bp, spl, it.kbeg, it.kend, slabs, slab_stride, lane, wave, ri)
#define W4_GO(NA_, NB_, RAW_) W4_GO_(NA_, NB_, RAW_, true)
    bool raw = false;
    if constexpr (sizeof(typename P::T) == 2) raw = (use_raw & bd.raw) != 0;      // input-matrix B tiles (16-bit operand policies only); use_raw bit 0: x, bit 1: labels
    if (raw) {
        if constexpr (sizeof(typename P::T) == 2) {
            if (nb == 4 && bd.rcol[0] + 128 <= bd.rncols) W4_GO(4, 4, 2);      // four full tiles: through the LDS staging rows
            else if (nb == 1) W4_GO(4, 1, 1);
            else if (nb == 2) W4_GO(4, 2, 1);
            else W4_GO(4, 4, 1);
        }
    } else if (sizeof(typename P::T) == 2 && P::NP == 2 && bd.raw == 2 && ylo_epoch != nullptr && *ylo_epoch != launch_id) {
        // label-fed blocks of a launch whose label tiles all fit one bf16 plane (binary labels): hi plane only
        if (nb == 1) W4_GO_(4, 1, 0, false);
        else if (nb == 2) W4_GO_(4, 2, 0, false);
        else W4_GO_(4, 4, 0, false);
    } else if (na == 1) {
        if (nb == 1) W4_GO(1, 1, 0);
        else if (nb == 2) W4_GO(1, 2, 0);
        else W4_GO(1, 4, 0);
    } else {
        if (nb == 1) W4_GO(4, 1, 0);
        else if (nb == 2) W4_GO(4, 2, 0);
        else W4_GO(4, 4, 0);
    }
#undef W4_GO
#undef W4_GO_
#ifndef W4_FOLD
#ifdef DVAE_DIAG
#define W4_FOLD 1      // 0: the folded optimizer tail compiled out (A/B of what its presence costs the main loop)
#else
#define W4_FOLD 0      // product build: no folded tail
#endif
#endif
#if W4_FOLD
    if (fold.cnt != nullptr) fold_tail<typename P::T, P::NP>(fold_apply, fold, bd, blocks + bi, bi, slice, ksplit, lane, wave, wsm);
#endif
}
// sum of up to NS slabs at element i: every load issued before the first addition (a run-time loop makes each addition wait for
// its own load: ten dependent round trips), additions in slab order (deterministic)
template <int NS>
__device__ __forceinline__ float slab_total(const float* __restrict__ slabs, int64_t i, int nslabs, int64_t stride) {
    float part[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) part[k] = slabs[(int64_t)(k < nslabs ? k : 0) * stride + i];
    float t = part[0];
#pragma unroll
    for (int k = 1; k < NS; ++k) if (k < nslabs) t += part[k];
    return t;
}
__device__ __forceinline__ float slab_total_any(const float* __restrict__ slabs, int64_t i, int nslabs, int64_t stride) {
    if (nslabs <= 8) return slab_total<8>(slabs, i, nslabs, stride);
    if (nslabs <= 16) return slab_total<16>(slabs, i, nslabs, stride);
    float s = slabs[i];
    for (int k = 1; k < nslabs; ++k) s += slabs[k * stride + i];
    return s;
}

// dst = (accumulate ? dst : 0) + sum of the slabs (fixed order: deterministic)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slabs, int64_t n, int nslabs, int64_t stride, float* __restrict__ dst, int accumulate) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s = slab_total_any(slabs, i, nslabs, stride);
        dst[i] = accumulate ? dst[i] + s : s;
    }
}

__global__ __launch_bounds__(256) void slab_reduce_kernel(float* __restrict__ slabs, int64_t n, int nslabs, int64_t stride) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        slabs[i] = slab_total_any(slabs, i, nslabs, stride);
}

// One thread per parameter over the flat buffer (every load independent); chunk_tensor maps each
// 64-float chunk to its tensor (tensors start on 64-float boundaries), 255 = alignment padding.
// The block after the last parameter block finalises the loss scalars.
template <typename T, bool ADAM, int NP = 1>
__global__ __launch_bounds__(256) void apply_kernel(const ApplyArgs g) {
    if (blockIdx.x == gridDim.x - 1) {                    // loss finalisation block
        if (!ADAM || g.losses3 == nullptr) return;
        __shared__ double red[4][4];
        finalize_losses(g, red);
        return;
    }
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.n_params) return;
    // Everything this thread reads sits at flat index idx (alignment padding between tensors included, the buffers
    // are allocated whole): request it all FIRST, so the two dependent table lookups below (chunk -> tensor ->
    // descriptor) overlap the one HBM round trip instead of preceding it.
    const float pi = g.p[idx];
    float m_old = 0.f, v_old = 0.f, gi = 0.f;
    if (ADAM) {
        m_old = g.m[idx]; v_old = g.v[idx];
        gi = slab_sum_at(g, idx);
    }
    // a wave covers one 64-float chunk: its tensor and the descriptor are wave-uniform, fetched by scalar loads
    const int t = g.chunk_tensor[__builtin_amdgcn_readfirstlane((int)(idx >> 6))];
    if (t == 255) return;
    const TensorDesc d = g.tensors[t];
    apply_element<T, ADAM, NP>(g, idx, d, pi, m_old, v_old, gi);
}

#ifdef DVAE_DIAG
// The optimizer step by UNITS (apply_common.hpp: defer_unit -- 8 rows x 32 columns of one weight matrix per wave, whole-line loads of
// parameters / moments / slabs, the kernel-layout copies as whole 8- and 16-byte pieces through the transposing LDS read): the same
// element arithmetic as apply_kernel on the same slab sums (bit-identical, tested), a quarter of its instructions, no lone 2-byte stores.
// One unit per wave; the block after the last unit block finalises the loss scalars.  bf16 / bf16x3 copies.
template <typename T, int NP>
__global__ __launch_bounds__(256) void apply_units_kernel(const ApplyArgs g, const DeferTask* __restrict__ tasks, int nunits) {
    __shared__ __attribute__((aligned(16))) char sm[4 * DeferLds<T, NP>::wave_elems * sizeof(T) > 128 ? 4 * DeferLds<T, NP>::wave_elems * sizeof(T) : 128];
    if (blockIdx.x == gridDim.x - 1) {
        if (g.losses3 == nullptr) return;
        finalize_losses(g, reinterpret_cast<double (*)[4]>(sm));
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // unit un of the launch: consecutive units of a tile on different workgroups (a tile's four units share lines at odd row lengths)
    const int un = wave * ((int)gridDim.x - 1) + (int)blockIdx.x;
    if (un >= nunits) return;
    T* const tile = reinterpret_cast<T*>(sm) + wave * DeferLds<T, NP>::wave_elems;
    defer_unit<T, NP, false>(g, tasks[un >> 2], un & 3, tile, lane);
}
#endif  // DVAE_DIAG

// ---------------------------------------------------------------------------------------------
// launchers (declared in wgrad_types.hpp)
int launch_wgrad_ring(int precision, const GroupDesc* groups, int ngroups, const WgradArgs& a, int gpw, hipStream_t s) {
    const dim3 g2((unsigned)(((ngroups + gpw - 1) / gpw) * a.ksplit));
    with_policy(precision, [&](auto pol) {
        hipLaunchKernelGGL((wgrad_kernel<decltype(pol)>), g2, dim3(64 * gpw), 0, s, groups, ngroups, a.ksplit, a.Bp, a.spl, a.kper, a.slabs, a.slab_stride);
    });
    DVAE_LAUNCH_OK("wgrad_kernel");
    return 0;
}

int launch_wgrad_lds(int precision, const BlockDesc* blocks, int nblocks, const WgradArgs& a, hipStream_t s) {
#ifdef DVAE_DIAG
    const int dev = current_device();
    const dim3 g3((unsigned)(nblocks * a.ksplit));
    auto lds = [&](auto pol) -> int {      // (two policies: there is no fp32 form of this kernel)
        using P = decltype(pol);
        static bool attr_done[64] = {};
        if (!attr_done[dev]) { DVAE_HIP(hipFuncSetAttribute((const void*)wgrad_lds_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, WgLds<P>::BYTES)); attr_done[dev] = true; }
        hipLaunchKernelGGL((wgrad_lds_kernel<P>), g3, dim3(256), WgLds<P>::BYTES, s, blocks, nblocks, a.ksplit, a.Bp, a.spl, a.kper, a.slabs, a.slab_stride);
        return 0;
    };
    const int rc = precision == DVAE_PREC_BF16X3 ? lds(PolX3{}) : lds(PolBF16{});
    if (rc) return rc;
    DVAE_LAUNCH_OK("wgrad_lds_kernel");
    return 0;
#else
    set_error("train_grads: DVAE_WGRAD=lds exists in the diagnostic build only (build.py --diag)");
    return DVAE_E_UNSUPPORTED;
#endif
}

int launch_wgrad4(int precision, const Wgrad4Args& a, int grid, hipStream_t s) {
    const int dev = current_device();
    // the operand stream addresses a block's four tiles (32 rows x Bp frames each) with 32-bit byte offsets into one buffer resource
    if (a.Bp > ((int64_t)1 << 22)) { set_error("train_grads: more than 4194304 frames per step"); return DVAE_E_UNSUPPORTED; }
    const int rc = with_policy(precision, [&](auto pol) -> int {
        using P = decltype(pol);
        static bool attr_done[64] = {};      // per device: the attribute belongs to the device's copy of the code object
        if (!attr_done[dev]) { DVAE_HIP(hipFuncSetAttribute((const void*)wgrad4_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Wg4<P>::BYTES)); attr_done[dev] = true; }
        hipLaunchKernelGGL((wgrad4_kernel<P>), dim3((unsigned)grid), dim3(256), Wg4<P>::BYTES, s, a.blocks, a.items, a.ksplit, a.Bp, a.spl, a.slabs, a.slab_stride, a.ri, a.use_raw,
                           a.ylo_epoch, a.launch_id, a.fold_apply, a.fold, a.fin_block, a.fin_err);
        return 0;
    });
    if (rc) return rc;
    DVAE_LAUNCH_OK("wgrad4_kernel");
    return 0;
}

int launch_slab_reduce(float* slabs, int64_t n, int nslabs, int64_t stride, hipStream_t s) {
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(512), dim3(256), 0, s, slabs, n, nslabs, stride);
    DVAE_LAUNCH_OK("slab_reduce_kernel");
    return 0;
}

int launch_slab_sum(const float* slabs, int64_t n, int nslabs, int64_t stride, float* dst, int accumulate, hipStream_t s) {
    hipLaunchKernelGGL(slab_sum_kernel, dim3(512), dim3(256), 0, s, slabs, n, nslabs, stride, dst, accumulate);
    DVAE_LAUNCH_OK("slab_sum_kernel");
    return 0;
}

int launch_apply_kernel(int precision, bool adam, const ApplyArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_params + 255) / 256 + 1));   // + 1: loss finalisation block
    if (precision == DVAE_PREC_BF16X3) {
        if (adam) hipLaunchKernelGGL((apply_kernel<__bf16, true, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((apply_kernel<__bf16, false, 2>), grid, dim3(256), 0, s, a);
    } else if (precision == DVAE_PREC_BF16) {
        if (adam) hipLaunchKernelGGL((apply_kernel<__bf16, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((apply_kernel<__bf16, false>), grid, dim3(256), 0, s, a);
    } else {
        if (adam) hipLaunchKernelGGL((apply_kernel<float, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((apply_kernel<float, false>), grid, dim3(256), 0, s, a);
    }
    DVAE_LAUNCH_OK("apply_kernel");
    return 0;
}

int launch_apply_losses(const ApplyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((apply_kernel<float, true>), dim3(1), dim3(256), 0, s, a);   // grid of 1 = the loss block only
    DVAE_LAUNCH_OK("apply_kernel(loss only)");
    return 0;
}

#ifdef DVAE_DIAG
int launch_apply_units(int precision, const ApplyArgs& a, const DeferTask* tasks, int nunits, hipStream_t s) {
    const dim3 gu((unsigned)((nunits + 3) / 4 + 1));
    if (precision == DVAE_PREC_BF16X3) hipLaunchKernelGGL((apply_units_kernel<__bf16, 2>), gu, dim3(256), 0, s, a, tasks, nunits);
    else hipLaunchKernelGGL((apply_units_kernel<__bf16, 1>), gu, dim3(256), 0, s, a, tasks, nunits);
    DVAE_LAUNCH_OK("apply_units_kernel");
    return 0;
}
#endif

}  // namespace fused
}  // namespace dvae

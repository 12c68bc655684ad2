// Plain tables and arguments of the weight-gradient and optimizer launches of the fused train step (train_wgrad.hip has the kernels and
// says what each does): what the host fills (train_fused.hip: fill_tables, w4_build_items) and the kernels read, and the launchers the
// host calls.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "apply_types.hpp"

namespace dvae {
namespace fused {

// wgrad_kernel: one wave = one 2 x 2 group of 32 x 32 tiles.  Missing halves (odd tile counts, 16-row heads) are null.
struct GroupDesc {
    const void* A[2];        // stash rows of dPre^T (32 output features each); A[1] may be null
    const void* Bm[2];       // stash rows of In^T (32 input features each); Bm[1] may be null
    int64_t out_off[2][2];   // float offset of tile (i, j) element (0, 0) in a gradient slab
    int64_t bias_off[2];     // float offset of the bias gradient rows of A block i, -1 = none
    int32_t ldo[2];          // row stride of the destination tensor of A block i
    int32_t mvalid[2];
    int32_t nvalid[2];
    int32_t split16;         // A block 0 holds two 16-row tensors (mu | log_var heads): rows >= 16 go to the *_hi targets
    int32_t ldo_hi;
    int64_t out_off_hi[2];
    int64_t bias_off_hi;
};

// wgrad_lds_kernel: one workgroup = one 4 x 4 block of 32 x 32 tiles
struct BlockDesc {
    const void* At[4];       // the block's A tiles (null = absent)
    const void* Bt[4];
    GroupDesc g[4];          // per wave (wr * 2 + wc): destinations of its 2 x 2 group; A[0] == null: nothing to do
};

// wgrad4_kernel: one workgroup = one 4 x 4 block of 32 x 32 tiles x one frame slice
struct Block4 {
    const void* At[4];       // stash rows of dPre^T, 32 output features each (null = absent; tiles are contiguous from 0)
    const void* Bt[4];       // stash rows of In^T, 32 input features each
    int64_t a_off[4];        // float offset, in a gradient slab, of (row 0 of A tile i, column 0) of its tensor
    int64_t bias_off[4];     // float offset of the bias-gradient rows of A tile i, -1 = none (only a layer's first B column carries them)
    int32_t ldo[4];          // row stride of A tile i's tensor
    int32_t mvalid[4];
    int32_t bcol[4];         // column of B tile j in the tensor
    int32_t nvalid[4];
    int32_t split16;         // A tile 0 holds two 16-row tensors (mu | log_var heads): rows >= 16 go to the *_hi targets
    int32_t ldo_hi;
    int64_t a_off_hi;
    int64_t bias_off_hi;
    // B tiles that are columns of the step's INPUTS (x: raw = 1, labels: raw = 2): the kernel can take them straight from the fp32
    // input matrix (the rows kernel then writes no stash for them); blocks never mix input tiles with stash tiles
    int32_t raw, rncols;     // rncols: columns of the input matrix (513 / y_dim)
    int32_t rcol[4];         // first column of B tile j in the input matrix
    int32_t wt[4], bt[4], wt_hi, bt_hi;   // tensor numbers of A tile i's weight / bias rows (and of the rows >= 16 of a split tile): fold_tail
    int32_t layer, pad_;                   // host side (w4_schedule): blocks of one emit() call share their A or their B tiles
};

// One workgroup of wgrad4_kernel = one item: block `block` over frames [kbeg, kend) into gradient slab `slice`.  The table is built on the
// host (w4_build_items): which slices a block is cut into, and which XCD a workgroup index lands on, are scheduling decisions the kernel
// only reads.  block < 0: an empty slot of the grid.
struct W4Item { int32_t block, slice; int64_t kbeg, kend; };
constexpr int W4_MAX_ITEMS = 4096;

struct RawIn { const float* x; const float* y; int ldx, ldy; int64_t B; };      // the step's fp32 input matrices (Block4::raw)

// the optimizer step folded into the tail of wgrad4_kernel (fold_tail; diagnostic builds): cnt = the flag header of the workspace
constexpr int FOLD_MAXB = 120;
struct FoldArgs { unsigned* cnt; unsigned target; unsigned max_polls; };

// ---- launchers (train_wgrad.hip).  Each returns 0 or an error code with set_error() called.
// the frame slicing of the two uniform-slice kernels: `ksplit` slices of `kper` frames, slice k into slab k
struct WgradArgs { int ksplit; int64_t Bp, spl, kper; float* slabs; int64_t slab_stride; };
// wgrad_kernel, `gpw` groups (waves) per workgroup
int launch_wgrad_ring(int precision, const GroupDesc* groups, int ngroups, const WgradArgs& a, int gpw, hipStream_t s);
// wgrad_lds_kernel (bf16 policies; diagnostic build only: DVAE_E_UNSUPPORTED in the product build)
int launch_wgrad_lds(int precision, const BlockDesc* blocks, int nblocks, const WgradArgs& a, hipStream_t s);
// wgrad4_kernel: its arguments in the kernel's order; grid = items of the host's table (+ 1 for the loss workgroup fin_block)
struct Wgrad4Args {
    const Block4* blocks; const W4Item* items; int ksplit; int64_t Bp, spl; float* slabs; int64_t slab_stride;
    RawIn ri; int use_raw; const unsigned* ylo_epoch; unsigned launch_id;
    ApplyArgs fold_apply; FoldArgs fold; int fin_block; const unsigned* fin_err;
};
int launch_wgrad4(int precision, const Wgrad4Args& a, int grid, hipStream_t s);
// slabs[0] = sum of the slabs, in place / dst = (accumulate ? dst : 0) + sum of the slabs
int launch_slab_reduce(float* slabs, int64_t n, int nslabs, int64_t stride, hipStream_t s);
int launch_slab_sum(const float* slabs, int64_t n, int nslabs, int64_t stride, float* dst, int accumulate, hipStream_t s);
// apply_kernel over a.n_params parameters (adam = false: refresh of the weight copies only); its loss block alone; apply_units_kernel
int launch_apply_kernel(int precision, bool adam, const ApplyArgs& a, hipStream_t s);
int launch_apply_losses(const ApplyArgs& a, hipStream_t s);
#ifdef DVAE_DIAG
int launch_apply_units(int precision, const ApplyArgs& a, const DeferTask* tasks, int nunits, hipStream_t s);
#endif

}  // namespace fused
}  // namespace dvae

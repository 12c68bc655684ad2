/* dvae_train.h -- C ABI of the fused train step (libdvae_hip.so).
 *
 * One step = the loop body of the reference's training scripts
 *   scripts/training_M1.py:134-139   r, mu, logvar = model(x); elbo; backward; Adam.step; zero_grad
 *   scripts/training_M2.py:142-147   the same with model(x, y)
 *   scripts/training_M2_info_vad.py:159-198   M2_info: + classifier(x), auxiliary(z), two BCE terms, two Adam
 *       groups incl. the reference's gradient-accumulation quirk (the auxiliary net sees (gamma - beta) * dBCE)
 * for the only geometry those scripts use (x_dim 513, z_dim 16, h_dim [128, 128]; y_dim 0, 1 or 513),
 * in three launches:
 *   rows kernel  : per 32-frame tile, the whole forward (encoder, reparametrisation, decoder),
 *                  the Itakura-Saito + KL sums and every backward-data product, on chip;
 *                  writes the operands of the weight gradients, transposed, to a stash;
 *   wgrad kernel : dW = dPre^T @ In for all layers (reduction over frames), k-split slabs;
 *   apply kernel : sums the slabs, torch.optim.Adam update of the fp32 master parameters,
 *                  refreshes the kernel-layout weight copies, finalises the loss scalars.
 * All state lives in caller-owned device buffers (PyTorch tensors): parameters / Adam
 * moments as flat fp32 buffers laid out per dvae_train_plan_t, scratch in `ws`.
 */
#ifndef DVAE_TRAIN_H
#define DVAE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DVAE_MODEL_M1 = 1, DVAE_MODEL_M2 = 2, DVAE_MODEL_M2_INFO = 3,
       /* encoder on x alone, decoder on [z | y]: the VAE body of DeepGenerativeModel_v3 / _v5 (packages/models/models.py:245-297, 437-444)
        * for the whole-model autograd path of the drop-in modules; y_dim 1, bf16 / bf16x3 operands (the 8-wave rows kernel) */
       DVAE_MODEL_M2_DEC = 4 };
/* Matrix-core operand policies (accumulation and master weights are always fp32):
 *   F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32)                       -- parity mode, 1/16 of the bf16 MFMA rate
 *   BF16   one bf16 per operand                                            -- fastest; weight gradients within ~4e-2 of their maximum
 *   BF16X3 split bf16: operand = hi + lo planes, product = hi*hi + lo*hi + hi*lo  -- parity-grade throughput mode
 *          (losses ~1e-7, gradients ~1e-4 of their maximum vs float64; tools/exp_precision.py), 3/16 of the F32 cost */
enum { DVAE_PREC_F32 = 0, DVAE_PREC_BF16 = 1, DVAE_PREC_BF16X3 = 2 };
#define DVAE_TRAIN_MAX_TENSORS 32

typedef struct {
    /* inputs (echoed) */
    int32_t model;            /* DVAE_MODEL_* */
    int32_t y_dim;            /* 0 (M1), 1 or 513 (M2), 1 (M2_info, M2_DEC) */
    int32_t precision;        /* DVAE_PREC_*: matrix-core operand type (accumulation is always fp32) */
    int32_t ksplit;           /* frame-axis slices of the weight-gradient reduction */
    int64_t B;                /* frames per step */
    /* flat fp32 parameter buffer: the reference's state_dict tensors, in state_dict order,
       each contiguous in nn.Linear layout [out, in] at a 256-byte aligned offset */
    int32_t n_tensors;
    int32_t reserved0;        /* schedule of the weight-gradient launch, set by dvae_train_plan: 0 = ksplit uniform frame slices; low 30 bits > 0 = class-sliced
                                 (workgroups of the launch; ksplit = the largest slice count of any block = slabs to sum); bit 30 = two launches
                                 (DVAE_EXCHANGE_GROUPS=2, dvae_train_grads_group).  Callers treat it as opaque. */
    int64_t n_params;                                   /* flat length in floats (with alignment gaps) */
    int64_t tensor_offset[DVAE_TRAIN_MAX_TENSORS];      /* in floats */
    int32_t tensor_rows[DVAE_TRAIN_MAX_TENSORS];
    int32_t tensor_cols[DVAE_TRAIN_MAX_TENSORS];        /* 1 for biases */
    /* scratch */
    int64_t workspace_bytes;
    int64_t grad_offset_bytes;   /* ws + this = ksplit slabs of n_params floats (slab 0 = flat gradient after reduce) */
    int64_t Bp;                  /* frames padded to the stash row length */
    int64_t rows_grid;           /* workgroups of the rows kernel */
    /* algorithmic work per step, for roofline accounting */
    double  flops_per_step;
    double  min_hbm_bytes_per_step;
    /* M2_info loss weights (scripts/training_M2_info_vad.py:53-55): enc_loss = ELBO + alpha*BCE(clf(x), y)
       - beta*BCE(aux(z), y), aux_loss = gamma*BCE(aux(z.detach()), y).  dvae_train_plan sets the script's
       defaults (0, 10, 1); the caller may overwrite them before dvae_train_init. */
    double  info_alpha, info_beta, info_gamma;
    /* Reparametrisation noise drawn inside the rows kernel when eps_noise == NULL: Philox4x32-10 keyed by rng_seed,
       counter (frame index, rng_step, draw); standard normals by Box-Muller.  The caller bumps rng_step every step
       (dvae_train_step uses its `step` argument instead).  dvae_train_noise reproduces the same numbers. */
    uint64_t rng_seed;
    uint64_t rng_step;
    /* Optional running sums for epoch logging (the scripts' `total_elbo += loss.item()`, training_M2.py:148-150, without a
       device-to-host sync per step): device pointer to 8 doubles, or 0.  dvae_train_apply / dvae_train_eval add the
       step's loss scalars (same order as losses3) to it. */
    uint64_t loss_accum;
    /* Optional gather (epoch shuffle without copying the data set): device pointer to B int64 row numbers, or 0.
       When set, x and y are the whole frame store (rows of ldx / ldy floats) and frame b of the step is row
       row_index[b].  row_count = rows of that store: an index outside [0, row_count) is never dereferenced -- the tile
       loader reads row 0 instead and adds one to the int32 device counter bad_row_counter (0 = none), which the
       caller inspects when it next synchronises. */
    uint64_t row_index;
    int64_t  row_count;
    uint64_t bad_row_counter;
    /* rows kernel generation chosen by dvae_train_plan: 2 = 8-wave chain + helper kernel (csrc/train_rows2.hip; M1 / M2 with
       bf16 or bf16x3 operands), 1 = 4-wave kernel (csrc/train_rows1.hip; every model and policy).  Environment override
       DVAE_ROWS=1 at plan time. */
    int32_t  rows_kernel;
    int32_t  reserved1;
} dvae_train_plan_t;

/* Fill `plan` for (model, y_dim, precision, B).  ksplit_hint 0 = choose.  Returns DVAE_E_UNSUPPORTED
 * for geometries the fused kernels do not cover (the layer-level path of dvae.h covers those). */
int dvae_train_plan(int model, int y_dim, int precision, int64_t B, int ksplit_hint, dvae_train_plan_t* plan);

/* One-time setup of `ws` (zero fill, tile table, kernel-layout weight copies from `params`).
 * Synchronises the stream once (host-to-device copy of the tile table). */
int dvae_train_init(const dvae_train_plan_t* plan, const float* params, void* ws, void* stream);

/* rows kernel + wgrad kernel (+ slab reduction into slab 0 when reduce_slabs != 0).
 * x [B, 513] (ldx), y [B, y_dim] (ldy, may be NULL for M1), eps_noise [B, 16]: fp32 device tensors; eps_noise NULL = draw
 * the noise in the kernel (the reference draws torch.randn(mu.size()) on the host and copies it, models.py:10-13).
 * elbo_eps is the `eps` of elbo(x, r, mu, logvar, eps) (packages/models/utils.py:73). */
int dvae_train_grads(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                     const float* y, int ldy, const float* eps_noise, float elbo_eps, int reduce_slabs, void* stream);

/* The gradient pass of a step in TWO calls, so that the exchange of the first part of the flat gradient can run while the second part is
 * computed (no reference call site: scripts/training_M2.py:31-33 is single-device).  For a plan made while
 * DVAE_EXCHANGE_GROUPS=2 is set: group 0 = rows kernel + the weight-gradient launch of the decoder-side tensors (and M2_info's side nets) --
 * floats [tensor_offset[8], n_params) of the flat gradient; group 1 = the launch of the encoder's tensors, floats [0, tensor_offset[8]);
 * group 1 must follow a group 0 call on the same workspace.  reduce_slabs sums the slabs of the group's range into slab 0.
 * dvae_train_grads on such a plan runs both launches.  dvae_train_group_range: the range of a group (-1: everything), *ngroups = 2 or 1. */
int dvae_train_grads_group(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx, const float* y, int ldy,
                           const float* eps_noise, float elbo_eps, int group, int reduce_slabs, void* stream);
int dvae_train_group_range(const dvae_train_plan_t* plan, int group, int64_t* lo, int64_t* hi, int* ngroups);

/* apply kernel: g = grad_scale * sum of n_slabs slabs; Adam(lr, beta1, beta2, adam_eps) at `step` (1-based) on
 * params/m/v; refresh weight copies; losses3 = {recon + KL, recon, KL} (means over the B local frames);
 * for M2_info the buffer holds 8 floats: {ELBO, recon, KL, enc_loss, classif_loss, aux_loss, aux_enc_loss, 0}. */
int dvae_train_apply(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws, int n_slabs,
                     int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale,
                     float* losses3, void* stream);

/* dvae_train_grads + dvae_train_apply (single-GPU step). */
int dvae_train_step(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws,
                    const float* x, int ldx, const float* y, int ldy, const float* eps_noise, float elbo_eps,
                    int step, double lr, double beta1, double beta2, double adam_eps, float* losses3, void* stream);

/* The same step in TWO launches (round 4): the optimizer update of step n is deferred into the opening of step n + 1's rows kernel, where
 * the GEMM waves would otherwise wait for the x tile (csrc/apply_common.hpp), and a step's loss scalars are finalised by its own rows
 * kernel.  After this call returns, losses3 (stream-ordered) holds step n's losses and the gradient slabs step n's gradient, but
 * params / m / v and the weight copies still hold the state BEFORE step n's update: it is PENDING on `ws` until the next
 * dvae_train_step_deferred on the same workspace or dvae_train_flush.  Every other entry point of this header flushes first by itself;
 * a caller that reads or writes params / m / v directly must call dvae_train_flush before (dvae_train_repack refuses while an update is
 * pending).  Results are bit-identical to dvae_train_step (same slab sums, same element arithmetic).  Falls back to dvae_train_step when
 * the plan cannot defer (M2_info, the 4-wave rows kernel, grids smaller than the update's task list or larger than the CUs) and unless
 * DVAE_DEFER_APPLY=1 is set: measured on the MI355X the two-launch step is bit-identical and NOT faster, so it is opt-in.  The same params / m / v pointers and hyper-parameter semantics as dvae_train_step. */
int dvae_train_step_deferred(const dvae_train_plan_t* plan, float* params, float* m, float* v, void* ws,
                             const float* x, int ldx, const float* y, int ldy, const float* eps_noise, float elbo_eps,
                             int step, double lr, double beta1, double beta2, double adam_eps, float* losses3, void* stream);
/* Apply the pending update of `ws`, if any (one apply launch on `stream`). */
int dvae_train_flush(const dvae_train_plan_t* plan, void* ws, void* stream);
/* 1 when an update is pending on `ws`. */
int dvae_train_pending(const void* ws);
/* 1 when dvae_train_step_deferred would defer on this plan / workspace / device / environment (otherwise it is dvae_train_step). */
int dvae_train_can_defer(const dvae_train_plan_t* plan, const void* ws);

/* Validation pass of the scripts (scripts/training_M2.py:176-193: forward + elbo, no backward, no update):
 * rows kernel + loss finalisation only.  losses3 as for dvae_train_apply. */
int dvae_train_eval(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                    const float* y, int ldy, const float* eps_noise, float elbo_eps, float* losses3, void* stream);

/* Whole-model autograd path of the drop-in modules (packages/models/models.py: VariationalAutoencoder.forward,
 * DeepGenerativeModel.forward -- reference models.py:172-179, 200-203): ONE launch for the model forward instead of one per
 * nn.Linear, and the backward pass as rows kernel + weight-gradient kernel + slab sum, under stock torch autograd / torch.optim.Adam
 * (scripts/training_M2.py:142-147).  M1 / M2 with bf16 / bf16x3 operands (plan->rows_kernel == 2), no gather table.
 *   dvae_module_forward : (repack != 0: rebuild the kernel-layout weight copies from `params` first) r = model(x, y) [B, 513] (ld_r),
 *                         mu, log_var, z [B, 16] (out_z may be NULL); eps_noise [B, 16] is the reparametrisation noise.
 *   dvae_module_backward: recomputes the forward, then the backward from the upstream gradients g_r [B, 513] (ld_gr), g_mu, g_lv,
 *                         g_z [B, 16] (each may be NULL = zero); grad_flat[n_params] (plan layout) = (accumulate ? grad_flat : 0) + dL/dparams. */
int dvae_module_forward(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                        const float* y, int ldy, const float* eps_noise, float* out_r, int ld_r, float* out_mu,
                        float* out_lv, float* out_z, int repack, void* stream);
int dvae_module_backward(const dvae_train_plan_t* plan, const float* params, void* ws, const float* x, int ldx,
                         const float* y, int ldy, const float* eps_noise, const float* g_r, int ld_gr,
                         const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate, void* stream);

/* The [B, 16] standard normals the rows kernel draws for (plan->rng_seed, step) when eps_noise == NULL. */
int dvae_train_noise(const dvae_train_plan_t* plan, uint64_t step, float* eps_out, void* stream);

/* Rebuild the kernel-layout weight copies after `params` was written from outside (load_state_dict). */
int dvae_train_repack(const dvae_train_plan_t* plan, const float* params, void* ws, void* stream);

/* ---- the fused train step for M1 / M2 of ANY covered size (csrc/train_generic.hip): x 513, y_dim 0 (M1) or 1..513 (M2: encoder on
 * [x | y], decoder on [z | y]), hidden widths h1 / h2 1..512, z_dim 1..128 -- the limits of dvae_mcem_plan_dims -- two tanh layers a side,
 * loss elbo, exact fp32.  Three launches per step whatever the geometry: rows kernel (forward, loss terms, backward-data chain; layer inputs
 * and pre-activation gradients to a stash), weight-gradient kernel (all seven matrices and biases, one partial slab per frame slice, no
 * atomics), apply kernel (slab sums in slab order, the Adam element of dvae_train_apply, both packed weight copies, the loss scalars).
 * The resident step above stays the default at z 16 / h (128, 128); this one also runs there when asked.  Same conventions: caller-owned
 * flat buffers laid out per the plan (state_dict order, 256-byte aligned tensors), scratch in `ws`, results stream-ordered. */
typedef struct {
    /* inputs (echoed) */
    int32_t model;            /* DVAE_MODEL_M1 or DVAE_MODEL_M2 (DVAE_MODEL_M2_DEC: dvae_module_generic_plan, the module entry points only) */
    int32_t y_dim, z_dim, h1, h2;
    int32_t precision;        /* DVAE_PREC_F32 */
    int32_t ksplit;           /* frame slices of the weight-gradient reduction = slabs the apply kernel sums (at most 16) */
    int32_t n_tensors;        /* 14 */
    int64_t B;                /* frames per step */
    int64_t n_params;         /* flat length in floats (with alignment gaps) */
    int64_t tensor_offset[DVAE_TRAIN_MAX_TENSORS];      /* in floats */
    int32_t tensor_rows[DVAE_TRAIN_MAX_TENSORS];
    int32_t tensor_cols[DVAE_TRAIN_MAX_TENSORS];        /* 1 for biases */
    int64_t workspace_bytes;
    int64_t grad_offset_bytes;   /* ws + this = ksplit slabs of n_params floats */
    int64_t Bp;                  /* frames padded to whole 16-frame tiles */
    int64_t rows_grid;           /* workgroups of the rows kernel (tiles beyond it are strided over) */
    int64_t slice_frames;        /* frames of a slice (a multiple of 16; the last slice may be shorter) */
    int64_t wgrad_items;         /* workgroups of the weight-gradient launch */
    int64_t lds_bytes;           /* dynamic LDS of the rows kernel */
    /* set by the caller between calls, as in dvae_train_plan_t: float64 running sums (8 doubles) or 0; the gather table (B int64 row
       numbers of the frame store x / y) or 0, the rows of that store, and the int32 counter of refused indices or 0.  An index outside
       [0, row_count) is never dereferenced: row 0 is read instead and the counter incremented. */
    uint64_t loss_accum;
    uint64_t row_index;
    int64_t  row_count;
    uint64_t bad_row_counter;
    /* std_norm (dvae_train_generic_plan_norm; 0 from dvae_train_generic_plan): set by the planner and part of the layout.  With it the
       caller sets, before the first launch, two device tables of 513 floats that stay alive and unchanged while the plan is used:
       norm_mean = mean, norm_div = fl32(std + fl32(norm_eps)) formed once on the host in float32. */
    int32_t  std_norm;
    int32_t  reserved0;
    uint64_t norm_mean;
    uint64_t norm_div;
    /* The weighted KL term; the planners set 1 and 0, the caller may overwrite both before any call (finite, >= 0; not part of the layout).
       With k_bj = -0.5 (lv_bj - mu_bj^2 - exp(lv_bj)) the element of the reference's KL (its minimum is 0.5), the objective is
           loss = recon + kl_weight * mean_b sum_j max(k_bj, kl_floor)
       with torch.clamp(k, min=kl_floor)'s gradient: the KL parts of d mu and d log_var are fl32(fl32(kl_weight) / B) times mu and
       -0.5 (1 - e^lv) where k_bj >= kl_floor and exact zeros below (the per-element form of free bits; kl_floor <= 0.5 clamps nothing).
       losses3 = {the objective, recon, KL}: recon and KL stay the raw, unweighted, unclamped means.  _grads, _reduce, _apply, _step and
       _eval read the fields at each call; a warm-up is the caller writing kl_weight before a step.  (1, 0) is the unweighted step, bit
       for bit.  The module entry points do not read them: their upstream gradients carry the loss. */
    double   kl_weight;
    double   kl_floor;
} dvae_train_generic_plan_t;

/* Host only.  ksplit_hint 0 = choose.  DVAE_E_UNSUPPORTED for M2_info / M2_DEC and the bf16 policies (they exist at the reference geometry
 * only), DVAE_E_BADARG naming the limits for a size outside them. */
int dvae_train_generic_plan(int model, int y_dim, int z_dim, int h1, int h2, int precision, int64_t B, int ksplit_hint,
                            dvae_train_generic_plan_t* plan);
/* dvae_train_generic_plan with the scripts' std_norm switch (scripts/training_M1.py:128-134, training_M2.py:136-144): std_norm 1 plans
 * the step whose ENCODER reads [xn | y], xn = fl32(fl32(x - mean) / div) per bin -- one IEEE subtraction and one correctly rounded IEEE
 * division in float32, bit for bit torch's (x - mean) / div --, while the labels, the Itakura-Saito term, its derivative and log(x + eps)
 * use the raw x: `model(x_norm, y)` scored by `elbo(x, r, ...)`.  Padded bins and frames past B stay exact zeros.  The rows kernel keeps xn in
 * a further stash block of 528 columns (behind every other block), from which the weight gradient of encoder layer 1 is formed; the
 * weight-gradient, apply, reduce, norm and clipped-apply kernels are the ones of the plain step.  std_norm 0 is dvae_train_generic_plan:
 * the same layout, workspace size, LDS and launches.  Every dvae_train_generic_* call below serves both kinds of plan. */
int dvae_train_generic_plan_norm(int model, int y_dim, int z_dim, int h1, int h2, int precision, int64_t B, int ksplit_hint, int std_norm,
                                 dvae_train_generic_plan_t* plan);
/* One-time setup of `ws` (item table, packed weight copies from `params`); synchronises the stream once. */
int dvae_train_generic_init(const dvae_train_generic_plan_t* plan, const float* params, void* ws, void* stream);
/* Rebuild both packed weight copies after `params` was written from outside. */
int dvae_train_generic_repack(const dvae_train_generic_plan_t* plan, const float* params, void* ws, void* stream);
/* rows kernel + weight-gradient kernel: x [B, 513] (ldx), y [B, y_dim] (ldy; NULL for M1) -- or the frame stores under a gather table --,
 * eps_noise [B, z_dim] (required).  The gradient of the mean loss over the B frames is left as plan->ksplit slabs. */
int dvae_train_generic_grads(const dvae_train_generic_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                             const float* eps_noise, float elbo_eps, void* stream);
/* apply kernel: g = grad_scale * (slabs summed in slab order); Adam at `step` (1-based); packed copies; losses3 = {recon + KL, recon, KL}
 * (under plan->kl_weight / kl_floor other than 1 / 0: {recon + kl_weight * the clamped KL, recon, KL}, see the plan).
 * Separate from _grads so that a gradient exchange can sit between them. */
int dvae_train_generic_apply(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr,
                             double beta1, double beta2, double adam_eps, double grad_scale, float* losses3, void* stream);
/* dvae_train_generic_grads + dvae_train_generic_apply with grad_scale 1. */
int dvae_train_generic_step(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                            const float* y, int64_t ldy, const float* eps_noise, float elbo_eps, int step, double lr, double beta1,
                            double beta2, double adam_eps, float* losses3, void* stream);
/* Forward and loss only (two launches): parameters, moments and gradient slabs are left alone. */
int dvae_train_generic_eval(const dvae_train_generic_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                            const float* eps_noise, float elbo_eps, float* losses3, void* stream);
/* Gradient accumulation and data parallelism: between _grads and the optimizer sits a flat gradient of plan->n_params floats in the plan's
 * layout (16-byte aligned).  _reduce (one launch): flat[i] = (accumulate ? flat[i] : nothing) + weight * (the plan->ksplit slabs of the last
 * _grads summed in slab order); with accumulate 0 `flat` is written and never read; the alignment gaps between tensors receive zeros, so
 * the buffer is finite everywhere and can travel through a collective whole.  weight 1.0 leaves the sum's bits untouched.  The same launch
 * finalises the micro-batch's loss scalars (and plan->loss_accum) as _apply would: a micro-batch is rows + weight gradients + reduce, three
 * launches.  _apply_flat: the apply kernel on `flat` as the ONE slab, g = grad_scale * flat: Adam at `step`, packed copies, no loss
 * scalars.  Both return DVAE_E_BADARG for a null pointer, accumulate outside {0, 1}, a non-finite weight / grad_scale or a changed plan,
 * before anything touches the device. */
int dvae_train_generic_reduce(const dvae_train_generic_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses3,
                              void* stream);
int dvae_train_generic_apply_flat(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step,
                                  double lr, double beta1, double beta2, double adam_eps, double grad_scale, void* stream);
/* _apply_flat with the global gradient norm clipped on the device: torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2) over
 * ALL tensors of the plan at once (one Adam, one norm), two launches and no host round trip.  With G = `flat`, gs = grad_scale:
 *   s          = sum over the floats of the plan's tensors of (double)G[i]^2 (the alignment gaps count as zero whatever they hold);
 *   total_norm = |gs| sqrt(s);   coef = min(1, max_norm / (total_norm + 1e-6));   gscale_eff = (float)(gs * coef), formed in double and
 *                rounded once;
 *   the update is _apply_flat's, element for element, with gscale_eff in the place of (float)grad_scale.  Where coef == 1 -- max_norm = +inf,
 *   or any max_norm >= total_norm + 1e-6 -- parameters, moments and packed copies come out bit-identical to _apply_flat's.
 * Order of summation: the norm launch gives workgroup c the chunk of floats [4096 c, 4096 (c + 1)) -- a compile-time constant, not a
 * function of the grid or the part --; a thread adds its sixteen squares in address order, then lanes, then the four waves in order, and
 * the partial goes to scratch[c] (doubles; dvae_train_gradnorm_scratch_bytes(plan->n_params) bytes, the caller's, 8-byte aligned).  The
 * guarded apply launch sums the partials in every workgroup alike: thread t takes chunks t, t + 256, ... ascending, then lanes, then
 * waves.  No floating-point atomics: the same `flat` gives the same s, coef and update on every run and on every rank, so replicas that
 * exchanged `flat` stay equal.
 * Skip rule: if s is not finite (an inf or NaN anywhere in the gradient, or an overflowing sum), NOTHING is written: parameters, both
 * moments and both packed copies stay bit for bit as they were; *skipped_counter (a device int32 the caller zeroes and reads) goes up by
 * one; total_norm is reported as it came out (inf or NaN) and coef as 0.  The caller's step count still advances: `step` is passed by
 * value for the bias corrections and the host cannot know of the skip without a synchronisation, so the update after a skipped one runs
 * with the bias corrections of one step later (a factor that tends to 1; the first steps of a run are where it matters).
 * norm2_out: two device floats, {total_norm, coef} of this call.  DVAE_E_BADARG, before anything touches the device, for a null pointer,
 * max_norm that is NaN or <= 0 (+inf is legal), a misaligned `flat` / scratch, and whatever _apply_flat refuses. */
int64_t dvae_train_gradnorm_scratch_bytes(int64_t n_params);    /* 0 (and dvae_last_error) for n_params < 1 or >= 2^31 - 4096 */
int dvae_train_generic_apply_flat_clipped(const dvae_train_generic_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat,
                                          int step, double lr, double beta1, double beta2, double adam_eps, double grad_scale, double max_norm,
                                          void* scratch, float* norm2_out, int32_t* skipped_counter, void* stream);

/* Whole-model autograd path of the drop-in modules at ANY covered size (disentangled-vae_amd/module_path.py: GenericModuleEngine):
 * dvae_module_forward / dvae_module_backward above on a dvae_train_generic_plan_t (M1 / M2, exact fp32), `ws` set up by
 * dvae_train_generic_init.  Two further modes of the generic rows kernel; the weight-gradient and reduce kernels are the train step's.
 *   _forward : (repack != 0: both packed weight copies rewritten from `params` first, one launch) then ONE launch: r = model(x, y)
 *              [B, 513] (ld_r >= 513), mu, log_var, z [B, z_dim] (out_z may be NULL); eps_noise [B, z_dim].  Padding between the rows of
 *              out_r is not written.  No stash, no loss sums.
 *   _backward: three launches -- the rows kernel recomputes the forward and runs the backward chain from the upstream gradients g_r
 *              [B, 513] (ld_gr >= 513), g_mu, g_lv, g_z [B, z_dim], each NULL = zero: da = g_r r; dz = dpre_d1 D1[:, :z] + g_z;
 *              d mu = dz + g_mu; d log_var = dz std eps / 2 + g_lv (no 1 / B, no KL term: the upstream gradients carry both); the
 *              weight-gradient kernel; the reduce kernel into grad_flat[n_params] (plan layout, 16-byte aligned): accumulate 0
 *              overwrites every element, accumulate 1 adds with one float32 addition per element; the alignment gaps between the
 *              tensors receive zeros in either mode, as from dvae_train_generic_reduce.
 * The same inputs give the same bits.  DVAE_E_BADARG by name, before anything is launched: ld_r / ld_gr below 513, ldx below 513 or ldy
 * below y_dim (rows that overlap), a std_norm plan (normalise in torch and pass x_norm), a plan with a gather table, a null pointer. */
int dvae_module_generic_forward(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                const float* y, int64_t ldy, const float* eps_noise, float* out_r, int64_t ld_r, float* out_mu,
                                float* out_lv, float* out_z, int repack, void* stream);
int dvae_module_generic_backward(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                 const float* y, int64_t ldy, const float* eps_noise, const float* g_r, int64_t ld_gr,
                                 const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate, void* stream);
/* The M2_info body ("M2_DEC": DeepGenerativeModel_v3's encoder on x ALONE, decoder on [z | y]) of any covered size on the same two entry
 * points.  dvae_module_generic_plan (host only): for DVAE_MODEL_M1 / _M2 the plan of dvae_train_generic_plan at DVAE_PREC_F32, byte for
 * byte; for DVAE_MODEL_M2_DEC, y_dim 1..513 with the same limits on h1 / h2 / z_dim, a plan whose tensor 0 is [h1, 513] (the encoder has no
 * label columns: the packed label block of encoder layer 1 has no elements) and whose tensor 8 is [h2, z_dim + y_dim]; one more packed
 * copy, the transposed label columns of decoder layer 1, sits behind the last packed copy of the workspace.  The plan is exact fp32 (there
 * is no precision argument; a plan whose precision field was changed is refused as any changed plan).  DVAE_E_BADARG naming the limits for
 * a size outside them, DVAE_E_UNSUPPORTED for any other model (M2_info as a whole: dvae_train_info_plan).
 * dvae_train_generic_init / _repack and dvae_module_generic_forward / _backward accept an M2_DEC plan (y is required).  Every train-step
 * entry point above (_grads, _step, _eval, _apply, _reduce, _apply_flat, _apply_flat_clipped) refuses it with DVAE_E_BADARG naming the
 * model before anything is launched: there is no train step on the body alone.
 * dvae_module_generic_backward_y is _backward plus the gradient with respect to the labels: g_y [B, y_dim] (ld_gy >= y_dim) receives
 * dpre_d1 D1[:, z:] -- the decoder's share, the only one: the encoder does not see y; no 1 / B, as for the other upstream gradients --
 * computed beside dz in the rows kernel, no further launch.  Padding between the rows of g_y is not written.  g_y NULL: exactly _backward
 * (nothing further is computed or written).  The parameter gradients have the same bits with and without g_y.  DVAE_E_BADARG by name,
 * before anything is launched: ld_gy below y_dim, a g_y on a plan whose model is not M2_DEC, and whatever _backward refuses. */
int dvae_module_generic_plan(int model, int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint, dvae_train_generic_plan_t* plan);
int dvae_module_generic_backward_y(const dvae_train_generic_plan_t* plan, const float* params, void* ws, const float* x, int64_t ldx,
                                   const float* y, int64_t ldy, const float* eps_noise, const float* g_r, int64_t ld_gr,
                                   const float* g_mu, const float* g_lv, const float* g_z, float* grad_flat, int accumulate,
                                   float* g_y, int64_t ld_gy, void* stream);

/* ---- the fused train step for the label classifier alone (csrc/train_classifier.hip): Classifier([513, [h1, h2], y_dim]) of
 * packages/models/models.py -- relu, relu, sigmoid -- under binary_cross_entropy (packages/models/utils.py:55-56) and Adam: the loop body
 * the reference sketches in scripts/train_audio_net.py, and the net it otherwise trains only as a side net of M2_info
 * (scripts/training_M2_info_vad_pretrain.py).  x 513, h1 / h2 1..512, y_dim 1..513 (the limits of dvae_classify_generic_batch, which runs
 * the result), exact fp32, one GPU.  Three launches per step: rows kernel (forward, BCE, confusion counts, backward-data chain, stash),
 * the weight-gradient and apply kernels of the generic step above on this step's tables.  Contract:
 *   loss      mean over the B frames of -sum_j [y_j log(p_j + eps) + (1 - y_j) log(1 - p_j + eps)], p = sigmoid(a); labels are floats,
 *             soft labels in [0, 1] go through the same formulas; summed per workgroup in double, workgroups in order;
 *   backward  d loss / d p = -(1 / B) (y / (p + eps) - (1 - y) / (1 - p + eps)) with the eps terms kept, then p (1 - p) and the relu masks;
 *   counts    tp, tn, fp, fn over all B * y_dim elements (prediction p > 0.5, truth y != 0; the order of dvae_label_counts_batch), integers;
 *   the same inputs give the same bits (no atomics on floats; slabs and partial sums in a fixed order);
 *   six tensors in Classifier.state_dict() order: hidden.0.weight, hidden.0.bias, hidden.1.weight, hidden.1.bias, output_layer.weight,
 *   output_layer.bias, each at a 256-byte aligned offset of the flat buffers. */
typedef struct {
    /* inputs (echoed) */
    int32_t h1, h2, y_dim;
    int32_t precision;        /* DVAE_PREC_F32 */
    int32_t ksplit;           /* frame slices of the weight-gradient reduction = slabs the apply kernel sums (at most 16) */
    int32_t n_tensors;        /* 6 */
    int64_t B;                /* frames per step */
    int64_t n_params;         /* flat length in floats (with alignment gaps) */
    int64_t tensor_offset[DVAE_TRAIN_MAX_TENSORS];      /* in floats */
    int32_t tensor_rows[DVAE_TRAIN_MAX_TENSORS];
    int32_t tensor_cols[DVAE_TRAIN_MAX_TENSORS];        /* 1 for biases */
    int64_t workspace_bytes;
    int64_t grad_offset_bytes;   /* ws + this = ksplit slabs of n_params floats */
    int64_t Bp;                  /* frames padded to whole 16-frame tiles */
    int64_t rows_grid;           /* workgroups of the rows kernel (tiles beyond it are strided over) */
    int64_t slice_frames;        /* frames of a slice (a multiple of 16; the last slice may be shorter) */
    int64_t wgrad_items;         /* workgroups of the weight-gradient launch */
    int64_t lds_bytes;           /* dynamic LDS of the rows kernel */
    /* set by the caller between calls: float64 running sums (8 doubles; the loss is added to the first two) or 0; int64 running counts
       (4) or 0; the gather table, the rows of the frame store and the counter of refused indices as in dvae_train_generic_plan_t */
    uint64_t loss_accum;
    uint64_t count_accum;
    uint64_t row_index;
    int64_t  row_count;
    uint64_t bad_row_counter;
} dvae_train_clf_plan_t;

/* Host only.  ksplit_hint 0 = choose.  DVAE_E_UNSUPPORTED naming the limits for a width outside them or another operand policy;
 * DVAE_E_BADARG for B < 1. */
int dvae_train_clf_plan(int h1, int h2, int y_dim, int precision, int64_t B, int ksplit_hint, dvae_train_clf_plan_t* plan);
/* One-time setup of `ws` (item table, packed weight copies from `params`); synchronises the stream once. */
int dvae_train_clf_init(const dvae_train_clf_plan_t* plan, const float* params, void* ws, void* stream);
/* Rebuild both packed weight copies after `params` was written from outside. */
int dvae_train_clf_repack(const dvae_train_clf_plan_t* plan, const float* params, void* ws, void* stream);
/* rows kernel + weight-gradient kernel: x [B, 513] (ldx), y [B, y_dim] (ldy) -- or the frame stores under a gather table.  The gradient
 * of the mean loss is left as plan->ksplit slabs. */
int dvae_train_clf_grads(const dvae_train_clf_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy, float bce_eps,
                         void* stream);
/* apply kernel: g = grad_scale * (slabs summed in slab order); Adam at `step` (1-based); packed copies; losses3 = {BCE, BCE, 0} (the
 * generic step's three scalars with no second term); counts4 = {tp, tn, fp, fn} of the step's batch. */
int dvae_train_clf_apply(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr, double beta1,
                         double beta2, double adam_eps, double grad_scale, float* losses3, int64_t* counts4, void* stream);
/* dvae_train_clf_grads + dvae_train_clf_apply with grad_scale 1. */
int dvae_train_clf_step(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                        const float* y, int64_t ldy, float bce_eps, int step, double lr, double beta1, double beta2, double adam_eps,
                        float* losses3, int64_t* counts4, void* stream);
/* Forward, loss and counts only (two launches): parameters, moments and gradient slabs are left alone. */
int dvae_train_clf_eval(const dvae_train_clf_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy, float bce_eps,
                        float* losses3, int64_t* counts4, void* stream);
/* dvae_train_generic_reduce / _apply_flat for this step; losses3 / counts4 (and plan->count_accum) as dvae_train_clf_apply. */
int dvae_train_clf_reduce(const dvae_train_clf_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses3, int64_t* counts4,
                          void* stream);
int dvae_train_clf_apply_flat(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step, double lr,
                              double beta1, double beta2, double adam_eps, double grad_scale, void* stream);
/* dvae_train_generic_apply_flat_clipped for this step: one norm over the six tensors. */
int dvae_train_clf_apply_flat_clipped(const dvae_train_clf_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step,
                                      double lr, double beta1, double beta2, double adam_eps, double grad_scale, double max_norm, void* scratch,
                                      float* norm2_out, int32_t* skipped_counter, void* stream);

/* ---- the fused train step for M2_info of ANY covered size (csrc/train_info.hip): DeepGenerativeModel_v5 of packages/models/models.py:390-444
 * -- encoder on x alone, decoder on [z | y], a relu classifier on x, an adversarial auxiliary relu classifier on z -- under the loop body of
 * scripts/training_M2_info_vad.py:159-198.  x 513, y_dim 1..513, hidden widths h1 / h2 1..512, z_dim 1..128, exact fp32, one GPU.  THREE
 * launches per step whatever the geometry and the batch: rows kernel (the four forward passes, the loss terms, every backward-data chain,
 * the stash), then the weight-gradient and apply kernels of the generic step above on this step's tables (thirteen matrices, 26 tensors).
 * Contract:
 *   enc_loss = ELBO + alpha BCE(clf(x), y) - beta BCE(aux(z), y): its gradient goes into every enc_dec_clf tensor, the -beta term through
 *              z into the encoder; aux_loss = gamma BCE(aux(z.detach()), y); the auxiliary tensors receive (gamma - beta) dBCE (the
 *              script never zeroes what enc_loss.backward() leaves in them); the auxiliary pre-activation gradients are formed once at
 *              unit weight, so beta = 0 divides nothing; the eps inside the BCE logs is elbo_eps, as in the script;
 *   one Adam update over all 26 tensors at the same step count (the script's two optimizers share their hyper-parameters);
 *   losses8 = {ELBO, recon, KL, enc_loss, classif_loss, aux_loss, aux_enc_loss, 0}, means over the B frames (the order of dvae_train_apply);
 *   the same inputs give the same bits (no atomics on floats; slabs and partial sums in a fixed order);
 *   26 tensors in DeepGenerativeModel_v5.state_dict() order, each at a 256-byte aligned offset of the flat buffers.
 * Two independent options (dvae_train_info_plan_mode; mode 0 is the contract above) give the loop body of
 * scripts/training_M2_info_vad_pretrain.py:162-200 and its kin.  With p_c = clf(x), p_a = aux(z):
 *   DVAE_INFO_DEC_CLASSIFIER  the decoder input is [z | p_c] instead of [z | y]: decoder layer 1 has dW = dpre_d1^T [z | p_c], and the
 *              reconstruction gradient reaches the classifier through its label columns: d enc_loss / d p_c = alpha dBCE / d p_c +
 *              dpre_d1 D1[:, z : z + y], then p_c (1 - p_c) and the relu masks.  With alpha = 0 that is the classifier's only gradient;
 *   DVAE_INFO_AUX_UNIFORM / DVAE_INFO_AUX_ENTROPY  the adversarial term of enc_loss is V(p_a) instead of BCE(p_a, y):
 *              enc_loss = ELBO + alpha BCE(p_c, y) - beta V, aux_loss = gamma BCE(p_a, y), losses8[6] = beta V, with
 *              V = binary_cross_entropy_v2 (targets 0.5; d V / d p = -0.5 / (p + eps) + 0.5 / (1 - p + eps)) or binary_cross_entropy_v3
 *              (targets p_a, the entropy; d V / d p = -[log(p + eps) + p / (p + eps) - log(1 - p + eps) - (1 - p) / (1 - p + eps)]), each a
 *              mean over the B frames of a sum over the y_dim columns, eps = elbo_eps.  dz = dpre_d1 D1[:, :z] - beta dV / dz; the auxiliary
 *              tensors receive gamma dBCE - beta dV: two output gradients through the same relu masks; beta = 0 still divides nothing.
 *   One Adam update, three launches and the same bits from the same inputs, as in mode 0. */
#define DVAE_INFO_DEC_CLASSIFIER 1
#define DVAE_INFO_AUX_UNIFORM    2
#define DVAE_INFO_AUX_ENTROPY    4
typedef struct {
    /* inputs (echoed) */
    int32_t y_dim, z_dim, h1, h2;
    int32_t ksplit;              /* frame slices of the weight-gradient reduction = slabs the apply kernel sums (at most 16) */
    int32_t n_tensors;           /* 26 */
    int32_t launches_per_step;   /* 3, whatever the geometry, B and the mode */
    int32_t info_mode;           /* DVAE_INFO_* bits; 0 from dvae_train_info_plan */
    int64_t B;                   /* frames per step */
    int64_t n_params;            /* flat length in floats (with alignment gaps) */
    int64_t tensor_offset[DVAE_TRAIN_MAX_TENSORS];      /* in floats */
    int32_t tensor_rows[DVAE_TRAIN_MAX_TENSORS];
    int32_t tensor_cols[DVAE_TRAIN_MAX_TENSORS];        /* 1 for biases */
    int64_t workspace_bytes;
    int64_t grad_offset_bytes;   /* ws + this = ksplit slabs of n_params floats; the auxiliary tensors hold (gamma - beta) dBCE */
    int64_t Bp;                  /* frames padded to whole 16-frame tiles */
    int64_t rows_grid;           /* workgroups of the rows kernel (tiles beyond it are strided over) */
    int64_t slice_frames;        /* frames of a slice (a multiple of 16; the last slice may be shorter) */
    int64_t wgrad_items;         /* workgroups of the weight-gradient launch */
    int64_t lds_bytes;           /* dynamic LDS of the rows kernel (at most 160 KB at every geometry within the limits) */
    /* loss weights: dvae_train_info_plan sets the script's defaults (0, 10, 1); the caller may overwrite them before dvae_train_info_init */
    double  info_alpha, info_beta, info_gamma;
    /* set by the caller between calls, as in dvae_train_generic_plan_t: float64 running sums (8 doubles) or 0; the gather table, the rows
       of the frame store and the int32 counter of refused indices or 0 */
    uint64_t loss_accum;
    uint64_t row_index;
    int64_t  row_count;
    uint64_t bad_row_counter;
    /* The weighted KL term of the VAE body, as in dvae_train_generic_plan_t (the planners set 1 and 0; read at each call): the ELBO of
       losses8[0], and of enc_loss in losses8[3], is recon + kl_weight * mean_b sum_j max(k_bj, kl_floor); losses8[1], [2] stay raw. */
    double   kl_weight;
    double   kl_floor;
} dvae_train_info_plan_t;

/* Host only (callable without a GPU).  ksplit_hint 0 = choose.  DVAE_E_BADARG naming the limits for a size outside them. */
int dvae_train_info_plan(int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint, dvae_train_info_plan_t* plan);
/* The same with a mode (a set of DVAE_INFO_* bits; 0 equals dvae_train_info_plan field for field): stash and workspace depend on it.  Host
 * only.  DVAE_E_BADARG naming the choices for an unknown bit or both DVAE_INFO_AUX_* bits at once. */
int dvae_train_info_plan_mode(int y_dim, int z_dim, int h1, int h2, int64_t B, int ksplit_hint, int mode, dvae_train_info_plan_t* plan);
/* One-time setup of `ws` (item table, packed weight copies from `params`); synchronises the stream once. */
int dvae_train_info_init(const dvae_train_info_plan_t* plan, const float* params, void* ws, void* stream);
/* Rebuild both packed weight copies after `params` was written from outside. */
int dvae_train_info_repack(const dvae_train_info_plan_t* plan, const float* params, void* ws, void* stream);
/* rows kernel + weight-gradient kernel: x [B, 513] (ldx), y [B, y_dim] (ldy) -- or the frame stores under a gather table --, eps_noise
 * [B, z_dim] (required).  The gradients are left as plan->ksplit slabs. */
int dvae_train_info_grads(const dvae_train_info_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                          const float* eps_noise, float elbo_eps, void* stream);
/* apply kernel: g = grad_scale * (slabs summed in slab order); Adam at `step` (1-based); packed copies; losses8. */
int dvae_train_info_apply(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, int step, double lr, double beta1,
                          double beta2, double adam_eps, double grad_scale, float* losses8, void* stream);
/* dvae_train_info_grads + dvae_train_info_apply with grad_scale 1. */
int dvae_train_info_step(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* x, int64_t ldx,
                         const float* y, int64_t ldy, const float* eps_noise, float elbo_eps, int step, double lr, double beta1, double beta2,
                         double adam_eps, float* losses8, void* stream);
/* Forward and losses only (two launches): parameters, moments and gradient slabs are left alone. */
int dvae_train_info_eval(const dvae_train_info_plan_t* plan, void* ws, const float* x, int64_t ldx, const float* y, int64_t ldy,
                         const float* eps_noise, float elbo_eps, float* losses8, void* stream);
/* dvae_train_generic_reduce / _apply_flat for this step (every mode); losses8 as dvae_train_info_apply. */
int dvae_train_info_reduce(const dvae_train_info_plan_t* plan, void* ws, float* flat, int accumulate, float weight, float* losses8, void* stream);
int dvae_train_info_apply_flat(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step, double lr,
                               double beta1, double beta2, double adam_eps, double grad_scale, void* stream);
/* dvae_train_generic_apply_flat_clipped for this step (every mode): one norm over all 26 tensors. */
int dvae_train_info_apply_flat_clipped(const dvae_train_info_plan_t* plan, float* params, float* m, float* v, void* ws, const float* flat, int step,
                                       double lr, double beta1, double beta2, double adam_eps, double grad_scale, double max_norm, void* scratch,
                                       float* norm2_out, int32_t* skipped_counter, void* stream);

/* Per-kernel device time of the last `dvae_train_*` calls made with profiling enabled:
 * enable != 0 brackets each launch with hipEvents on its stream (a few us of host cost each).
 * dvae_train_profile_read synchronises and returns accumulated ms and launch counts
 * for {rows, wgrad, reduce, apply}, then clears them. */
int dvae_train_profile(int enable);
/* Diagnostic builds only: buf = device array of rows_grid * 32 uint64, filled with 100 MHz wall-clock stamps at the
 * phase boundaries of the rows kernel (NULL switches it off).  Never enabled by bench.py's timed region. */
int dvae_train_debug_stamps(void* buf);
int dvae_train_profile_read(double ms[4], int64_t calls[4]);

/* ---- direct gradient exchange of the data-parallel step (no reference call site: scripts/training_M2.py:31-33 is
 * single-device).  One launch per rank on the step's stream: slab sum -> reduce-scatter by pull -> all-gather by push over peer pointers
 * (hipIpc-mapped exchange buffers; xGMI on a multi-GPU node), see csrc/allreduce.hip.  Every wait for a peer is bounded by wall time
 * (dvae_comm_set_timeout_ms; default 20 s, env DVAE_COMM_TIMEOUT_MS): a missing or late peer ends the launch on EVERY rank with `out`
 * filled with NaN and dvae_comm_status() != 0 from then on, never with a hang and never with a stale sum.  The exchange buffer is
 * fine-grained device memory; where the platform has none, dvae_comm_create fails (no coarse-grained fallback).
 *   dvae_comm_create   allocates this rank's exchange buffer for n_floats and returns its IPC handle (DVAE_IPC_HANDLE_BYTES bytes);
 *   the caller gathers the handles of all ranks in rank order (e.g. torch.distributed.all_gather_object) and passes them to
 *   dvae_comm_connect; every rank must call dvae_allreduce_flat the same number of times.
 *   dvae_allreduce_flat: out[0 .. n) = sum over ranks of (sum over k < n_slabs of slabs[k * slab_stride + i]); `out` may alias slab 0. */
#define DVAE_IPC_HANDLE_BYTES 128   /* hipIpc handle + owning process + PCI address of the device */
typedef struct dvae_comm dvae_comm_t;
int dvae_comm_create(int rank, int world, int64_t n_floats, dvae_comm_t** out, unsigned char handle[DVAE_IPC_HANDLE_BYTES]);
int dvae_comm_connect(dvae_comm_t* c, const unsigned char* handles /* world x DVAE_IPC_HANDLE_BYTES, rank order */);
int dvae_allreduce_flat(dvae_comm_t* c, const float* slabs, int n_slabs, int64_t slab_stride, float* out, void* stream);
int dvae_comm_set_timeout_ms(dvae_comm_t* c, int64_t ms);   /* bound of every in-kernel wait of the following launches (0: one poll) */
int dvae_comm_status(dvae_comm_t* c, int* failed);      /* synchronises; *failed = 1 when a bounded wait expired on ANY rank since creation */
int dvae_comm_destroy(dvae_comm_t* c);

#ifdef __cplusplus
}
#endif
#endif /* DVAE_TRAIN_H */

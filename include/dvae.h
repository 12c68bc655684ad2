/* dvae.h -- C ABI of libdvae_hip.so: the MI355X (gfx950) hot path of
 * sp-uhh/disentangled-vae (VAE train step + STFT/ISTFT).
 *
 * The reference has no FFI of its own (pure Python on torch/librosa): the
 * drop-in boundary is its Python import surface.  Each entry
 * point below states which reference lines it replaces; the Python shells in
 * packages/ (same names/signatures as the reference) bind them with ctypes,
 * see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensor
 *     storage, passed as data_ptr()), fp32 row-major unless stated;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     kernels are enqueued on it and the call never synchronises;
 *   - the library allocates no user-visible memory; scratch comes from the
 *     caller (sizes from the *_workspace_bytes queries);
 *   - return 0 on success, non-zero (hipError_t or DVAE_E_*) on failure;
 *     dvae_last_error() returns a thread-local message; no exception crosses.
 */
#ifndef DVAE_H
#define DVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_ABI_VERSION 1

enum { DVAE_E_BADARG = 1001, DVAE_E_WORKSPACE = 1002, DVAE_E_UNSUPPORTED = 1003 };

/* activations of the fused Linear+act kernels */
enum { DVAE_ACT_NONE = 0, DVAE_ACT_TANH = 1, DVAE_ACT_RELU = 2, DVAE_ACT_SIGMOID = 3, DVAE_ACT_EXP = 4 };

int         dvae_abi_version(void);
const char* dvae_last_error(void);
/* 1 for the diagnostic build (-DDVAE_DIAG: product kernels + the measured-slower alternates behind their A/B switches), 0 for the default one. */
int dvae_build_has_diag(void);
/* number of HIP devices visible to the library (0 when none): lets the host fail loudly */
int         dvae_device_count(void);

/* ---------------------------------------------------------------------------
 * Layer-level ops: what packages/models/models.py modules call per nn.Linear.
 * ------------------------------------------------------------------------- */

/* out[B,N] = act([x0 | x1] @ W^T + bias)            (x1 may be NULL, k1 = 0)
 * replaces `x = torch.tanh(layer(x))` / `torch.relu(layer(x))` / `torch.sigmoid(...)` /
 * `torch.exp(self.reconstruction(x))` and the `torch.cat([x, y], dim=1)` in front of it:
 * packages/models/models.py:57-63, 102-105, 119-122, 201-202.  W is nn.Linear layout [N, k0+k1]. */
int dvae_linear_act_fwd(const float* x0, int k0, int ld0, const float* x1, int k1, int ld1,
                        const float* W, int ldw, const float* bias,
                        float* out, int ldo, int64_t B, int N, int act, void* stream);

/* dpre[B,N] = dout * act'(out)  (act' expressed through the OUTPUT: tanh 1-o^2, relu o>0,
 * sigmoid o(1-o), exp o); autograd of the activations above. */
int dvae_act_bwd(const float* dout, int ldd, const float* out, int ldo, float* dpre, int ldp,
                 int64_t B, int N, int act, void* stream);

/* din[B,K] (+)= dpre[B,N] @ W[:, koff:koff+K]     (autograd of F.linear wrt its input);
 * accumulate != 0 adds into din (sum of the mu / log_var heads, models.py:34-36). */
int dvae_linear_bwd_data(const float* dpre, int ldp, const float* W, int ldw, int koff,
                         float* din, int ldi, int64_t B, int N, int K, int accumulate, void* stream);

/* dW[N, k0+k1] = dpre^T @ [x0 | x1],  db[N] = colsum(dpre)   (autograd of F.linear wrt W, b).
 * Reduction over the B frames is split over `ksplit` workgroup slices combined with fp32
 * atomics when ksplit > 1 (pass 0 to let the library choose).  db may be NULL. */
int dvae_linear_bwd_weight(const float* dpre, int ldp, const float* x0, int k0, int ld0,
                           const float* x1, int k1, int ld1, float* dW, int ldw, float* db,
                           int64_t B, int N, int ksplit, void* stream);
/* The same with a DETERMINISTIC combination of the slices (what the drop-in modules call: the reference's own GPU path -- cuBLAS -- returns
 * the same bits for the same inputs): every slice writes its partial matrix into `workspace` (dvae_linear_bwd_weight_workspace_bytes; may be
 * NULL when that is 0) and a second launch sums the slices in ascending order. */
size_t dvae_linear_bwd_weight_workspace_bytes(int64_t B, int N, int Kin, int ksplit);
int dvae_linear_bwd_weight_det(const float* dpre, int ldp, const float* x0, int k0, int ld0,
                               const float* x1, int k1, int ld1, float* dW, int ldw, float* db,
                               int64_t B, int N, int ksplit, void* workspace, void* stream);

/* z = mu + exp(0.5*logvar) * eps     packages/models/models.py:9-22 (Stochastic.reparametrize) */
int dvae_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z,
                     int64_t n, void* stream);
/* dmu = dz ; dlogvar = dz * eps * 0.5 * exp(0.5*logvar) */
int dvae_reparam_bwd(const float* dz, const float* logvar, const float* eps, float* dmu,
                     float* dlogvar, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * Losses: packages/models/utils.py
 * ------------------------------------------------------------------------- */

/* elbo(x, r, mu, logvar, eps) -> out3 = {recon+KL, recon, KL}   utils.py:73-76.
 * recon = mean_b sum_f (x/r - log(x+eps) + log r - 1); KL = -0.5 mean_b sum_k (lv - mu^2 - e^lv).
 * Also writes kl_b[B] = per-frame KL (models.py:165-167 `_kld_v2`) when kl_b != NULL.
 * ws: dvae_elbo_workspace_bytes(B) bytes of scratch. */
size_t dvae_elbo_workspace_bytes(int64_t B);
int dvae_elbo_fwd(const float* x, int ldx, const float* r, int ldr, const float* mu,
                  const float* logvar, float eps, int64_t B, int F, int Z,
                  float* out3, float* kl_b, void* ws, void* stream);
/* gradients of g2[0]*recon + g2[1]*KL wrt r, mu, logvar; g2 = DEVICE pointer to
 * {g_loss + g_recon, g_loss + g_kl} (the upstream grads of the three returned scalars). */
int dvae_elbo_bwd(const float* x, int ldx, const float* r, int ldr, const float* mu,
                  const float* logvar, const float* g2, int64_t B, int F, int Z,
                  float* dr, int lddr, float* dmu, float* dlogvar, void* stream);
/* The same with the three upstream gradients of elbo()'s outputs (loss, recon, KL) as device scalars, each may be NULL (= 0):
 * d/d recon = *g_loss + *g_recon, d/d KL = *g_loss + *g_kl -- no host-side arithmetic on them (autograd hands them over separately). */
int dvae_elbo_bwd3(const float* x, int ldx, const float* r, int ldr, const float* mu, const float* logvar,
                   const float* g_loss, const float* g_recon, const float* g_kl, int64_t B, int F, int Z,
                   float* dr, int lddr, float* dmu, float* dlogvar, void* stream);

/* binary_cross_entropy family, utils.py:55-63: variant 0 = (r, x), 1 = _v2 (targets 0.5),
 * 2 = _v3 (targets r).  out1 = -mean_b sum_j [t log(r+eps) + (1-t) log(1-r+eps)]. */
int dvae_bce_fwd(const float* r, const float* t, float eps, int64_t B, int Y, int variant,
                 float* out1, void* ws, void* stream);
/* dr = g * d(bce)/dr ; dt (variant 0 only, may be NULL) */
int dvae_bce_bwd(const float* r, const float* t, float eps, const float* g, int64_t B, int Y,
                 int variant, float* dr, float* dt, void* stream);

/* ---------------------------------------------------------------------------
 * The rest of the loss zoo of packages/models/utils.py (reference :65-118; the earlier M2v3 / M2v4 experiments train on them).
 * Row layout [B, F] with leading dimensions like elbo; partial sums in double, no atomics; `ws` as for elbo.
 * ------------------------------------------------------------------------- */
/* per-frame Itakura-Saito rows recon_rows[b] = sum_f (x/r - log(x+eps) + log r - 1) (utils.py:68-71, 79) and, when kl_rows != NULL,
 * kl_rows[b] = -0.5 sum_k (logvar - mu^2 - exp(logvar)) (utils.py:80): L_loss / ikatura_saito_divergence */
int dvae_isrows_fwd(const float* x, int ldx, const float* r, int ldr, const float* mu, const float* logvar, float eps,
                    int64_t B, int F, int Z, float* recon_rows, float* kl_rows, void* stream);
/* gradients from per-frame upstream gradients g_recon_rows / g_kl_rows ([B], either may be NULL = zeros); outputs may be NULL */
int dvae_isrows_bwd(const float* x, int ldx, const float* r, int ldr, const float* mu, const float* logvar,
                    const float* g_recon_rows, const float* g_kl_rows, int64_t B, int F, int Z,
                    float* dr, int lddr, float* dmu, float* dlogvar, void* stream);
/* binary_cross_entropy_2classes (utils.py:65-66): -mean_b sum_j [t log(r1+eps) + (1-t) log(r2+eps)] */
int dvae_bce2_fwd(const float* r1, const float* r2, const float* t, float eps, int64_t B, int Y, float* out1, void* ws, void* stream);
int dvae_bce2_bwd(const float* r1, const float* r2, const float* t, float eps, const float* g, int64_t B, int Y,
                  float* dr1, float* dr2, float* dt, void* stream);
/* squared-error losses (utils.py:107-118), mean_b sum_f |d|^2.  mode 0 mean_square_error_signal: d = (y - yhat) x;
 * mode 1 mean_square_error_mask: d = y - yhat (x unused); mode 2 magnitude_spectrum_approxiamation_loss: d = s - yhat x with
 * x, y (= s) complex64 [B, F] and a real mask yhat.  Backward: dyhat always; dy, dx for the real modes (NULL = not wanted). */
int dvae_sqerr_fwd(int mode, const void* x, const void* y, const float* yhat, int64_t B, int F, float* out1, void* ws, void* stream);
int dvae_sqerr_bwd(int mode, const void* x, const void* y, const float* yhat, const float* g, int64_t B, int F,
                   float* dyhat, float* dy, float* dx, void* stream);

/* ---------------------------------------------------------------------------
 * Optimiser: torch.optim.Adam(lr, betas) as the scripts construct it
 * (scripts/training_M2.py:122); op order of torch's single-tensor Adam.
 * ------------------------------------------------------------------------- */
int dvae_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr,
                   double beta1, double beta2, double eps, int step, double grad_scale, void* stream);

/* ---------------------------------------------------------------------------
 * STFT / ISTFT: packages/processing/stft.py:13-60, 63-99 (librosa semantics, center=False
 * or pre-padded input), periodic Hann.  Indexing (pad rule, frame count) is decided on the
 * host in double precision by the Python shell; the kernels take the final frame count.
 * ------------------------------------------------------------------------- */

/* x: n samples (already end-padded / centre-padded by the caller), in_f64 selects double input.
 * out: layout 0 = [nfft/2+1, T] interleaved complex64 (column = frame, the librosa layout; the
 *      same bytes are the legacy torch.stft real view [nfft/2+1, T, 2] of stft_pytorch,
 *      packages/processing/stft.py:145-151);
 *      layout 1 = [T, nfft/2+1] float32 power |.|^2 (one training frame per row,
 *      scripts/create_train_set.py:152 / scripts/reconstruct_M2.py:153);
 *      layout 2 = [T, nfft/2+1] interleaved complex64 (row = frame): the values of layout 0 in the MEMORY order of
 *      librosa's result (librosa.stft fills a Fortran-ordered [nfft/2+1, T] array, packages/processing/stft.py:50-57);
 *      the host returns its transpose view, so the caller sees the reference's shape and strides.
 * window: nfft doubles (device).  Power-of-two nfft in [8, 2048] runs the LDS FFT; any other
 * even nfft <= 2048 (e.g. the wrapper's never-used 800-sample default) runs a plain DFT. */
int dvae_stft(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop,
              int64_t T, void* out, int layout, void* stream);

/* The transform of stft_pytorch (packages/processing/stft.py:123-152: torch.stft of a float32 tensor with torch.hann_window) in ITS
 * arithmetic: window product, FFT and result in float32 (dvae_stft computes in double whatever the input type -- the arithmetic of
 * stft(), where librosa multiplies by a float64 window).  nfft 1024 / hop 256 only (every caller); window: nfft floats (device);
 * layout 2 = [T, 513] interleaved complex64, row = frame -- the memory of the legacy torch.stft result, whose [513, T, 2] real view
 * is the transpose view of it; layout 1 = [T, 513] float32 re * re + im * im (packages/data_handling.py:136).  Signal and result
 * below 2 GB each.  Any other size / layout: DVAE_E_ARG (use dvae_stft). */
int dvae_stft_f32(const float* x, int64_t n, const float* window, int nfft, int hop, int64_t T, void* out, int layout, void* stream);

/* S: complex64 [nfft/2+1, ldT] of which the first T columns (frames) are used;
 * y[out_len] float32 = overlap-add of window * irfft(S[:, t]) (float32 accumulation in frame
 * order, as librosa), divided by the window sum-square where it exceeds FLT_MIN, read from
 * sample `start` on, zero padded / trimmed to out_len.  ws: dvae_istft_workspace_bytes_hop(T, nfft, hop) bytes
 * (nfft 1024 / hop 256 -- every caller of the reference -- runs inverse FFT and overlap-add in one kernel: 16 bytes below 1024
 * frames, T * 513 complex64 from there on (dvae_istft transposes long bin-major input into it and runs the frame-major walk);
 * otherwise T * nfft doubles, which dvae_istft_workspace_bytes(T, nfft) always returns). */
size_t dvae_istft_workspace_bytes(int64_t T, int nfft);
size_t dvae_istft_workspace_bytes_hop(int64_t T, int nfft, int hop);
int dvae_istft(const void* S, int64_t T, int64_t ldT, const double* window, int nfft, int hop,
               int64_t start, float* y, int64_t out_len, void* ws, void* stream);
/* The same transform of a FRAME-major spectrogram: S complex64 [T, ldF], row t = frame t (its first nfft/2+1 entries) -- the
 * memory order of a Fortran-ordered [nfft/2+1, T] array such as librosa.stft / dvae_stft layout 2 return.  Results are
 * bit-identical to dvae_istft on the transposed array (packages/processing/stft.py:63-99). */
int dvae_istft_frames(const void* S, int64_t T, int64_t ldF, const double* window, int nfft, int hop,
                      int64_t start, float* y, int64_t out_len, void* ws, void* stream);

/* Ragged batches of the two transforms above (nfft 1024 / hop 256 only, which every caller of the reference uses; any other size:
 * DVAE_E_BADARG naming the single-signal functions).  U utterances are packed end to end; a work item is one utterance and a run of at
 * most `chunk` of its frames, and `tables` (device int64) starts with the prefix of the per-utterance item counts, items[U + 1]
 * (items[0] = 0, items[U] = n_items).  Every frame and sample is bit-identical to the single-signal call on the utterance alone.  The
 * kernels check each table entry against the scalar extents before touching memory: a bad entry drops that utterance's work, it is
 * never an out-of-bounds access.  Each utterance (not the batch) must stay below 2 GB of input and of output.
 *
 * dvae_stft_batch: the transform of dvae_stft (double arithmetic) of x (n samples, float64 when in_f64, else float32: the padded
 * signals, as dvae_stft takes them), output frame-major [T_total][513] in layout 1 (float32 power) or 2 (complex64).
 *   tables = [items (U + 1) | frames (U + 1) | x0 (U)]: utterance u's frames are output rows [frames[u], frames[u + 1]) and read
 *   samples from x0[u] on ((frames[u + 1] - frames[u] - 1) * 256 + 1024 of them). */
int dvae_stft_batch(const void* x, int in_f64, int64_t n, const double* window, int nfft, int hop, int U, const int64_t* tables,
                    int64_t n_items, int chunk, int64_t T_total, void* out, int layout, void* stream);
/* dvae_istft_batch: the transform of dvae_istft_frames of S complex64 [T_total][513] (frame-major rows).
 *   tables = [items (U + 1) | f0 (U) | nfr (U) | y0 (U) | len (U) | gcol (U)]: utterance u transforms rows [f0[u], f0[u] + nfr[u])
 *   and writes y[y0[u] ... y0[u] + len[u]) (y0 even), `start` as in dvae_istft_frames, zeros past the utterance's own signal.
 *   gain0 (may be NULL): every bin is first scaled by a real gain, re = g xr and im = g xi in float32 (numpy's `WF * X` of a float32
 *   gain and a complex64 spectrogram), g = gain0[k * ldg + gcol[u] + t] for bin k of the utterance's frame t (McemBatch's bin-major
 *   Wiener gains, 513 * ldg floats below 2 GB); gain1 (may be NULL) does the same into y1 in the same launch. */
int dvae_istft_batch(const void* S, int64_t T_total, const double* window, int nfft, int hop, int U, const int64_t* tables, int64_t n_items,
                     int chunk, int64_t start, float* y, int64_t y_total, const float* gain0, const float* gain1, int64_t ldg, float* y1,
                     void* stream);

/* The inverse transform of istft_pytorch (packages/processing/stft.py:154-190: torch.istft of a complex64 tensor with
 * torch.hann_window, center handled by `start` / `out_len` as above) in ITS arithmetic: inverse FFT, window product, overlap-add and
 * the division by the window envelope in float32 (dvae_istft computes in double -- the arithmetic of istft(), librosa's).  nfft 1024 /
 * hop 256 only; window: nfft floats (device).  frames = 0: S is [513][ld] (bin-major, ld >= T), transposed into ws (T * 513
 * complex64) first; frames = 1: S is [T][ld] (frame-major, ld >= 513), read in place, ws may be null.  Any other size: DVAE_E_ARG. */
int dvae_istft_f32(const void* S, int64_t T, int64_t ld, int frames, const float* window, int nfft, int hop,
                   int64_t start, float* y, int64_t out_len, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Fused train step (the build's own harness; mirrors scripts/training_M1.py:134-139,
 * scripts/training_M2.py:142-147, scripts/training_M2_info_vad.py:159-198).
 * Declared in dvae_train.h.
 * ------------------------------------------------------------------------- */

/* ---- frame store (GPU-resident replacement of HDF5CleanSpectrogramLabeledFrames, packages/data_handling.py:19-67) ----
 * dvae_transpose: the on-disk (F, N) matrix (one frame per column, scripts/create_train_set.py:116) -> frames-major
 *   [N][F] rows, the layout the train step reads.  rows/cols describe `in`; rows <= 2M.
 * dvae_gather_rows: dst[i] = src[idx[i]] (epoch shuffle: what DataLoader(shuffle=True) does frame by frame,
 *   scripts/training_M2.py:84-86).  Indices outside [0, nsrc) are skipped and counted in *bad_count (device int,
 *   may be NULL). */
int dvae_transpose(const float* in, int64_t rows, int64_t cols, int64_t ldi, float* out, int64_t ldo, void* stream);
int dvae_gather_rows(const float* src, int64_t ld, int64_t nsrc, const int64_t* idx, int64_t n, int cols, float* dst,
                     int64_t ldd, int* bad_count, void* stream);

/* ---- train-set statistics (csrc/frame_stats.hip): X_train_mean / X_train_std of scripts/create_train_set.py:123-219 ----
 * dvae_frame_stats: per-bin mean and standard deviation over the frames of X, float32 rows [n_store][ld] with ld >= 513 (the layout of
 *   the frame store and of a FrameBatch's rows), into mean[513] and std[513] (device float32).  rows == NULL: every frame; else rows is
 *   a device int64 table of n_rows indices into the store (a train split of a larger store; an index may repeat).
 *   Contract: the reference's formula evaluated in double,
 *     s = sum x,  q = sum x^2 (the square of a float32 is exact in double),  mean = s / n,  std = sqrt((q - n mean^2) / (n - 1)),
 *   every operation rounded on its own, both results rounded to float32 at the end.  One deliberate departure from numpy: where rounding
 *   makes q - n mean^2 negative (a constant bin), std is 0, not NaN.
 *   An index outside [0, n_store) is never dereferenced: it is counted in *bad_count (device int, may be NULL) and left out of both sums;
 *   n is the number of valid indices.  n < 2 is refused (DVAE_E_BADARG) where the host can see it -- n_store < 2 without a table,
 *   n_rows < 2 with one --; a table that leaves fewer than two valid indices gives NaN in every bin.
 *   Order of summation: two launches on `stream`, no host synchronisation.  Chunk c is the frames (or table entries)
 *   [c C, (c + 1) C), C = DVAE_FRAME_STATS_CHUNK, a constant whatever the grid; within a chunk wave w of four adds the frames w, w + 4, ...
 *   ascending into its own accumulators, then the waves are added in wave order; the finalising launch, one thread a bin, adds the chunks
 *   in chunk order.  No floating-point atomics: the result depends on (X, rows) alone -- the same bits on every run, and for a table
 *   of valid indices the bits of the contiguous copy of those rows (an index left out adds nothing but keeps its place in the order).
 *   workspace: dvae_frame_stats_workspace_bytes(n) bytes of device memory, 8-byte aligned (0 for n < 1), n = n_rows or n_store. */
#define DVAE_FRAME_STATS_CHUNK 4096
int dvae_frame_stats_chunk(void);
size_t dvae_frame_stats_workspace_bytes(int64_t n);
int dvae_frame_stats(const float* X, int64_t ld, int64_t n_store, const int64_t* rows, int64_t n_rows, float* mean, float* std,
                     int* bad_count, void* workspace, void* stream);

/* ---- label makers of the training-set builders (packages/processing/target.py) ----
 * dvae_vad_labels: clean_speech_VAD (target.py:5-56, center=False): vad[t] = E[t] > 10^vad_threshold * min_t E[t],
 *   E[t] = sum of squares of frame t (double accumulation); y: n samples (float32, or float64 when in_f64), the zero
 *   end-pad of `hop` samples is implied (frames may reach n + hop); frames from the host-side pad rule.  vad: (frames).
 * dvae_ibm_labels: clean_speech_IBM (target.py:58-70): mask = 20 log10(|S| + eps) > max - ibm_threshold over the whole
 *   (rows, cols) complex64 matrix S; vad_gate (cols) or NULL multiplies each column (noise_robust_clean_speech_IBM,
 *   target.py:72-104).  mask: (rows, cols) float32. */
size_t dvae_vad_workspace_bytes(int64_t frames);
int dvae_vad_labels(const void* y, int in_f64, int64_t n, int nfft, int hop, int64_t frames, double vad_threshold,
                    float* vad, void* workspace, void* stream);
size_t dvae_ibm_workspace_bytes(void);
int dvae_ibm_labels(const void* S, int64_t rows, int64_t cols, float eps, float ibm_threshold, const float* vad_gate,
                    float* mask, void* workspace, void* stream);

/* Ragged batches of the training-set front end (scripts/create_train_set.py:133-170 over a whole split): U utterances packed end to
 * end, a work item is one utterance and a run of at most `chunk` of its samples / frames / bins, and `tables` (device int64) starts
 * with the prefix of the per-utterance item counts, items[U + 1] (items[0] = 0, items[U] = n_items, items[u + 1] - items[u] =
 * ceil(extent_u / chunk)).  The kernels check every table entry against the scalar extents before touching memory: a bad entry drops
 * that utterance's work.  Two launches each on `stream`, no host synchronisation; the per-utterance results are bit-identical to the
 * single-signal calls on the utterance alone.
 *
 * dvae_peak_normalise_batch: x[x0[u] : x0[u] + len[u]] /= max |x| over that range (IEEE double division: numpy's
 *   `speech / np.max(np.abs(speech))`, create_train_set.py:137), in place; peak[u] = the maximum (0 for an all-zero utterance, which
 *   then holds NaN; a NaN sample makes the peak NaN, as np.max).  Samples outside every range are not touched.
 *   tables = [items (U + 1) | x0 (U) | len (U)], chunk in samples; workspace: dvae_peak_normalise_workspace_bytes(n_items).
 * dvae_vad_labels_batch: dvae_vad_labels of every utterance (any nfft / hop): utterance u reads y[x0[u] : x0[u] + n[u]] (zeros past
 *   n[u]; frames may reach n[u] + hop) and writes vad[frame_off[u] : frame_off[u + 1]].  tables = [items (U + 1) | x0 (U) | n (U) |
 *   frame_off (U + 1)], chunk in frames, T_total = the length of vad; workspace: dvae_vad_batch_workspace_bytes(T_total, n_items).
 * dvae_ibm_labels_batch: dvae_ibm_labels of every segment S[e0[u] : e0[u] + count[u]] (complex64, a row-major (count / cols, cols)
 *   matrix: a frame-major [T_u, 513] slice of packed frames or a host [513, T_u] matrix) into the same elements of mask (n of each);
 *   vad_gate (n_gate floats) or NULL: element i of segment u is multiplied by vad_gate[g0[u] + i % cols[u]].  tables = [items (U + 1)
 *   | e0 (U) | count (U) | cols (U) | g0 (U)], chunk in bins; workspace: dvae_ibm_batch_workspace_bytes(n_items). */
size_t dvae_peak_normalise_workspace_bytes(int64_t n_items);
int dvae_peak_normalise_batch(double* x, int64_t n, int U, const int64_t* tables, int64_t n_items, int chunk, double* peak,
                              void* workspace, void* stream);
size_t dvae_vad_batch_workspace_bytes(int64_t T_total, int64_t n_items);
int dvae_vad_labels_batch(const void* y, int in_f64, int64_t n, int nfft, int hop, double vad_threshold, int U, const int64_t* tables,
                          int64_t n_items, int chunk, int64_t T_total, float* vad, void* workspace, void* stream);
size_t dvae_ibm_batch_workspace_bytes(int64_t n_items);
int dvae_ibm_labels_batch(const void* S, int64_t n, float eps, float ibm_threshold, int U, const int64_t* tables, int64_t n_items,
                          int chunk, const float* vad_gate, int64_t n_gate, float* mask, void* workspace, void* stream);

/* ---- scoring (packages/metrics.py:12-82: si_sdr_components, energy_ratios, si_sdr_leroux) ----
 * dvae_si_ratios_batch: the scale-invariant energy ratios of U utterances in three launches on `stream`, no host synchronisation,
 *   no atomics.  s_hat (the estimate), s (clean speech) and n (noise, or NULL: the n-free form of si_sdr_leroux) are packed device
 *   buffers of n_s_hat / n_s / n_n elements, float32 or float64 by their flags; all arithmetic is in double.  With
 *   alpha_s = <s_hat, s> / |s|^2 and alpha_n = <s_hat, n> / |n|^2 (IEEE division), per utterance
 *     ratios[u] = 10 log10 of { |alpha_s s|^2 / |s_hat - alpha_s s|^2,  |alpha_s s|^2 / |alpha_n n|^2,
 *                               |alpha_s s|^2 / |s_hat - alpha_s s - alpha_n n|^2 }            (SI-SDR, SI-SIR, SI-SAR in dB)
 *     sums[u]   = { <s_hat, s>, |s|^2, <s_hat, n>, |n|^2, |s_hat - alpha_s s|^2, |s_hat - alpha_s s - alpha_n n|^2,
 *                   alpha_s^2 |s|^2, alpha_n^2 |n|^2 }
 *   The residuals are formed per sample with the reference's operations: e_art = (s_hat - alpha_s s) - alpha_n n, and the SI-SDR
 *   denominator is |alpha_n n + e_art|^2 with n, |s_hat - alpha_s s|^2 without.  Without n the entries that need it are NaN.  IEEE
 *   semantics throughout, as numpy gives the reference: an all-zero s or n gives NaN (in all three ratios), a perfect estimate +inf.  ratios [U, 3] or sums [U, 8] may be NULL, not both.
 *   tables (device int64) = [items (U + 1) | s_hat0 (U) | s0 (U) | n0 (U) | len (U)]: utterance u is s_hat[s_hat0[u] : s_hat0[u] +
 *   len[u]] and likewise in s and n (n0 is ignored without n); a work item is one utterance and a run of at most DVAE_SI_CHUNK of its
 *   samples, items[u + 1] - items[u] = ceil(len[u] / DVAE_SI_CHUNK), items[U] = n_items.  The chunk is fixed, and an utterance's
 *   partial sums are added in item order, so its results do not depend on what else is in the batch and repeat bit for bit.  The
 *   kernels check every table entry against the scalar extents before touching memory: a bad entry leaves NaN in that utterance's
 *   rows.  workspace: dvae_si_ratios_workspace_bytes(n_items). */
#define DVAE_SI_CHUNK 4096
size_t dvae_si_ratios_workspace_bytes(int64_t n_items);
int dvae_si_ratios_batch(const void* s_hat, int64_t n_s_hat, int s_hat_f64, const void* s, int64_t n_s, int s_f64, const void* n,
                         int64_t n_n, int n_f64, int U, const int64_t* tables, int64_t n_items, double* ratios, double* sums,
                         void* workspace, void* stream);

/* ---- noisy mixtures at a target SNR (scripts/create_test_set.py:95-115: process_save_utt) ----
 * dvae_mix_snr_batch: speech, noise and mixture of U utterances in at most five launches on `stream` whatever U is, no host
 *   synchronisation, no atomics.  speech and noise are packed device buffers of n_speech / n_noise elements, float32 or float64 by
 *   their flags; all arithmetic is in double, every operation rounded on its own in the reference's order.  Per utterance, over its
 *   len samples:
 *   1 p = max |speech|, s = speech / p (IEEE division per sample); normalise_speech == 0: s = speech, and p is reported as 1.
 *   2 Ps = sum s^2, Pn = sum noise^2 (squares rounded, then added).
 *   3 k = (Ps snr_factor[u]) / Pn, g = sqrt(k), v = noise g.  snr_factor (device, [U]) is np.power(10, -snr_dB / 10) from the host:
 *     the reference's own bits, no pow in the kernel.
 *   4 norm = max(|s|, |v|, |s + v|).
 *   5 out_speech = s / norm, out_noise = v / norm, out_mix = (s + v) / norm: the rounded sum divided, not the sum of the quotients.
 *   6 stats[u] = {p, Ps, Pn, k, norm, 10 log10(sum out_speech^2 / sum out_noise^2)} (the achieved SNR, from the double quotients
 *     before any rounding to float32); stats [U, 6] may be NULL.
 *   The three outputs are three buffers of n_out elements each, float64, or float32 when out_f64 == 0 (one more rounding of the
 *   double result).  Maxima propagate NaN as numpy's; no clamping, no epsilon: an all-zero noise segment gives NaN outputs (0 inf),
 *   an all-zero speech under normalise_speech NaN.
 *   tables (device int64) = [items (U + 1) | speech0 (U) | noise0 (U) | out0 (U) | len (U) | out_extent (U)]: utterance u reads
 *   speech[speech0[u] : speech0[u] + len[u]] and noise[noise0[u] : ...] and writes [out0[u], out0[u] + out_extent[u]) of all three
 *   outputs: len[u] samples, then zeros (out_extent[u] >= len[u]: room for the end pad of a later STFT).  Input ranges may overlap or
 *   repeat; output ranges may not overlap, and no output may alias an input.  Output samples outside every range are not touched.  A
 *   work item is one utterance and a run of at most DVAE_MIX_CHUNK of its samples, items[u + 1] - items[u] = ceil(len[u] /
 *   DVAE_MIX_CHUNK), items[U] = n_items.  The chunk is fixed, the sums are added in item order and a maximum is exact in any order, so
 *   an utterance's results do not depend on what else is in the batch and repeat bit for bit.  The kernels check every table entry
 *   against n_speech, n_noise and n_out before touching memory: a bad entry leaves NaN in that utterance's stats row and writes
 *   nothing else for it.  workspace: dvae_mix_snr_workspace_bytes(n_items, U). */
#define DVAE_MIX_CHUNK 4096
size_t dvae_mix_snr_workspace_bytes(int64_t n_items, int U);
int dvae_mix_snr_batch(const void* speech, int64_t n_speech, int speech_f64, const void* noise, int64_t n_noise, int noise_f64, int U,
                       const int64_t* tables, int64_t n_items, const double* snr_factor, int normalise_speech, void* out_speech,
                       void* out_noise, void* out_mix, int64_t n_out, int out_f64, double* stats, void* workspace, void* stream);

/* ---- intelligibility: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) ----
 * dvae_estoi_batch: the score d[u] of U utterances (x clean, y processed, equal lengths) in six
 *   launches on `stream` whatever U is, no host synchronisation, no atomics, double arithmetic throughout.  The contract is the
 *   algorithm below, laid out the way the pystoi package does it and restated in numpy by tests/estoi_ref.py; the package itself is
 *   not available to this repository, so parity with it is unpinned.  FS = 10000, frames of 256 at hop 128, w = hanning(258)[1:-1],
 *   EPS = 2^-52.
 *   1 resample (taps != NULL): output k of ceil(len p / q) = p sum_j taps[j] xu[k q + j - L], xu = the signal zero-stuffed by p and
 *     zero outside it, taps [2 L + 1] built by the host (scipy.signal.resample_poly(x, p, q, window=taps)); p / q = FS / fs reduced.
 *     taps == NULL (p = q = 1, L = 0): the samples as they are.
 *   2 silent frames: frames of x and y at i = 0, 128, ... with i + 256 <= n; e_j = 20 log10(|w x_j| + EPS); frame j of BOTH signals is
 *     kept iff (max e - 40) - e_j < 0; the kept windowed frames are overlap-added at hop 128 in kept order.
 *   3 spectra: frames of the result at i = 0, 128, ... with i + 256 < n (strict), windowed by w again, 512-point real FFT, power.
 *   4 bands: tob[m][b] = sqrt(sum of the power of bins [bands[b], bands[b + 1])), b < DVAE_ESTOI_BANDS (bands: 16 device int64,
 *     0 <= bands[b] <= bands[b + 1] <= 256).
 *   5 segments m = 30 ... M of the 15 x 30 blocks of frames m - 30 ... m - 1; fewer than 30 frames: d = 1e-5.
 *     extended (ESTOI): rows minus their mean, divided by (norm + EPS), then the same by column; d = mean over segments of sum(xn yn) / 30.
 *     otherwise (STOI): alpha = |x_row| / (|y_row| + EPS), y' = min(alpha y, x (1 + 10^(15 / 20))), rows of x and y' minus their mean and
 *     divided by (norm + EPS); d = mean over segments of sum(y'n xn) / 15.
 *   x / y are packed device buffers of n_x / n_y elements, float32 or float64 by their flags.  tables (device int64) = [items_res (U + 1)
 *   | items_frame (U + 1) | items_seg (U + 1) | x0 (U) | y0 (U) | len (U) | r0 (U) | f0 (U)]: utterance u is x[x0[u] : x0[u] + len[u]] and
 *   y[y0[u] : ...]; with n10 = ceil(len p / q) and J = frames of rule 2 in n10 samples, its resampled signals live at r0[u] of the n_res
 *   workspace samples and its per-frame data at f0[u] of the n_frames workspace rows (r0, f0: prefixes of n10 and J), and it has
 *   max(1, ceil(n10 / (DVAE_ESTOI_RES_RUN p))), max(1, ceil(J / DVAE_ESTOI_FRAME_RUN)) and max(1, ceil(max(J - 30, 0) /
 *   DVAE_ESTOI_SEG_RUN)) work items in the three prefixes (whose last entries are n_res_items, n_frame_items, n_seg_items).  The runs
 *   are fixed and every reduction has a fixed order, so an utterance's score does not depend on what else is in the batch and repeats
 *   bit for bit.  The kernels check every table entry against the scalar extents before touching memory: a bad entry leaves NaN in
 *   d[u] (and -1 in info[u]).  d [U] float64; info [U, 3] int64 or NULL: resampled length, kept frames, segments; tob [2, n_frames,
 *   DVAE_ESTOI_BANDS] float64 or NULL: a debug output, the bands of x then y, utterance u's M rows from row f0[u] (the rest of its J
 *   rows untouched).  workspace: dvae_estoi_workspace_bytes(n_res, n_frames, n_seg_items, U). */
#define DVAE_ESTOI_BANDS 15
#define DVAE_ESTOI_RES_RUN 256
#define DVAE_ESTOI_FRAME_RUN 16
#define DVAE_ESTOI_SEG_RUN 8
size_t dvae_estoi_workspace_bytes(int64_t n_res, int64_t n_frames, int64_t n_seg_items, int U);
int dvae_estoi_batch(const void* x, int64_t n_x, int x_f64, const void* y, int64_t n_y, int y_f64, int U, const int64_t* tables,
                     int64_t n_res_items, int64_t n_frame_items, int64_t n_seg_items, int64_t n_res, int64_t n_frames,
                     const double* taps, int p, int q, int L, const double* window, const int64_t* bands, int extended, double* d,
                     int64_t* info, double* tob, void* workspace, void* stream);

/* ---- resampling (packages/dataset/qut_database.py:63-83: preprocess_noise) ----
 * dvae_resample_batch: U signals resampled by the rational factor p / q in one launch on `stream`, no host synchronisation, no
 *   atomics, double arithmetic.  The contract is the algorithm below -- the one of step 1 of dvae_estoi_batch, for any target rate --
 *   restated in numpy by tests/estoi_ref.py::resample; the reference's librosa.resample (resampy's kaiser_best table) is not
 *   available to this repository, so parity with it is unpinned.
 *   Given odd-length taps h[0 .. 2 L] (float64), integers p, q >= 1 with p != q, and a signal x[0 .. n - 1]:
 *   - the output has ceil(n p / q) samples;
 *   - out[k] = p sum_t h[j0 + t p] x[src0 + t] with j0 = (L - k q) mod p, src0 = (k q + j0 - L) / p (the division is exact),
 *     t = 0 .. nt - 1, nt = (2 L - j0) / p + 1 (no term when j0 > 2 L), x zero outside [0, n);
 *   - the sum is accumulated in double from 0.0 with t ascending, one fma per tap, and then multiplied by (double)p; a float32 input
 *     converts to double exactly; a float32 output is the double result rounded once.
 *   The order is fixed, so a signal's output does not depend on the tiling, on its place in the batch or on the batch, and repeats
 *   bit for bit.  This is scipy.signal.resample_poly(x, p, q, window=h) up to the order of the sum.
 *   x is a device buffer of n_x elements, float64 when x_f64, else float32; sample i of signal u is x[x0[u] + i stride] (stride >= 1
 *   elements: channel c of an interleaved [n, C] recording is x0 = c, stride = C, read in place).  y is a device buffer of n_y
 *   elements, float64 when y_f64, else float32; signal u writes y[y0[u] ... y0[u] + ceil(len[u] p / q)), nothing else is touched;
 *   output ranges may not overlap and y may not alias x.
 *   taps (device, float64) are PHASE-MAJOR, [p][nt_max] with nt_max = 2 L / p + 1: taps[j0 nt_max + t] = h[j0 + t p], 0 past the
 *   row's own nt (never read).  p, q <= 2^15, L <= 2^24 as in dvae_estoi_batch.
 *   tables (device int64) = [items (U + 1) | x0 (U) | len (U) | y0 (U)], 1 <= len <= 2^31.  A work item is one signal and a run of
 *   dvae_resample_run(p, q, L) of its outputs, items[u + 1] - items[u] = ceil(ceil(len[u] p / q) / run), items[U] = n_items.  The
 *   run is the largest multiple of 64 p (p <= 16; else of 64), at most DVAE_RESAMPLE_MAX_RUN, whose input span ceil((run - 1) q / p) +
 *   1 + nt_max fits the DVAE_RESAMPLE_SPAN samples that a wave stages in LDS; a ratio and filter whose smallest run does not fit
 *   (dvae_resample_run = 0: roughly q / p > 16, or more than a thousand taps per output) is refused with DVAE_E_BADARG.  The kernel
 *   checks every table entry against n_x, n_y and the item counts before touching memory: a bad entry drops that signal's work (its
 *   outputs stay as they were). */
#define DVAE_RESAMPLE_SPAN 1240
#define DVAE_RESAMPLE_MAX_RUN 4096
int dvae_resample_run(int p, int q, int L);
int dvae_resample_batch(const void* x, int64_t n_x, int x_f64, int64_t stride, void* y, int64_t n_y, int y_f64, int U,
                        const int64_t* tables, int64_t n_items, const double* taps, int p, int q, int L, void* stream);

/* ---- classifier labels and their scores (scripts/evaluate_ntcd_M2_info_vad.py:175-219, packages/models/utils.py:120-159) ----
 * dvae_classify_batch: the reference's Classifier without batch norm (packages/models/models.py:41-63), 513 -> 128 (relu) -> 128
 *   (relu) -> y_dim (sigmoid), y_dim 1 or 513, over the frames of a ragged batch in one launch on `stream`, no host synchronisation,
 *   no atomics, float32 throughout.
 *   Input, N rows: src_complex = 1: complex64 frames [N][513] (what dvae_stft_batch writes in layout 2, ld = 513); the power of a bin
 *   is formed in the kernel as a = numpy's complex64 magnitude (larger * sqrt(fma(r, r, 1)), r = smaller / larger, correctly rounded
 *   float32 operations), p = a * a rounded once -- the bits of dvae_mcem_spec_init and of `(np.abs(X) ** 2).astype(np.float32)`.
 *   src_complex = 0: float32 power rows, row r at src + r ld, ld >= 513.
 *   weights (device, float32, dvae_classify_weights_floats(y_dim) of them; 0 for a y_dim not covered): the state_dict tensors in
 *   their own [out][in] layout, one after the other: W1 [128][513] | b1 [128] | W2 [128][128] | b2 [128] | W3 [y_dim][128] | b3 [y_dim].
 *   Per frame with power p:  h1[j] = max(0, (sum_k p[k] W1[j][k]) + b1[j]);  h2[j] = max(0, (sum_k h1[k] W2[j][k]) + b2[j]);
 *   logit[c] = (sum_k h2[k] W3[c][k]) + b3[c];  soft = 1 / (1 + expf(-logit));  hard = soft > 0.5 ? 1 : 0, decided from the float32
 *   soft that is stored.  Every sum is ONE float32 chain from 0 with k ascending (on the matrix unit two products per step, as
 *   v_mfma_f32_32x32x2_f32 adds them; layer 1 is padded with zero products to k = 544), the bias added after it: the order does not
 *   depend on the frame's place in a tile, on the tile's place in the grid or on the batch, so a frame gives the same bits alone, in
 *   any batch and from run to run.
 *   frame_off_host (HOST int64 [U + 1]): utterance u is rows frame_off[u] .. frame_off[u + 1] - 1.  It is checked here, before
 *   anything is launched: 0 <= frame_off[0], non-decreasing, frame_off[U] <= N, else DVAE_E_BADARG naming the utterance.  Rows
 *   outside [frame_off[0], frame_off[U]) are neither read nor written.
 *   soft, hard [N][y_dim] float32 (the training layout of Y); logits [N][y_dim] or NULL.
 * dvae_label_counts_batch: the confusion counts of f1_loss per utterance.  pred, truth: float32 rows [N][y_dim] with leading dimensions
 *   ldp, ldt >= y_dim; an element counts as 1 when it is not zero.  counts [U][4] int64 = tp, tn, fp, fn over all y_dim (frame_off[u + 1]
 *   - frame_off[u]) elements of utterance u; zeroed and then added to with integer vector atomics on `stream` (integer sums: any
 *   order gives the same result).  frame_off_host is checked as above; frame_off_dev is the same table on the device (the kernel
 *   clamps what it reads from it to [frame_off[0], frame_off[U]], so a copy that differs miscounts but reads nothing outside the rows). */
size_t dvae_classify_weights_floats(int y_dim);
int dvae_classify_batch(const void* src, int src_complex, int64_t ld, int64_t N, int U, const int64_t* frame_off_host,
                        const float* weights, int y_dim, float* soft, float* hard, float* logits, void* stream);
int dvae_label_counts_batch(const float* pred, int64_t ldp, const float* truth, int64_t ldt, int64_t N, int y_dim, int U,
                            const int64_t* frame_off_host, const int64_t* frame_off_dev, int64_t* counts, void* stream);

/* ---- the VAE encoder over a ragged batch (packages/models/mcem.py:200, 364; scripts/reconstruct_ntcd_M2.py:231-358) ----
 * dvae_encode_batch: the reference's Encoder([513 + y_dim, [128, 128], 16]) (packages/models/models.py:91-105), [x | y] -> 128 (tanh) ->
 *   128 (tanh) -> {mu 16, log_var 16}, y_dim 0 (M1 and the x-only encoders of _v3 / _v5), 1 or 513 (M2), over the frames of a ragged
 *   batch in one launch on `stream`, no host synchronisation, no atomics, float32 throughout.
 *   Input as for dvae_classify_batch: src_complex = 1: complex64 frames [N][513], the power formed in the kernel with the bits of
 *   dvae_mcem_spec_init; src_complex = 0: float32 power rows, ld >= 513.  y: float32 label rows, row r at y + r ldy, ldy >= y_dim;
 *   required exactly when y_dim > 0.
 *   weights (device, float32, dvae_encode_weights_floats(y_dim) of them; 0 for a y_dim not covered): the state_dict tensors in their
 *   own [out][in] layout, one after the other: W1 [128][513 + y_dim] | b1 [128] | W2 [128][128] | b2 [128] | Wmu [16][128] | bmu [16] |
 *   Wlv [16][128] | blv [16].
 *   Per frame with power p and labels l, v = [p | l] as torch.cat([x, y], 1) lays it:  h1[j] = tanhf((sum_k v[k] W1[j][k]) + b1[j]);
 *   h2[j] = tanhf((sum_k h1[k] W2[j][k]) + b2[j]);  mu[c] = (sum_k h2[k] Wmu[c][k]) + bmu[c];  log_var likewise;
 *   z[c] = mu[c] + expf(0.5f log_var[c]) eps[c], product and sum rounded separately (log_var.mul(0.5).exp_(), mu.addcmul(std, eps)).
 *   Every sum is ONE float32 chain from 0 with k ascending (on the matrix unit two products per step, as v_mfma_f32_32x32x2_f32 adds
 *   them; layer 1 is padded with zero products to the next multiple of 32), the bias added after it: the order does not depend on the
 *   frame's place in a tile, on the tile's place in the grid or on the batch, so a frame gives the same bits alone, in any batch and
 *   from run to run.
 *   frame_off_host (HOST int64 [U + 1]) as for dvae_classify_batch: checked before anything is launched; rows outside
 *   [frame_off[0], frame_off[U]) are neither read nor written.
 *   Outputs, each may be NULL, at least one must not be: mu, log_var [N][16]; z [N][16], which needs eps [N][16]; Z [16][ntot], the
 *   layout of McemBatch: mu of row r of utterance u goes to column col[u] + (r - frame_off[u]), every other column is left as it is.
 *   Z needs col_host (HOST int64 [U]: checked here against frame_off_host and ntot: col[u] >= col[u - 1] + frames of u - 1,
 *   col[u] + frames of u <= ntot, else DVAE_E_BADARG naming the utterance) and tables_dev (DEVICE int64 [frame_off (U + 1) | col (U)],
 *   the table of dvae_mcem_spec_init; a frame whose column by the device copy falls outside [0, ntot) is not written). */
size_t dvae_encode_weights_floats(int y_dim);
int dvae_encode_batch(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                      const int64_t* frame_off_host, const float* weights, int y_dim, const float* eps, float* mu, float* log_var,
                      float* z, float* Z, int64_t ntot, const int64_t* col_host, const int64_t* tables_dev, void* stream);

/* ---- the encoder and the classifier at any covered size (csrc/mlp_generic.hip) ----
 * The two networks above for every geometry within the limits of dvae_mcem_plan_dims, exact float32 on v_mfma_f32_16x16x4_f32, one
 * launch each on `stream`, no host synchronisation, no atomics.  The entry points above stay as they are and stay the default for
 * 513-128-128; these serve the other sizes (and that one too, on request).
 *   encoder:    [x | y] (513 + y_dim) -> h1 (tanh) -> h2 (tanh) -> {mu z_dim, log_var z_dim}; y_dim 0..513, h1 / h2 1..512, z_dim 1..128
 *   classifier: x (513) -> h1 (relu) -> h2 (relu) -> y_dim logits (sigmoid); y_dim 1..513, h1 / h2 1..512, no batch norm
 * Dims outside the limits: the size queries return 0, every other call DVAE_E_BADARG with the limits named, nothing launched.
 * dvae_encode_generic_weights_floats / dvae_classify_generic_weights_floats: floats of the packed copy.
 * dvae_encode_generic_pack / dvae_classify_generic_pack: write the packed copy on `stream` from the state_dict tensors (device,
 *   float32, [out][in] with leading dimensions ld* >= their row length; biases packed).  Layout, with up16(v) the next multiple of 16:
 *   W1x [up16(h1)][528] | W1y [up16(h1)][up16(y_dim)] (encoder with labels only) | W2 [up16(h2)][up16(h1)] | W3 [rows][up16(h2)] |
 *   b1 [up16(h1)] | b2 [up16(h2)] | b3 [rows]; W3 / b3 are the heads, mu in rows 0 .. z_dim - 1 and log_var in rows up16(z_dim) ..
 *   up16(z_dim) + z_dim - 1 of 2 up16(z_dim) rows, or the output layer in up16(y_dim) rows.  Every matrix is stored in fragment
 *   order [row tile of 16][k block of 16][lane 0..63][4]: lane l holds row l & 15, inputs 16 b + 4 i + (l >> 4), i = 0..3.  Padding
 *   rows, inputs and biases are zero: a padded hidden unit is tanh 0 = relu 0 = 0 and has zero out-weights, a padded output row is
 *   computed and dropped.  The x block (columns 0..512 of W1) and the label block (columns 513..) are padded separately.
 * dvae_encode_generic_batch: dvae_encode_batch's arguments and contract with the dims after y_dim: inputs, tables, outputs, the
 *   table checks before anything is launched, z = mu + expf(0.5f log_var) eps with product and sum rounded separately, tanhf.  mu,
 *   log_var, z, eps are [N][z_dim], Z is [z_dim][ntot].
 * dvae_classify_generic_batch: dvae_classify_batch's arguments and contract with the dims after y_dim: soft = 1 / (1 + expf(-logit)),
 *   hard = soft > 0.5 ? 1 : 0 decided from the float32 soft that is stored; soft, hard, logits (or NULL) [N][y_dim].
 *   Summation: every pre-activation is ONE float32 chain from 0 with k ascending, four products per step as v_mfma_f32_16x16x4_f32
 *   adds them, over the 528 padded x inputs first, then the up16(y_dim) padded label inputs (as torch.cat([x, y], 1) lays them), the
 *   bias added after it.  A workgroup owns 16 frames; the order does not depend on the frame's place in its tile, on the tile's place
 *   in the grid or on the batch, so a frame gives the same bits alone, in any batch and from run to run (the bits of the entry
 *   points above, which add two products per step, are not promised; on the committed fixtures they came out equal).
 *   Never touched: rows outside [frame_off[0], frame_off[U]) or past N are neither read nor written; label rows are read in place at
 *   ldy; columns of Z outside the utterances' stay as they are, and a frame whose column by the device table falls outside
 *   [0, ntot) is not written. */
size_t dvae_encode_generic_weights_floats(int y_dim, int h1, int h2, int z_dim);
size_t dvae_classify_generic_weights_floats(int h1, int h2, int y_dim);
int dvae_encode_generic_pack(int y_dim, int h1, int h2, int z_dim, const float* W1, int64_t ld1, const float* b1, const float* W2,
                             int64_t ld2, const float* b2, const float* Wmu, int64_t ldmu, const float* bmu, const float* Wlv, int64_t ldlv,
                             const float* blv, float* weights, void* stream);
int dvae_classify_generic_pack(int h1, int h2, int y_dim, const float* W1, int64_t ld1, const float* b1, const float* W2, int64_t ld2,
                               const float* b2, const float* W3, int64_t ld3, const float* b3, float* weights, void* stream);
int dvae_encode_generic_batch(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                              const int64_t* frame_off_host, const float* weights, int y_dim, int h1, int h2, int z_dim, const float* eps,
                              float* mu, float* log_var, float* z, float* Z, int64_t ntot, const int64_t* col_host,
                              const int64_t* tables_dev, void* stream);
int dvae_classify_generic_batch(const void* src, int src_complex, int64_t ld, int64_t N, int U, const int64_t* frame_off_host,
                                const float* weights, int y_dim, int h1, int h2, float* soft, float* hard, float* logits, void* stream);
/* dvae_encode_generic_batch for an encoder trained on standardised input (the std_norm switch of the train scripts; dvae_train.h:
 * dvae_train_generic_plan_norm): norm_mean, norm_div are device tables of 513 floats, and the x block of layer 1 is
 * xn = fl32(fl32(p - norm_mean) / norm_div), p the power formed from a complex frame or read from a float row -- one IEEE subtraction
 * and one correctly rounded IEEE division, torch's (p - mean) / div bit for bit.  Labels are not normalised; the padded inputs 513..527 and
 * rows outside the table stay exact zeros.  Everything else, argument for argument, is dvae_encode_generic_batch. */
int dvae_encode_generic_batch_norm(const void* src, int src_complex, int64_t ld, const float* y, int64_t ldy, int64_t N, int U,
                                   const int64_t* frame_off_host, const float* weights, int y_dim, int h1, int h2, int z_dim,
                                   const float* eps, float* mu, float* log_var, float* z, float* Z, int64_t ntot, const int64_t* col_host,
                                   const int64_t* tables_dev, const float* norm_mean, const float* norm_div, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVAE_H */

// The host path of the three fused train steps of any covered size, written once: what dvae_train_generic_*, dvae_train_info_* and
// dvae_train_clf_* (include/dvae_train.h) do between their arguments and the launches of train_tables.hpp.  Each step describes itself
// in a struct S of its own file (train_generic.hip: MStep; train_info.hip: IStep; train_classifier.hip: CStep):
//   Plan, Layout                            the plan struct of the C ABI and the layout make_layout derives from it
//   NT, NG, ORDER[NG]                       its share of the tables (G_NT / G_NG entries) and the matrix order of the item table
//   COUNTS, WGRAD_Y                         the classifier: confusion counts beside the losses, and no label columns in a weight gradient
//   plan_layout(who, plan, L, setup)        the plan's checks and messages; setup: _init / _repack, which prepare a workspace
//   check_inputs(who, plan, ws, in)         what _grads / _eval refuse
//   launch_rows(plan, L, ws, in, fwd_only, s)
//   tensors(L, T), gemms(L, G)              the tables (every entry written or zeroed)
//   partials_bytes(L)                       what _init clears at o_partials
//   extend_apply_args(plan, L, a)           what the step adds to ApplyArgs
//   extend_table(plan, L, ws, counts4, g)   what it adds to GApplyArgs; g.finalize says whether the launch finalises
// The extern "C" functions stay in the step's file and forward here under their own name `who`, which every message starts with.  The
// order of the checks of an entry point, its return codes and its runtime calls are part of its behaviour (tests/test_train_host_cpu.py).
#pragma once
#include <math.h>
#include <vector>
#include "common.hpp"
#include "train_tables.hpp"

namespace dvae {
namespace tg {

using fused::ApplyArgs;

struct StepInputs { const float* x; int64_t ldx; const float* y; int64_t ldy; const float* eps; float loss_eps; };     // eps: the noise [B][z] (the classifier: null)
struct StepUpdate { float* params; float* m; float* v; int step; double lr, beta1, beta2, adam_eps, grad_scale; };
struct StepOutputs { float* losses; long long* counts4; };        // counts4: the classifier alone

// The plan's defaults (1, 0) leave every argument of every launch as it was without a weighted KL term.
template <class Plan>
bool kl_weighted(const Plan* plan) { return !((float)plan->kl_weight == 1.f && (float)plan->kl_floor == 0.f); }

// adam: the Adam scalars of step u.step; otherwise u gives the parameter pointers alone
template <class S>
ApplyArgs apply_args(const typename S::Plan* plan, const typename S::Layout& L, char* ws, const StepUpdate& u, bool adam, float* losses) {
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.p = u.params; a.m = u.m; a.v = u.v;
    a.slabs = (const float*)(ws + L.o_grads); a.slab_stride = L.n_params; a.nslabs = L.nslices;
    a.n_params = L.n_params;
    if (adam) {
        const double bc1 = 1.0 - pow(u.beta1, (double)u.step), bc2 = 1.0 - pow(u.beta2, (double)u.step);
        a.one_minus_b1 = (float)(1.0 - u.beta1); a.b2 = (float)u.beta2; a.one_minus_b2 = (float)(1.0 - u.beta2);
        a.step_size = (float)(u.lr / bc1); a.bc2_sqrt = (float)sqrt(bc2); a.eps = (float)u.adam_eps; a.gscale = (float)u.grad_scale;
    }
    a.partials = (const double*)(ws + L.o_partials); a.npartials = (int)L.rows_grid; a.B = L.B; a.losses3 = losses;
    a.accum = (double*)(uintptr_t)plan->loss_accum;
    S::extend_apply_args(plan, L, a);
    return a;
}

// the table of an apply or reduce launch.  adam: the optimizer step on every parameter; otherwise only the packed copies are rewritten
// (elements, a.p given) and / or the losses finalised
template <class S>
void fill_table(const typename S::Plan* plan, const typename S::Layout& L, const ApplyArgs& a, char* ws, bool adam, bool elements, bool finalize,
                long long* counts4, GApplyArgs& g) {
    memset(&g, 0, sizeof(g));
    g.a = a;
    if (!elements) g.a.n_params = 0;
    S::tensors(L, g.t);
    g.ws = (float*)ws; g.adam = adam ? 1 : 0; g.finalize = finalize ? 1 : 0;
    S::extend_table(plan, L, ws, counts4, g);
}

// (clip: the norm launch and the guarded apply kernel in place of the apply kernel)
template <class S>
int launch_apply(const typename S::Plan* plan, const typename S::Layout& L, const ApplyArgs& a, char* ws, bool adam, bool elements, bool finalize,
                 long long* counts4, hipStream_t s, const GClipHost* clip = nullptr) {
    GApplyArgs g;
    fill_table<S>(plan, L, a, ws, adam, elements, finalize, counts4, g);
    return clip ? launch_apply_clipped_table(g, *clip, s) : launch_apply_table(g, s);
}

// the slabs of a.slabs in slab order into flat (GReduceArgs); finalize: the micro-batch's loss scalars as the apply launch writes them
template <class S>
int launch_reduce(const typename S::Plan* plan, const typename S::Layout& L, const ApplyArgs& a, char* ws, bool finalize, long long* counts4,
                  float* flat, int accumulate, float weight, hipStream_t s) {
    GReduceArgs g;
    memset(&g, 0, sizeof(g));
    fill_table<S>(plan, L, a, ws, false, true, finalize, counts4, g.f);
    g.flat = flat; g.accumulate = accumulate; g.weight = weight;
    return launch_reduce_table(g, s);
}

template <class S>
int launch_wgrad(const typename S::Plan* plan, const typename S::Layout& L, char* ws, const StepInputs& in, hipStream_t s) {
    GWgradArgs g;
    memset(&g, 0, sizeof(g));
    g.x = in.x; g.ldx = in.ldx;
    if (S::WGRAD_Y) { g.y = in.y; g.ldy = in.ldy; }     // (the classifier: y_w 0 in every matrix)
    g.row_index = (const int64_t*)(uintptr_t)plan->row_index; g.row_count = plan->row_count;
    g.stash = (const float*)(ws + L.o_stash); g.slabs = (float*)(ws + L.o_grads); g.slab_stride = L.n_params;
    g.B = L.B; g.slice_frames = L.slice_frames; g.items = (const GItem*)(ws + L.o_items); g.S = L.S;
    S::gemms(L, g.gm);
    for (int t = 0; t < S::NT; ++t) g.toff[t] = L.toff[t];
    return launch_wgrad_table(g, L.n_items, s);
}

// every element of both packed copies from `params`, the padding zeroed first
template <class S>
int repack_copies(const typename S::Plan* plan, const typename S::Layout& L, const float* params, void* ws, hipStream_t s) {
    DVAE_HIP(hipMemsetAsync(ws, 0, (size_t)L.wpack_elems * 4, s));          // the padding of the packed copies
    StepUpdate u = {};
    u.params = (float*)params;
    return launch_apply<S>(plan, L, apply_args<S>(plan, L, (char*)ws, u, false, nullptr), (char*)ws, false, true, false, nullptr, s);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the entry points
template <class S>
int step_repack(const char* who, const typename S::Plan* plan, const float* params, void* ws, void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, true)) return rc;
    DVAE_CHECK_ARG(params && ws, "%s: null pointer", who);
    return repack_copies<S>(plan, L, params, ws, (hipStream_t)stream);
}

template <class S>
int step_init(const char* who, const typename S::Plan* plan, const float* params, void* ws, void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, true)) return rc;
    DVAE_CHECK_ARG(params && ws, "%s: null pointer", who);
    hipStream_t s = (hipStream_t)stream;
    GGemm gm[S::NG];
    S::gemms(L, gm);
    const std::vector<GItem> items = make_items(gm, S::ORDER, S::NG, L.nslices);
    DVAE_CHECK_ARG((int)items.size() == L.n_items, "%s: %d items for a table of %d", who, (int)items.size(), L.n_items);
    DVAE_HIP(hipMemcpyAsync((char*)ws + L.o_items, items.data(), items.size() * sizeof(GItem), hipMemcpyHostToDevice, s));
    DVAE_HIP(hipMemsetAsync((char*)ws + L.o_partials, 0, S::partials_bytes(L), s));
    DVAE_HIP(hipStreamSynchronize(s));                                      // the table leaves host memory that ends with this call
    return repack_copies<S>(plan, L, params, ws, s);
}

template <class S>
int step_grads(const char* who, const typename S::Plan* plan, void* ws, const StepInputs& in, void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, false)) return rc;
    if (int rc = S::check_inputs(who, plan, ws, in)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = S::launch_rows(plan, L, (char*)ws, in, false, s)) return rc;
    return launch_wgrad<S>(plan, L, (char*)ws, in, s);
}

template <class S>
int step_apply(const char* who, const typename S::Plan* plan, const StepUpdate& u, void* ws, const StepOutputs& out, void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, false)) return rc;
    DVAE_CHECK_ARG(u.params && u.m && u.v && ws && out.losses && (!S::COUNTS || out.counts4), "%s: null pointer", who);
    DVAE_CHECK_ARG(u.step >= 1, "%s: step %d (1-based)", who, u.step);
    const ApplyArgs a = apply_args<S>(plan, L, (char*)ws, u, true, out.losses);
    return launch_apply<S>(plan, L, a, (char*)ws, true, true, true, out.counts4, (hipStream_t)stream);
}

template <class S>
int step_reduce(const char* who, const typename S::Plan* plan, void* ws, float* flat, int accumulate, float weight, const StepOutputs& out,
                void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, false)) return rc;
    if (int rc = check_reduce_args(who, ws, flat, accumulate, weight)) return rc;
    DVAE_CHECK_ARG(out.losses && (!S::COUNTS || out.counts4), "%s: null pointer", who);
    const ApplyArgs a = apply_args<S>(plan, L, (char*)ws, StepUpdate{}, false, out.losses);
    return launch_reduce<S>(plan, L, a, (char*)ws, true, out.counts4, flat, accumulate, weight, (hipStream_t)stream);
}

// _apply_flat, and with `clip` _apply_flat_clipped (u.grad_scale is then clip->grad_scale)
template <class S>
int step_apply_flat(const char* who, const typename S::Plan* plan, const StepUpdate& u, void* ws, const float* flat, const GClipHost* clip,
                    void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, false)) return rc;
    if (int rc = check_apply_flat_args(who, u.params, u.m, u.v, ws, flat, u.step, u.lr, u.grad_scale)) return rc;
    if (clip)
        if (int rc = check_clip_args(who, flat, *clip)) return rc;
    ApplyArgs a = apply_args<S>(plan, L, (char*)ws, u, true, nullptr);
    a.slabs = flat; a.nslabs = 1;                       // the flat gradient is the one slab
    return launch_apply<S>(plan, L, a, (char*)ws, true, true, false, nullptr, (hipStream_t)stream, clip);
}

// grads, then apply at grad_scale 1: under the names of those two entry points, as their messages say
template <class S>
int step_step(const char* who, const char* who_grads, const char* who_apply, const typename S::Plan* plan, StepUpdate u, void* ws,
              const StepInputs& in, const StepOutputs& out, void* stream) {
    DVAE_CHECK_ARG(u.params && u.m && u.v && out.losses && (!S::COUNTS || out.counts4), "%s: null pointer", who);
    DVAE_CHECK_ARG(u.step >= 1, "%s: step %d (1-based)", who, u.step);
    if (int rc = step_grads<S>(who_grads, plan, ws, in, stream)) return rc;
    u.grad_scale = 1.0;
    return step_apply<S>(who_apply, plan, u, ws, out, stream);
}

template <class S>
int step_eval(const char* who, const typename S::Plan* plan, void* ws, const StepInputs& in, const StepOutputs& out, void* stream) {
    typename S::Layout L;
    if (int rc = S::plan_layout(who, plan, L, false)) return rc;
    if (int rc = S::check_inputs(who, plan, ws, in)) return rc;
    DVAE_CHECK_ARG(out.losses && (!S::COUNTS || out.counts4), "%s: null pointer", who);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = S::launch_rows(plan, L, (char*)ws, in, true, s)) return rc;
    const ApplyArgs a = apply_args<S>(plan, L, (char*)ws, StepUpdate{}, false, out.losses);
    return launch_apply<S>(plan, L, a, (char*)ws, false, false, true, out.counts4, s);
}

}  // namespace tg
}  // namespace dvae

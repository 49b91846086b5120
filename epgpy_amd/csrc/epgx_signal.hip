// epgx_signal.hip -- the entry points of include/epgx.h that read a signal, a dictionary or a Jacobian left in HBM.  Every entry
// is: the context's NULL guard, the argument checks (epgx_signal_check.h: plain C++, tested on the CPU), the early return for
// nothing to do, set_device, the kernel's argument struct, the launch.  Of the context an entry uses the stream, the number of
// compute units and the allocator (epgx_ctx.h).  (epgx_signal_reduce and epgx_signal_narrow: epgx_api.hip, next to their kernels.)
#include <algorithm>
#include <cmath>
#include <cstring>

#include "epgx_ctx.h"
#include "epgx_signal_check.h"
#include "epgx_stats.h"
#include "epgx_match.h"
#include "epgx_match32.h"
#include "epgx_compress.h"
#include "epgx_refine.h"
#include "epgx_nnls.h"

using namespace epgx;

static int no_ctx(const char *who) { return fail(EPGX_ERR_INVALID, "%s: NULL argument", who); }
static int launched(const char *who, hipError_t e) { return e == hipSuccess ? EPGX_OK : fail(EPGX_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

// ------------------------------------------------------------------------------ Cramer-Rao bounds (epgx_stats.hip)
static void fill_crlb(CrlbArgs &a, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrec, int32_t nparam,
                      const int32_t *rows, int64_t vox0, int64_t nvox, const double *weights, double sigma2, int32_t flags, void *out) {
    memset(&a, 0, sizeof(a));
    for (int c = 0; c < nparam; ++c) a.rows[c] = rows[c], a.w[c] = weights ? weights[c] : 1.0;
    a.signal = (const d2 *)signal, a.record_stride = record_stride, a.row_stride = row_stride;
    a.nrec = nrec, a.vox0 = vox0, a.nvox = nvox;
    a.inv_sigma2 = 1.0 / sigma2;
    a.flags = flags;
    crlb_slices(nrec, &a.slices, &a.slice_len);
    a.out = (double *)out;
}

extern "C" int epgx_signal_crlb(epgx_ctx *ctx, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow,
                                int32_t nrec, int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox,
                                const double *weights, double sigma2, int32_t flags, void *out) {
    const char *who = "epgx_signal_crlb";
    if (!ctx) return no_ctx(who);
    if (int rc = crlb_check(who, signal, record_stride, row_stride, nrow, nrec, nparam, rows, vox0, nvox, weights, sigma2, flags, out)) return rc;
    if (nvox == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    CrlbArgs a;
    fill_crlb(a, signal, record_stride, row_stride, nrec, nparam, rows, vox0, nvox, weights, sigma2, flags, out);
    return launched(who, epgx_launch_crlb(ctx->stream, nparam, a));
}

extern "C" int epgx_signal_crlb_grad(epgx_ctx *ctx, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow,
                                     int32_t nrec, int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox,
                                     const void *hess, int64_t hess_len, int32_t nx, const int64_t *offsets,
                                     const int64_t *record_strides, const double *weights, double sigma2, int32_t flags,
                                     void *out_cost, void *out_grad) {
    const char *who = "epgx_signal_crlb_grad";
    if (!ctx) return no_ctx(who);
    if (int rc = crlb_grad_check(who, signal, record_stride, row_stride, nrow, nrec, nparam, rows, vox0, nvox, hess, hess_len, nx, offsets,
                                 record_strides, weights, sigma2, flags, out_cost, out_grad))
        return rc;
    if (nvox == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    CrlbArgs a;
    fill_crlb(a, signal, record_stride, row_stride, nrec, nparam, rows, vox0, nvox, weights, sigma2, flags, out_cost);
    for (int32_t x0 = 0; x0 < nx; x0 += CRLB_GRAD_XB) {      // one launch per chunk of design variables
        CrlbGradArgs h;
        memset(&h, 0, sizeof(h));
        h.hess = (const d2 *)hess;
        h.nx = std::min<int32_t>(CRLB_GRAD_XB, nx - x0);
        h.write_cost = x0 == 0;
        h.grad = (double *)out_grad + (int64_t)x0 * nvox;
        for (int x = 0; x < CRLB_GRAD_XB; ++x)
            for (int c = 0; c < CRLB_MAX_P; ++c) {
                const bool used = x < h.nx && c < nparam;
                h.off[x][c] = used ? offsets[(int64_t)c * nx + x0 + x] : -1;
                h.stride[x][c] = used ? record_strides[(int64_t)c * nx + x0 + x] : 0;
            }
        if (int rc = launched(who, epgx_launch_crlb_grad(ctx->stream, nparam, a, h))) return rc;
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ dictionary matching (epgx_match.hip, epgx_match32.hip)
extern "C" int epgx_signal_norms(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, void *out) {
    const char *who = "epgx_signal_norms";
    if (!ctx) return no_ctx(who);
    if (int rc = norms_check(who, dict, row_stride, nrec, natoms, out, 16)) return rc;
    if (int rc = set_device(ctx)) return rc;
    return launched(who, epgx_launch_norms(ctx->stream, dict, row_stride, nrec, natoms, (double *)out));
}

extern "C" int epgx_signal_norms_c64(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, void *out) {
    const char *who = "epgx_signal_norms_c64";
    if (!ctx) return no_ctx(who);
    if (int rc = norms_check(who, dict, row_stride, nrec, natoms, out, 8)) return rc;
    if (int rc = set_device(ctx)) return rc;
    return launched(who, epgx_launch_norms32(ctx->stream, dict, row_stride, nrec, natoms, (double *)out));
}

// one body for both precisions: Elem = d2 with MatchArgs / MatchMergeArgs, f2 with Match32Args / Match32MergeArgs
template <class Args, class MergeArgs, hipError_t (*Launch)(hipStream_t, const Args &), hipError_t (*LaunchMerge)(hipStream_t, const MergeArgs &),
          class Elem, int CHUNK>
static int signal_match(const char *who, epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms,
                        const void *sig, int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit, void *out_index,
                        void *out_scale, void *out_score) {
    if (!ctx) return no_ctx(who);
    MatchPlan plan;
    if (int rc = match_check(who, dict, dict_row_stride, norms, natoms, sig, sig_row_stride, nrec, nmeas, nsplit, out_index, out_scale,
                             out_score, ctx->prop.multiProcessorCount, (int)sizeof(Elem), CHUNK, &plan))
        return rc;
    if (nmeas == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    void *part = nullptr;
    hipError_t e = dev_alloc(ctx, &part, sizeof(MatchPartial) * (size_t)plan.scratch_len);
    if (e != hipSuccess)
        return fail(EPGX_ERR_NOMEM, "%s: scratch for %d splits of %lld voxels: %s", who, plan.nsplit, (long long)nmeas, hipGetErrorString(e));
    Args a;
    memset(&a, 0, sizeof(a));
    a.dict = (const Elem *)dict, a.dict_stride = dict_row_stride;
    a.norms = (const double *)norms, a.natoms = natoms;
    a.sig = (const Elem *)sig, a.sig_stride = sig_row_stride;
    a.nmeas = nmeas, a.nvt = plan.nvt;
    a.nrec = nrec, a.nsplit = plan.nsplit;
    a.chunk = plan.chunk, a.nchunk = plan.nchunk;
    a.part = (MatchPartial *)part;
    e = Launch(ctx->stream, a);
    if (e == hipSuccess) {
        MergeArgs g;
        memset(&g, 0, sizeof(g));
        g.part = a.part, g.norms = a.norms;
        g.sig = a.sig, g.sig_stride = sig_row_stride;
        g.nmeas = nmeas, g.nrec = nrec, g.nsplit = plan.nsplit;
        g.index = (int64_t *)out_index, g.scale = (d2 *)out_scale, g.score = (double *)out_score;
        e = LaunchMerge(ctx->stream, g);
    }
    dev_free(ctx, part);      // (stream-ordered: the block is recycled behind the kernels that use it)
    return launched(who, e);
}

extern "C" int epgx_signal_match(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms,
                                 const void *sig, int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit,
                                 void *out_index, void *out_scale, void *out_score) {
    return signal_match<MatchArgs, MatchMergeArgs, epgx_launch_match, epgx_launch_match_merge, d2, MATCH_CHUNK>(
        "epgx_signal_match", ctx, dict, dict_row_stride, norms, natoms, sig, sig_row_stride, nrec, nmeas, nsplit, out_index, out_scale, out_score);
}

extern "C" int epgx_signal_match_c64(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms,
                                     const void *sig, int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit,
                                     void *out_index, void *out_scale, void *out_score) {
    return signal_match<Match32Args, Match32MergeArgs, epgx_launch_match32, epgx_launch_match32_merge, f2, MATCH32_CHUNK>(
        "epgx_signal_match_c64", ctx, dict, dict_row_stride, norms, natoms, sig, sig_row_stride, nrec, nmeas, nsplit, out_index, out_scale, out_score);
}

// ------------------------------------------------------------------------------ Gauss-Newton refinement (epgx_refine.hip)
extern "C" int epgx_signal_refine(epgx_ctx *ctx, const void *jac, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                                  int32_t nparam, const int32_t *rows, int64_t natoms, const void *sig, int64_t sig_row_stride,
                                  int64_t nmeas, const void *index, const double *limit, double rcond, void *out_delta, void *out_scale,
                                  void *out_score) {
    const char *who = "epgx_signal_refine";
    if (!ctx) return no_ctx(who);
    if (int rc = refine_check(who, jac, record_stride, row_stride, nrow, nrec, nparam, rows, natoms, sig, sig_row_stride, nmeas, index, limit,
                              rcond, out_delta, out_scale, out_score))
        return rc;
    if (nmeas == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    RefineArgs a;
    memset(&a, 0, sizeof(a));
    for (int c = 0; c < nparam; ++c) a.rows[c] = rows[c], a.limit[c] = limit ? limit[c] : (double)INFINITY;
    a.jac = (const d2 *)jac, a.record_stride = record_stride, a.row_stride = row_stride;
    a.nrec = nrec, a.natoms = natoms;
    a.sig = (const d2 *)sig, a.sig_stride = sig_row_stride, a.nmeas = nmeas;
    a.index = (const int64_t *)index;
    a.rcond = rcond;
    refine_slices(nrec, &a.slices, &a.slice_len);
    a.delta = (double *)out_delta, a.scale = (d2 *)out_scale, a.score = (double *)out_score;
    return launched(who, epgx_launch_refine(ctx->stream, nparam, a));
}

// ------------------------------------------------------------------------------ non-negative mixtures (epgx_nnls.hip)
extern "C" int epgx_signal_component_gram(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp,
                                          int64_t axis_stride, int64_t nouter, int64_t ninner, void *out_gram, void *out_mask) {
    const char *who = "epgx_signal_component_gram";
    if (!ctx) return no_ctx(who);
    if (int rc = component_gram_check(who, dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner, out_gram, out_mask)) return rc;
    if (int rc = set_device(ctx)) return rc;
    ComponentGramArgs a;
    memset(&a, 0, sizeof(a));
    a.c = ComponentArgs{(const d2 *)dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner};
    a.gram = (double *)out_gram, a.mask = (unsigned long long *)out_mask;
    return launched(who, epgx_launch_component_gram(ctx->stream, a));
}

// the NnlsArgs of epgx_signal_nnls and epgx_signal_nnls_chi2 from arguments that nnls_check has passed
static void fill_nnls(NnlsArgs &a, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride, int64_t nouter,
                      int64_t ninner, const void *gram, const void *mask, const void *sig, int64_t sig_row_stride, int64_t nmeas, double reg,
                      double tol, const void *group, void *out_weights, void *out_group, void *out_residual, void *out_status) {
    memset(&a, 0, sizeof(a));
    a.c = ComponentArgs{(const d2 *)dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner};
    a.gram = (const double *)gram, a.mask = (const unsigned long long *)mask;
    a.sig = (const d2 *)sig, a.sig_stride = sig_row_stride, a.nmeas = nmeas;
    a.reg = reg, a.tol = tol;
    a.group = (const int64_t *)group;
    a.weights = (double *)out_weights, a.out_group = (int64_t *)out_group;
    a.residual = (double *)out_residual, a.status = (int32_t *)out_status;
}

// (the context's NULL guard of the next two is in nnls_check, where the helper they shared had it)
extern "C" int epgx_signal_nnls(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                                int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig,
                                int64_t sig_row_stride, int64_t nmeas, double reg, double tol, const void *group, void *out_weights,
                                void *out_group, void *out_residual, void *out_status) {
    const char *who = "epgx_signal_nnls";
    if (int rc = nnls_check(who, ctx, dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner, gram, mask, sig, sig_row_stride, nmeas, reg,
                            tol, group, out_weights, out_group, out_residual, out_status))
        return rc;
    if (nmeas == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    NnlsArgs a;
    fill_nnls(a, dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner, gram, mask, sig, sig_row_stride, nmeas, reg, tol, group,
              out_weights, out_group, out_residual, out_status);
    return launched(who, epgx_launch_nnls(ctx->stream, a));
}

extern "C" int epgx_signal_nnls_chi2(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                                     int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig,
                                     int64_t sig_row_stride, int64_t nmeas, double reg, double tol, const void *group, double chi2,
                                     double chi2_rtol, int32_t max_evals, void *out_weights, void *out_group, void *out_residual,
                                     void *out_status, void *out_mu, void *out_chi2, void *out_evals) {
    const char *who = "epgx_signal_nnls_chi2";
    if (int rc = nnls_chi2_outputs_check(who, out_mu, out_chi2, out_evals)) return rc;
    if (int rc = nnls_check(who, ctx, dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner, gram, mask, sig, sig_row_stride, nmeas, reg,
                            tol, group, out_weights, out_group, out_residual, out_status))
        return rc;
    if (int rc = nnls_chi2_search_check(who, reg, chi2, chi2_rtol, max_evals)) return rc;
    if (nmeas == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    NnlsChi2Args a;
    memset(&a, 0, sizeof(a));
    fill_nnls(a.n, dict, row_stride, nrec, ncomp, axis_stride, nouter, ninner, gram, mask, sig, sig_row_stride, nmeas, reg, tol, group,
              out_weights, out_group, out_residual, out_status);
    a.chi2 = chi2, a.rtol = chi2_rtol, a.max_evals = max_evals;
    a.mu = (double *)out_mu, a.ratio = (double *)out_chi2, a.evals = (int32_t *)out_evals;
    if (!group) {      // the group search first; its out_group stays on the device and is what the second launch reads
        if (int rc = launched(who, epgx_launch_nnls(ctx->stream, a.n))) return rc;
        a.n.group = a.n.out_group;
    }
    return launched(who, epgx_launch_nnls_chi2(ctx->stream, a));
}

// ------------------------------------------------------------------------------ dictionary compression (epgx_compress.hip)
extern "C" int epgx_signal_gram(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int32_t nrec, int64_t natoms,
                                int32_t nsplit, void *out) {
    const char *who = "epgx_signal_gram";
    if (!ctx) return no_ctx(who);
    GramPlan plan;
    if (int rc = gram_check(who, dict, dict_row_stride, norms, nrec, natoms, nsplit, out, &plan)) return rc;
    if (int rc = set_device(ctx)) return rc;
    void *part = nullptr;
    hipError_t e = dev_alloc(ctx, &part, sizeof(d2) * (size_t)plan.scratch_len);
    if (e != hipSuccess)
        return fail(EPGX_ERR_NOMEM, "%s: scratch for %d partial Gram matrices of %d x %d: %s", who, plan.nsplit, nrec, nrec, hipGetErrorString(e));
    GramArgs a;
    memset(&a, 0, sizeof(a));
    a.dict = (const d2 *)dict, a.dict_stride = dict_row_stride;
    a.norms = (const double *)norms, a.natoms = natoms;
    a.nrec = nrec, a.nsplit = plan.nsplit;
    a.nblock = plan.nblock, a.npair = plan.npair;
    a.part = (d2 *)part;
    e = epgx_launch_gram(ctx->stream, a);
    if (e == hipSuccess) {
        GramReduceArgs g;
        memset(&g, 0, sizeof(g));
        g.part = a.part, g.nrec = nrec, g.nsplit = plan.nsplit;
        g.out = (d2 *)out;
        e = epgx_launch_gram_reduce(ctx->stream, g);
    }
    dev_free(ctx, part);      // (stream-ordered: the block is recycled behind the kernels that use it)
    return launched(who, e);
}

extern "C" int epgx_signal_project(epgx_ctx *ctx, const void *basis, int32_t rank, const void *src, int64_t src_row_stride, int32_t nrec,
                                   int64_t ncol, void *out, int64_t out_row_stride) {
    const char *who = "epgx_signal_project";
    if (!ctx) return no_ctx(who);
    if (int rc = project_check(who, basis, rank, src, src_row_stride, nrec, ncol, out, out_row_stride)) return rc;
    if (ncol == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    ProjectArgs a;
    memset(&a, 0, sizeof(a));
    a.basis = (const d2 *)basis;
    a.src = (const d2 *)src, a.src_stride = src_row_stride, a.ncol = ncol;
    a.out = (d2 *)out, a.out_stride = out_row_stride;
    a.nrec = nrec, a.rank = rank;
    return launched(who, epgx_launch_project(ctx->stream, a));
}

// epgx_signal_check.cpp -- argument checks of the signal consumers (epgx_signal_check.h).  Plain C++17, no HIP.
#include "epgx_signal_check.h"

#include <algorithm>
#include <cmath>

namespace epgx {

static bool off(const void *p, uintptr_t align) { return ((uintptr_t)p & (align - 1)) != 0; }      // p is not aligned to `align` bytes

bool records_extent_ok(int64_t rows, int64_t row_stride, int64_t cols, int64_t elem_bytes) {
    int64_t span;
    return row_stride >= cols && !__builtin_mul_overflow(rows - 1, row_stride, &span) && !__builtin_add_overflow(span, cols, &span) &&
           span <= INT64_MAX / elem_bytes;
}

int jacobian_block_check(const char *who, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec) {
    if (record_stride / nrow < row_stride)
        return fail(EPGX_ERR_INVALID, "%s: record_stride = %lld holds fewer than nrow = %d rows of %lld", who, (long long)record_stride, nrow,
                    (long long)row_stride);
    int64_t span, last;
    if (__builtin_mul_overflow((int64_t)(nrec - 1), record_stride, &span) || __builtin_mul_overflow((int64_t)nrow, row_stride, &last) ||
        __builtin_add_overflow(span, last, &span) || span > INT64_MAX / 16)
        return fail(EPGX_ERR_INVALID, "%s: nrec = %d records of record_stride = %lld elements overflow the address range", who, nrec,
                    (long long)record_stride);
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ Cramer-Rao bounds (epgx_stats.hip)
// the Jacobian block, weights, sigma2 and flags of epgx_signal_crlb / epgx_signal_crlb_grad
static int crlb_jacobian_check(const char *who, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                               int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox, const double *weights, double sigma2,
                               int32_t flags, int32_t known_flags) {
    if (off(signal, 16)) return fail(EPGX_ERR_INVALID, "%s: signal must be aligned to 16 bytes", who);
    if (nparam < 1 || nparam > CRLB_MAX_P) return fail(EPGX_ERR_INVALID, "%s: nparam = %d not in [1, %d]", who, nparam, CRLB_MAX_P);
    if (nrec < 1 || nrow < 1) return fail(EPGX_ERR_INVALID, "%s: nrec = %d, nrow = %d: both must be >= 1", who, nrec, nrow);
    if (vox0 < 0 || nvox < 0 || row_stride < 1 || nvox > row_stride - vox0)
        return fail(EPGX_ERR_INVALID, "%s: voxels [%lld, %lld + %lld) outside a row of %lld", who, (long long)vox0, (long long)vox0,
                    (long long)nvox, (long long)row_stride);
    if (int rc = jacobian_block_check(who, record_stride, row_stride, nrow, nrec)) return rc;
    if (flags & ~known_flags) return fail(EPGX_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
    if (!(sigma2 > 0.0) || !std::isfinite(sigma2)) return fail(EPGX_ERR_INVALID, "%s: sigma2 = %g is not a positive finite number", who, sigma2);
    for (int c = 0; c < nparam; ++c) {
        if (rows[c] < 0 || rows[c] >= nrow) return fail(EPGX_ERR_INVALID, "%s: rows[%d] = %d not in [0, nrow = %d)", who, c, rows[c], nrow);
        if (weights && !std::isfinite(weights[c])) return fail(EPGX_ERR_INVALID, "%s: weights[%d] is not finite", who, c);
    }
    if (nvox / 64 >= 0x7fffffff) return fail(EPGX_ERR_INVALID, "%s: %lld voxels in one call", who, (long long)nvox);
    return EPGX_OK;
}

int crlb_check(const char *who, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec, int32_t nparam,
               const int32_t *rows, int64_t vox0, int64_t nvox, const double *weights, double sigma2, int32_t flags, const void *out) {
    if (!signal || !rows || !out) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(out, 8)) return fail(EPGX_ERR_INVALID, "%s: out must be aligned to 8 bytes", who);
    return crlb_jacobian_check(who, signal, record_stride, row_stride, nrow, nrec, nparam, rows, vox0, nvox, weights, sigma2, flags,
                               EPGX_CRLB_SPLIT | EPGX_CRLB_LOG10);
}

int crlb_grad_check(const char *who, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                    int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox, const void *hess, int64_t hess_len, int32_t nx,
                    const int64_t *offsets, const int64_t *record_strides, const double *weights, double sigma2, int32_t flags,
                    const void *out_cost, const void *out_grad) {
    if (!signal || !rows || !hess || !offsets || !record_strides || !out_cost || !out_grad)
        return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(hess, 16) || off(out_cost, 8) || off(out_grad, 8))
        return fail(EPGX_ERR_INVALID, "%s: hess must be aligned to 16 bytes, out_cost and out_grad to 8", who);
    if (int rc = crlb_jacobian_check(who, signal, record_stride, row_stride, nrow, nrec, nparam, rows, vox0, nvox, weights, sigma2, flags,
                                     EPGX_CRLB_LOG10))
        return rc;
    if (nx < 1) return fail(EPGX_ERR_INVALID, "%s: nx = %d must be >= 1", who, nx);
    if (hess_len < 0 || hess_len > INT64_MAX / 16) return fail(EPGX_ERR_INVALID, "%s: hess_len = %lld", who, (long long)hess_len);
    int64_t grad_len;
    if (__builtin_mul_overflow((int64_t)nx, nvox, &grad_len) || grad_len > INT64_MAX / 8)
        return fail(EPGX_ERR_INVALID, "%s: nx = %d maps of %lld voxels overflow the address range", who, nx, (long long)nvox);
    // every entry of H that is read lies inside [hess, hess + hess_len): the kernel reads elements
    // offset + r * stride + vox0 + j,  r < nrec, j < nvox
    for (int64_t i = 0; i < (int64_t)nparam * nx; ++i) {
        const int64_t first = offsets[i], step = record_strides[i];
        if (first < 0) continue;
        int64_t end;
        if (step < 0 || (nrec > 1 && step < nvox) || __builtin_mul_overflow((int64_t)(nrec - 1), step, &end) ||
            __builtin_add_overflow(end, first, &end) || __builtin_add_overflow(end, vox0, &end) || __builtin_add_overflow(end, nvox, &end) ||
            end > hess_len)
            return fail(EPGX_ERR_INVALID, "%s: entry (%lld, %lld) of H: offset = %lld, record stride = %lld, %d records of voxels [%lld, %lld + %lld) "
                        "do not lie inside hess_len = %lld elements (or the records overlap)", who, (long long)(i / nx), (long long)(i % nx),
                        (long long)first, (long long)step, nrec, (long long)vox0, (long long)vox0, (long long)nvox, (long long)hess_len);
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ dictionary matching (epgx_match.hip, epgx_match32.hip)
int norms_check(const char *who, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, const void *out, int elem_bytes) {
    if (!dict || !out) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(dict, elem_bytes) || off(out, 8))
        return fail(EPGX_ERR_INVALID, elem_bytes == 16 ? "%s: dict must be aligned to 16 bytes, out to 8" : "%s: dict and out must be aligned to 8 bytes", who);
    if (nrec < 1 || natoms < 1) return fail(EPGX_ERR_INVALID, "%s: nrec = %d, natoms = %lld: both must be >= 1", who, nrec, (long long)natoms);
    if (!records_extent_ok(nrec, row_stride, natoms, elem_bytes) || natoms / 256 >= 0x7fffffff)
        return fail(EPGX_ERR_INVALID, "%s: %d records of row_stride = %lld do not hold %lld atoms each (or overflow the address range)", who,
                    nrec, (long long)row_stride, (long long)natoms);
    return EPGX_OK;
}

int match_check(const char *who, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms, const void *sig,
                int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit, const void *out_index, const void *out_scale,
                const void *out_score, int cu_count, int elem_bytes, int chunk_max, MatchPlan *plan) {
    *plan = MatchPlan{};
    if (!dict || !norms || !sig || !out_index || !out_scale || !out_score) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(dict, elem_bytes) || off(sig, elem_bytes) || off(out_scale, 16) || off(norms, 8) || off(out_index, 8) || off(out_score, 8))
        return fail(EPGX_ERR_INVALID, elem_bytes == 16 ? "%s: dict, sig and out_scale must be aligned to 16 bytes, norms, out_index and out_score to 8"
                                                       : "%s: out_scale must be aligned to 16 bytes, dict, sig, norms, out_index and out_score to 8", who);
    if (nrec < 1 || natoms < 1 || nmeas < 0)
        return fail(EPGX_ERR_INVALID, "%s: nrec = %d, natoms = %lld (both >= 1), nmeas = %lld (>= 0)", who, nrec, (long long)natoms, (long long)nmeas);
    if (nsplit < 0 || nsplit > natoms) return fail(EPGX_ERR_INVALID, "%s: nsplit = %d not in [0, natoms = %lld]", who, nsplit, (long long)natoms);
    if (!records_extent_ok(nrec, dict_row_stride, natoms, elem_bytes))
        return fail(EPGX_ERR_INVALID, "%s: %d records of dict_row_stride = %lld do not hold %lld atoms each (or overflow the address range)", who,
                    nrec, (long long)dict_row_stride, (long long)natoms);
    if (!records_extent_ok(nrec, sig_row_stride, nmeas, elem_bytes))
        return fail(EPGX_ERR_INVALID, "%s: %d records of sig_row_stride = %lld do not hold %lld voxels each (or overflow the address range)", who,
                    nrec, (long long)sig_row_stride, (long long)nmeas);
    if (nmeas == 0) return EPGX_OK;
    plan->nvt = (nmeas + MATCH_VOX - 1) / MATCH_VOX;
    if (nsplit == 0) {
        const int64_t want = 4 * (int64_t)std::max(cu_count, 1);
        const int64_t most = std::max<int64_t>(natoms / (MATCH_WAVES * MATCH_TILE), 1);
        nsplit = (int32_t)std::min<int64_t>(std::min<int64_t>((want + plan->nvt - 1) / plan->nvt, most), 1 << 16);
    }
    if (plan->nvt > (int64_t)0x7fffffff / nsplit || __builtin_mul_overflow((int64_t)nsplit, nmeas, &plan->scratch_len) ||
        plan->scratch_len > INT64_MAX / (int64_t)sizeof(MatchPartial))
        return fail(EPGX_ERR_INVALID, "%s: nsplit = %d splits of %lld voxels in one call", who, nsplit, (long long)nmeas);
    plan->nsplit = nsplit;
    plan->chunk = (int32_t)std::min<int64_t>(((int64_t)nrec + MATCH_STEP - 1) / MATCH_STEP * MATCH_STEP, chunk_max);      // (int64: nrec up to 2^31 - 1)
    plan->nchunk = (int32_t)(((int64_t)nrec + plan->chunk - 1) / plan->chunk);
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ Gauss-Newton refinement (epgx_refine.hip)
int refine_check(const char *who, const void *jac, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec, int32_t nparam,
                 const int32_t *rows, int64_t natoms, const void *sig, int64_t sig_row_stride, int64_t nmeas, const void *index,
                 const double *limit, double rcond, const void *out_delta, const void *out_scale, const void *out_score) {
    if (!jac || !rows || !sig || !index || !out_delta || !out_scale || !out_score) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(jac, 16) || off(sig, 16) || off(out_scale, 16) || off(index, 8) || off(out_delta, 8) || off(out_score, 8))
        return fail(EPGX_ERR_INVALID, "%s: jac, sig and out_scale must be aligned to 16 bytes, index, out_delta and out_score to 8", who);
    if (nparam < 1 || nparam > REFINE_MAX_P) return fail(EPGX_ERR_INVALID, "%s: nparam = %d not in [1, %d]", who, nparam, REFINE_MAX_P);
    if (nrec < 1 || nrow < 1) return fail(EPGX_ERR_INVALID, "%s: nrec = %d, nrow = %d: both must be >= 1", who, nrec, nrow);
    if (natoms < 1 || nmeas < 0) return fail(EPGX_ERR_INVALID, "%s: natoms = %lld (>= 1), nmeas = %lld (>= 0)", who, (long long)natoms, (long long)nmeas);
    if (row_stride < 1 || natoms > row_stride)
        return fail(EPGX_ERR_INVALID, "%s: %lld atoms outside a row of %lld", who, (long long)natoms, (long long)row_stride);
    if (int rc = jacobian_block_check(who, record_stride, row_stride, nrow, nrec)) return rc;
    if (!records_extent_ok(nrec, sig_row_stride, nmeas, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d records of sig_row_stride = %lld do not hold %lld voxels each (or overflow the address range)", who,
                    nrec, (long long)sig_row_stride, (long long)nmeas);
    if (nmeas / 64 >= 0x7fffffff) return fail(EPGX_ERR_INVALID, "%s: %lld voxels in one call", who, (long long)nmeas);
    if (!(rcond >= 0.0 && rcond < 1.0)) return fail(EPGX_ERR_INVALID, "%s: rcond = %g not in [0, 1)", who, rcond);
    for (int c = 0; c < nparam; ++c) {
        if (rows[c] < 1 || rows[c] >= nrow)
            return fail(EPGX_ERR_INVALID, "%s: rows[%d] = %d not in [1, nrow = %d) (row 0 is the state)", who, c, rows[c], nrow);
        for (int k = 0; k < c; ++k)
            if (rows[k] == rows[c]) return fail(EPGX_ERR_INVALID, "%s: rows[%d] = rows[%d] = %d: a repeated row", who, k, c, rows[c]);
        if (limit && !(limit[c] > 0.0)) return fail(EPGX_ERR_INVALID, "%s: limit[%d] = %g is not positive", who, c, limit[c]);
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ non-negative mixtures (epgx_nnls.hip)
// the dictionary read as D[t, a, g] (ComponentArgs): the checks all three entries share
static int component_check(const char *who, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride, int64_t nouter, int64_t ninner) {
    if (ncomp < 1 || ncomp > NNLS_MAX_A) return fail(EPGX_ERR_INVALID, "%s: ncomp = %d not in [1, %d]", who, ncomp, NNLS_MAX_A);
    if (nrec < 1) return fail(EPGX_ERR_INVALID, "%s: nrec = %d must be >= 1", who, nrec);
    if (nouter < 1 || ninner < 1)
        return fail(EPGX_ERR_INVALID, "%s: nouter = %lld, ninner = %lld: both must be >= 1", who, (long long)nouter, (long long)ninner);
    if (axis_stride < ninner)
        return fail(EPGX_ERR_INVALID, "%s: axis_stride = %lld below ninner = %lld", who, (long long)axis_stride, (long long)ninner);
    int64_t groups, cols;      // cols: one past the last column an atom lies at
    if (__builtin_mul_overflow(nouter, ninner, &groups) || groups > 0x7fffffff)
        return fail(EPGX_ERR_INVALID, "%s: nouter = %lld times ninner = %lld groups in one call", who, (long long)nouter, (long long)ninner);
    if (__builtin_mul_overflow(nouter, (int64_t)ncomp, &cols) || __builtin_mul_overflow(cols - 1, axis_stride, &cols) ||
        __builtin_add_overflow(cols, ninner, &cols) || !records_extent_ok(nrec, row_stride, cols, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d records of row_stride = %lld do not hold %lld x %d atoms of stride %lld (or overflow the address range)",
                    who, nrec, (long long)row_stride, (long long)nouter, ncomp, (long long)axis_stride);
    return EPGX_OK;
}

int component_gram_check(const char *who, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                         int64_t nouter, int64_t ninner, const void *out_gram, const void *out_mask) {
    if (!dict || !out_gram || !out_mask) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(dict, 16) || off(out_gram, 8) || off(out_mask, 8))
        return fail(EPGX_ERR_INVALID, "%s: dict must be aligned to 16 bytes, out_gram and out_mask to 8", who);
    return component_check(who, row_stride, nrec, ncomp, axis_stride, nouter, ninner);
}

int nnls_check(const char *who, const void *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
               int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig, int64_t sig_row_stride, int64_t nmeas,
               double reg, double tol, const void *group, const void *out_weights, const void *out_group, const void *out_residual,
               const void *out_status) {
    if (!ctx || !dict || !gram || !mask || !sig || !out_weights || !out_group || !out_residual || !out_status)
        return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(dict, 16) || off(sig, 16) || off(gram, 8) || off(mask, 8) || off(group, 8) || off(out_weights, 8) || off(out_group, 8) ||
        off(out_residual, 8) || off(out_status, 4))
        return fail(EPGX_ERR_INVALID, "%s: dict and sig must be aligned to 16 bytes, out_status to 4, the others to 8", who);
    if (int rc = component_check(who, row_stride, nrec, ncomp, axis_stride, nouter, ninner)) return rc;
    if (nmeas < 0) return fail(EPGX_ERR_INVALID, "%s: nmeas = %lld must be >= 0", who, (long long)nmeas);
    if (!records_extent_ok(nrec, sig_row_stride, nmeas, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d records of sig_row_stride = %lld do not hold %lld voxels each (or overflow the address range)", who,
                    nrec, (long long)sig_row_stride, (long long)nmeas);
    if (nmeas >= 0x7fffffff) return fail(EPGX_ERR_INVALID, "%s: %lld voxels in one call", who, (long long)nmeas);
    if (!(reg >= 0.0 && reg < (double)INFINITY)) return fail(EPGX_ERR_INVALID, "%s: reg = %g is not a finite number >= 0", who, reg);
    if (!(tol >= 0.0 && tol < (double)INFINITY)) return fail(EPGX_ERR_INVALID, "%s: tol = %g is not a finite number >= 0", who, tol);
    return EPGX_OK;
}

int nnls_chi2_outputs_check(const char *who, const void *out_mu, const void *out_chi2, const void *out_evals) {
    if (!out_mu || !out_chi2 || !out_evals) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(out_mu, 8) || off(out_chi2, 8) || off(out_evals, 4))
        return fail(EPGX_ERR_INVALID, "%s: out_mu and out_chi2 must be aligned to 8 bytes, out_evals to 4", who);
    return EPGX_OK;
}

int nnls_chi2_search_check(const char *who, double reg, double chi2, double chi2_rtol, int32_t max_evals) {
    if (!(reg > 0.0)) return fail(EPGX_ERR_INVALID, "%s: reg = %g must be > 0: the bracket grows from mu_0 = reg * mean H_aa", who, reg);
    if (!(chi2 > 1.0 && chi2 < (double)INFINITY)) return fail(EPGX_ERR_INVALID, "%s: chi2 = %g is not a finite number > 1", who, chi2);
    if (!(chi2_rtol > 0.0 && chi2_rtol < 1.0)) return fail(EPGX_ERR_INVALID, "%s: chi2_rtol = %g not in (0, 1)", who, chi2_rtol);
    if (max_evals < 0 || max_evals > NNLS_CHI2_EVALS)
        return fail(EPGX_ERR_INVALID, "%s: max_evals = %d not in [0, %d]", who, max_evals, NNLS_CHI2_EVALS);
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ dictionary compression (epgx_compress.hip)
int gram_check(const char *who, const void *dict, int64_t dict_row_stride, const void *norms, int32_t nrec, int64_t natoms, int32_t nsplit,
               const void *out, GramPlan *plan) {
    *plan = GramPlan{};
    if (!dict || !norms || !out) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(dict, 16) || off(out, 16) || off(norms, 8)) return fail(EPGX_ERR_INVALID, "%s: dict and out must be aligned to 16 bytes, norms to 8", who);
    if (nrec < 1 || natoms < 1) return fail(EPGX_ERR_INVALID, "%s: nrec = %d, natoms = %lld: both must be >= 1", who, nrec, (long long)natoms);
    if (nsplit < 0 || nsplit > natoms) return fail(EPGX_ERR_INVALID, "%s: nsplit = %d not in [0, natoms = %lld]", who, nsplit, (long long)natoms);
    if (!records_extent_ok(nrec, dict_row_stride, natoms, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d records of dict_row_stride = %lld do not hold %lld atoms each (or overflow the address range)", who,
                    nrec, (long long)dict_row_stride, (long long)natoms);
    if (nsplit == 0) nsplit = gram_default_nsplit(nrec, natoms);
    const int32_t nblock = gram_nblock(nrec);
    const int64_t npair = (int64_t)nblock * (nblock + 1) / 2;
    int64_t scratch_len;
    if (npair > (int64_t)0x7fffffff / nsplit || __builtin_mul_overflow((int64_t)nrec * nrec, (int64_t)nsplit, &scratch_len) ||
        scratch_len > INT64_MAX / 16)
        return fail(EPGX_ERR_INVALID, "%s: nsplit = %d partial Gram matrices of %d x %d in one call", who, nsplit, nrec, nrec);
    *plan = GramPlan{nsplit, nblock, (int32_t)npair, scratch_len};
    return EPGX_OK;
}

int project_check(const char *who, const void *basis, int32_t rank, const void *src, int64_t src_row_stride, int32_t nrec, int64_t ncol,
                  const void *out, int64_t out_row_stride) {
    if (!basis || !src || !out) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (off(basis, 16) || off(src, 16) || off(out, 16)) return fail(EPGX_ERR_INVALID, "%s: basis, src and out must be aligned to 16 bytes", who);
    if (nrec < 1 || ncol < 0) return fail(EPGX_ERR_INVALID, "%s: nrec = %d (>= 1), ncol = %lld (>= 0)", who, nrec, (long long)ncol);
    if (rank < 1 || rank > PROJ_MAX_RANK || rank > nrec)
        return fail(EPGX_ERR_INVALID, "%s: rank = %d not in [1, min(%d, nrec = %d)]", who, rank, PROJ_MAX_RANK, nrec);
    if (!records_extent_ok(nrec, src_row_stride, ncol, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d records of src_row_stride = %lld do not hold %lld columns each (or overflow the address range)", who,
                    nrec, (long long)src_row_stride, (long long)ncol);
    if (!records_extent_ok(rank, out_row_stride, ncol, 16))
        return fail(EPGX_ERR_INVALID, "%s: %d rows of out_row_stride = %lld do not hold %lld columns each (or overflow the address range)", who,
                    rank, (long long)out_row_stride, (long long)ncol);
    if (ncol / (PROJ_WAVES * PROJ_TILE) >= 0x7fffffff) return fail(EPGX_ERR_INVALID, "%s: ncol = %lld columns in one call", who, (long long)ncol);
    return EPGX_OK;
}

}  // namespace epgx

// epgx_signal_check.h -- argument checks of the signal consumers: everything the entry points that read a signal, a dictionary or
// a Jacobian left in HBM (epgx_signal.hip) decide before they need the device.
//
//   records_extent_ok      the one "rows of row_stride elements hold cols columns each, and the extent can be addressed" predicate;
//   jacobian_block_check   the block [nrec][nrow][row_stride] of epgx_signal_crlb, _crlb_grad and _refine, in the wording they share;
//   crlb_check ... project_check
//                          one function per entry point (the two norms and the two match entries differ by their element size
//                          alone): the checks of that entry, in the order in which they fire, with the entry's message texts;
//   MatchPlan, GramPlan    the launch facts that fall out of the checks -- the resolved nsplit, the scratch length, the LDS chunks --
//                          so that the entry does not derive them again.
//
// No HIP here.  Device pointers arrive as `const void *`: they are looked at for NULL and alignment and never dereferenced.  What is
// read are the small HOST arrays of the ABI: rows, weights, limit, offsets, record_strides.  `who` is the entry's name, the prefix
// of every message.  A function returns EPGX_OK, or the code of the first failing check with the message left for
// epgx_last_error() (fail).  The context is the entry's business (its NULL guard comes first, in the same words), except where the
// entries already shared a helper that looked at it: nnls_check takes it as one more pointer.  This unit compiles with a plain
// host compiler (tests/host/signal_check.cpp).
#pragma once
#include <cstdint>

#include "../../include/epgx.h"
#include "epgx_error.h"
#include "epgx_signal_limits.h"

namespace epgx {

// `rows` records of `row_stride` elements of `elem_bytes` bytes of which the first `cols` columns are read: false when
// row_stride < cols or the extent (rows - 1) * row_stride + cols cannot be addressed
bool records_extent_ok(int64_t rows, int64_t row_stride, int64_t cols, int64_t elem_bytes);

// nrec records of nrow rows of row_stride complex128 (nrec, nrow >= 1 checked by the caller): the rows fit in a record and the
// elements up to the end of the last record are expressible (the kernel's pointer arithmetic)
int jacobian_block_check(const char *who, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec);

// ------------------------------------------------------------------------------ Cramer-Rao bounds
int crlb_check(const char *who, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec, int32_t nparam,
               const int32_t *rows, int64_t vox0, int64_t nvox, const double *weights, double sigma2, int32_t flags, const void *out);
int crlb_grad_check(const char *who, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                    int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox, const void *hess, int64_t hess_len, int32_t nx,
                    const int64_t *offsets, const int64_t *record_strides, const double *weights, double sigma2, int32_t flags,
                    const void *out_cost, const void *out_grad);

// ------------------------------------------------------------------------------ dictionary matching, complex128 (elem_bytes 16) and complex64 (8)
int norms_check(const char *who, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, const void *out, int elem_bytes);

struct MatchPlan {            // all zero when nmeas = 0: nothing to do
    int64_t nvt;              // voxel tiles of MATCH_VOX
    int32_t nsplit;           // the caller's, or for 0 the library's: four workgroups per compute unit, every split at least one
                              // pass of the workgroup, 65 536 at most (by the launch shape alone: the result does not depend on it)
    int64_t scratch_len;      // MatchPartial blocks: nsplit * nmeas
    int32_t chunk, nchunk;    // records per LDS chunk (a multiple of MATCH_STEP, <= chunk_max) and their number
};
// cu_count: compute units of the device; chunk_max: MATCH_CHUNK or MATCH32_CHUNK
int match_check(const char *who, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms, const void *sig,
                int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit, const void *out_index, const void *out_scale,
                const void *out_score, int cu_count, int elem_bytes, int chunk_max, MatchPlan *plan);

// ------------------------------------------------------------------------------ Gauss-Newton refinement
int refine_check(const char *who, const void *jac, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec, int32_t nparam,
                 const int32_t *rows, int64_t natoms, const void *sig, int64_t sig_row_stride, int64_t nmeas, const void *index,
                 const double *limit, double rcond, const void *out_delta, const void *out_scale, const void *out_score);

// ------------------------------------------------------------------------------ non-negative mixtures
int component_gram_check(const char *who, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                         int64_t nouter, int64_t ninner, const void *out_gram, const void *out_mask);
// the checks epgx_signal_nnls and epgx_signal_nnls_chi2 share
int nnls_check(const char *who, const void *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
               int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig, int64_t sig_row_stride, int64_t nmeas,
               double reg, double tol, const void *group, const void *out_weights, const void *out_group, const void *out_residual,
               const void *out_status);
// what epgx_signal_nnls_chi2 adds: the three outputs of the search in front of nnls_check, its parameters behind
int nnls_chi2_outputs_check(const char *who, const void *out_mu, const void *out_chi2, const void *out_evals);
int nnls_chi2_search_check(const char *who, double reg, double chi2, double chi2_rtol, int32_t max_evals);

// ------------------------------------------------------------------------------ dictionary compression
struct GramPlan {
    int32_t nsplit;           // the caller's, or for 0 gram_default_nsplit(nrec, natoms)
    int32_t nblock, npair;    // record blocks of GRAM_BLOCK and their pairs I <= J
    int64_t scratch_len;      // complex128 elements: nsplit * nrec * nrec
};
int gram_check(const char *who, const void *dict, int64_t dict_row_stride, const void *norms, int32_t nrec, int64_t natoms, int32_t nsplit,
               const void *out, GramPlan *plan);
int project_check(const char *who, const void *basis, int32_t rank, const void *src, int64_t src_row_stride, int32_t nrec, int64_t ncol,
                  const void *out, int64_t out_row_stride);

}  // namespace epgx

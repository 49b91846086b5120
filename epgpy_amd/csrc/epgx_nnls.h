// epgx_nnls.h -- arguments and host-side launchers of the component Gram kernel and the non-negative least-squares kernel
// (epgx_nnls.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"
#include "epgx_signal_limits.h"   // NNLS_MAX_A, NNLS_CHI2_EVALS

namespace epgx {

constexpr int NNLS_WAVES = 4;              // wavefronts (voxels) of a block in the group search; they share the staged H_g
constexpr int NNLS_GRAM_THREADS = 256;     // threads of a block of component_gram_kernel (one block per group)

// the dictionary read as D[t, a, g]: atom a < ncomp of group g = o * ninner + i (o < nouter, i < ninner) of record t at
// dict[t * row_stride + (o * ncomp + a) * axis_stride + i]
struct ComponentArgs {
    const d2 *dict;
    int64_t row_stride;
    int32_t nrec, ncomp;
    int64_t axis_stride, nouter, ninner;
};

struct ComponentGramArgs {
    ComponentArgs c;
    double *gram;                 // [G][ncomp][ncomp]
    unsigned long long *mask;     // [G]: bit a set where H_g[a,a] is finite and > 0
};

struct NnlsArgs {
    ComponentArgs c;
    const double *gram;
    const unsigned long long *mask;
    const d2 *sig;                // record t, voxel m at sig[t * sig_stride + m]
    int64_t sig_stride, nmeas;
    double reg, tol;
    const int64_t *group;         // NULL: search every group; else [nmeas], outside [0, G): the voxel reads nothing
    double *weights;              // [ncomp][nmeas]
    int64_t *out_group;           // [nmeas]
    double *residual;             // [nmeas]
    int32_t *status;              // [nmeas]
};

// the chi^2-driven ridge (include/epgx.h epgx_signal_nnls_chi2): the bracket grows by this factor per evaluation from mu_0, and a
// voxel's search ends after NNLS_CHI2_EVALS fits (DESIGN 4.17 has the counts both come from)
constexpr double NNLS_CHI2_FACTOR = 16.0;

struct NnlsChi2Args {
    NnlsArgs n;                   // group is never NULL here: the caller's, or what nnls_kernel wrote to out_group just before
    double chi2, rtol;
    int32_t max_evals;            // NNLS_CHI2_EVALS (a test lowers it)
    double *mu;                   // [nmeas]
    double *ratio;                // [nmeas]: Jd(mu) / Jd(mu_0)
    int32_t *evals;               // [nmeas]
};

// LDS of a block of nnls_kernel: H_g (A x A doubles), per wavefront the strict lower triangle of the passive-set Cholesky factor
// (A (A - 1) / 2 doubles; the diagonal lives in registers as its inverse) and 64 ints of scratch for compactions.
// A = 64: 32 KiB + waves x 16 000 B: 95.5 KiB for the 4 wavefronts of the search, 47.8 KiB for the single one of a fixed group
constexpr size_t nnls_lds_bytes(int A, int waves) {
    return sizeof(double) * ((size_t)A * A + (size_t)waves * (A * (A - 1) / 2)) + sizeof(int) * 64 * (size_t)waves;
}

}  // namespace epgx

// every field validated by the caller (epgx_signal_component_gram, epgx_signal_nnls)
hipError_t epgx_launch_component_gram(hipStream_t stream, const epgx::ComponentGramArgs &a);
hipError_t epgx_launch_nnls(hipStream_t stream, const epgx::NnlsArgs &a);
// (epgx_nnls_chi2.hip; validated by epgx_signal_nnls_chi2)  One wavefront, one block per voxel
hipError_t epgx_launch_nnls_chi2(hipStream_t stream, const epgx::NnlsChi2Args &a);

// epgx_refine.h -- arguments and host-side launcher of the Gauss-Newton refinement kernel (epgx_refine.hip).  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"
#include "epgx_signal_limits.h"   // REFINE_MAX_P

namespace epgx {

constexpr int REFINE_UNROLL = 2;           // records whose loads a lane has in flight (REFINE_UNROLL x (2 + P) loads of 16 bytes)
constexpr int REFINE_SLICE = 16;           // up to this many records one wavefront sums all records of its voxels
constexpr int REFINE_MAX_SLICES = 8;       // wavefronts that share the records of a voxel (1, 2, 4 or 8)
constexpr int REFINE_MEET = 8;             // partial sums that meet in LDS at a time: (slices - 1) x 8 x 64 doubles, 28 KiB at most

// fp64 partial sums of a lane: n, E, c (2), b (2 P), h (2 P) and the lower triangle of Re M
constexpr int refine_sums(int P) { return 4 + 4 * P + P * (P + 1) / 2; }

struct RefineArgs {
    const d2 *jac;                // record t, row r, atom a at jac[t * record_stride + r * row_stride + a]; row 0: the dictionary
    int64_t record_stride, row_stride;
    int32_t nrec;
    int32_t rows[REFINE_MAX_P];   // the row of every chosen column, >= 1
    int64_t natoms;
    const d2 *sig;                // record t, voxel m at sig[t * sig_stride + m]
    int64_t sig_stride, nmeas;
    const int64_t *index;         // [nmeas]; outside [0, natoms): the voxel loads nothing and comes back unresolved
    double limit[REFINE_MAX_P];   // |delta_p| <= limit_p (+Inf for none)
    double rcond;
    int32_t slices, slice_len;    // refine_slices(nrec): a function of nrec ALONE (the order of the sums must not depend on nmeas)
    double *delta;                // [P][nmeas]
    d2 *scale;                    // [nmeas]
    double *score;                // [nmeas]
};

// how the records of a voxel are cut into slices: 1 slice up to 16 records, 2 up to 32, 4 up to 64, 8 beyond -- by nrec alone,
// so that the association order of a voxel's sums (and with it every bit of its result) is the same in every launch.  Shorter
// slices than crlb_slices': the gather of an atom's columns is bound by latency, and a call over few voxels needs the waves
inline void refine_slices(int32_t nrec, int32_t *slices, int32_t *slice_len) {
    int s = 1;
    while (s < REFINE_MAX_SLICES && (int64_t)s * REFINE_SLICE < nrec) s *= 2;
    const int32_t len = (nrec + s - 1) / s;
    *slices = s;
    *slice_len = (len + REFINE_UNROLL - 1) / REFINE_UNROLL * REFINE_UNROLL;
}

// wavefronts of a block = slices x voxel groups (64 voxels each): 4 wavefronts up to 4 slices, 8 at 8 slices
inline int refine_voxel_groups(int slices) { return slices >= 4 ? 1 : 4 / slices; }

}  // namespace epgx

// nparam = 1 .. REFINE_MAX_P; every other field of `a` validated by the caller (epgx_signal_refine)
hipError_t epgx_launch_refine(hipStream_t stream, int nparam, const epgx::RefineArgs &a);

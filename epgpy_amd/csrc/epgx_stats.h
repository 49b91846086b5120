// epgx_stats.h -- arguments and host-side launchers of the Cramer-Rao kernels (epgx_stats.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"
#include "epgx_signal_limits.h"   // CRLB_MAX_P

namespace epgx {

constexpr int CRLB_UNROLL = 4;             // records whose loads a lane has in flight (CRLB_UNROLL x P loads of 16 bytes)
constexpr int CRLB_SLICE = 64;             // up to this many records one wavefront sums all records of its voxels
constexpr int CRLB_MAX_SLICES = 8;         // wavefronts that share the records of a voxel (1, 2, 4 or 8)
constexpr int CRLB_FLAG_SPLIT = 1;         // = EPGX_CRLB_SPLIT: one bound per column instead of their weighted sum
constexpr int CRLB_FLAG_LOG10 = 2;         // = EPGX_CRLB_LOG10
constexpr int CRLB_GRAD_XB = 4;            // design variables one crlb_grad_kernel launch takes together (G_x of XB variables in registers)

struct CrlbArgs {
    const d2 *signal;             // record r, column c, voxel v at signal[r * record_stride + rows[c] * row_stride + v]
    int64_t record_stride, row_stride;
    int32_t nrec;
    int32_t rows[CRLB_MAX_P];
    int64_t vox0, nvox;           // voxels [vox0, vox0 + nvox) of every row; out[j] belongs to voxel vox0 + j
    double w[CRLB_MAX_P];         // weights (1 for none)
    double inv_sigma2;
    int32_t flags;
    int32_t slices, slice_len;    // crlb_slices(nrec): a function of nrec ALONE (the order of the sum must not depend on nvox)
    double *out;                  // [nvox], or with CRLB_FLAG_SPLIT [P][nvox]
};

// one chunk of up to CRLB_GRAD_XB design variables for crlb_grad_kernel, next to the CrlbArgs of the Jacobian (whose `out` is
// the cost [nvox], written when `write_cost` is set: every chunk computes it, the first one stores it)
struct CrlbGradArgs {
    const d2 *hess;               // entry (a, x) of record r, voxel v at hess[off[x][a] + r * stride[x][a] + v]; off < 0: all zero
    int64_t off[CRLB_GRAD_XB][CRLB_MAX_P], stride[CRLB_GRAD_XB][CRLB_MAX_P];
    int32_t nx;                   // design variables of this chunk, 1 .. CRLB_GRAD_XB
    int32_t write_cost;
    double *grad;                 // [nx][nvox] of this chunk
};

// how the records of a voxel are cut into slices: 1 slice up to 64 records, then 2, 4, 8 -- by nrec alone, so that the
// association order of a voxel's sum (and with it every bit of its result) is the same in every launch
inline void crlb_slices(int32_t nrec, int32_t *slices, int32_t *slice_len) {
    int s = 1;
    while (s < CRLB_MAX_SLICES && (int64_t)s * CRLB_SLICE < nrec) s *= 2;
    const int32_t len = (nrec + s - 1) / s;
    *slices = s;
    *slice_len = (len + CRLB_UNROLL - 1) / CRLB_UNROLL * CRLB_UNROLL;
}

// wavefronts of a block = slices x voxel groups (64 voxels each): 4 wavefronts up to 4 slices, 8 at 8 slices
inline int crlb_voxel_groups(int slices) { return slices >= 4 ? 1 : 4 / slices; }

}  // namespace epgx

// nparam = 1 .. CRLB_MAX_P; every other field of `a` validated by the caller (epgx_signal_crlb)
hipError_t epgx_launch_crlb(hipStream_t stream, int nparam, const epgx::CrlbArgs &a);
// the same for one chunk of design variables (epgx_signal_crlb_grad); CRLB_FLAG_SPLIT must not be set
hipError_t epgx_launch_crlb_grad(hipStream_t stream, int nparam, const epgx::CrlbArgs &a, const epgx::CrlbGradArgs &h);

// epgx_prune.h -- arguments and host-side launchers of the per-voxel float shift (epgx_prune.hip; epgpy/shift.py:478-629
// `shiftprune`): every voxel carries its own coordinate set next to its state.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"

namespace epgx {

constexpr int PRUNE_K = 64;            // stored orders of a voxel, in and out: one per lane
constexpr int PRUNE_CAND = 3 * PRUNE_K;    // candidates of a shift: Z stays, F moves by +s, the mirror of F by -s
constexpr int PRUNE_SLOTS = 3;         // destination rows a lane holds before the prune (PRUNE_CAND / 64)
constexpr int PRUNE_MAX_DIMS = 8;      // grid axes of the shift table
constexpr int PRUNE_MAX_BLOCKS = 65536;    // one wavefront per block; the rest by the grid-stride loop

struct PruneArgs {
    d2 *dst;                  // [nvox][3][64]
    const d2 *src;            // [nvox][3][64]
    double *kdst;             // [nvox][kdim][64]
    const double *ksrc;       // [nvox][kdim][64]
    int32_t *ndst;            // [nvox] live stored rows of the destination
    const int32_t *nsrc;      // [nvox]
    int64_t nvox;
    int32_t kdim;
    // the shift of voxel v: table[sum_d ((v / vstride[d]) % shape[d]) * sstride[d]][kdim]; an axis the shift does not vary along
    // has sstride 0
    const double *table;
    int32_t ndim;
    int64_t shape[PRUNE_MAX_DIMS], vstride[PRUNE_MAX_DIMS], sstride[PRUNE_MAX_DIMS];
    double scale_in[4];       // coordinates -> wavenumbers (ktvalue)
    double scale_out[4];      // divisor on the way back
    double grid[4];
    int32_t nmax;             // trim to this many positive rows; < 0: no trim
    int32_t prune;            // remove the rows whose norm is <= tol
    double tol;
    int32_t *partial;         // [nblocks][2]: largest live count, overflow flag of the voxels of a block
    int32_t *result;          // [2]: the same over all blocks
    int32_t nblocks;
};

struct PruneReadArgs {
    const d2 *state;          // [nvox][3][64]
    const double *k;          // [nvox][4][64]
    const int32_t *nlive;     // [nvox]
    int64_t nvox;
    double tscale;            // time coordinate -> accumulated time (tvalue)
    d2 *out;                  // [nvox]
};

struct CoordsWidenArgs {
    double *dst;              // [nvox][kd][64]
    const double *src;        // [nsrc][ks][64], nsrc = nvox or 1 (broadcast)
    int32_t *ndst;
    const int32_t *nsrc_rows;
    int64_t nvox;
    int32_t kd, ks, broadcast;
};

}  // namespace epgx

// every field validated by the caller (epgx_state_prune_shift / epgx_state_prune_read / epgx_coords_*)
hipError_t epgx_launch_prune_shift(hipStream_t stream, const epgx::PruneArgs &a);
hipError_t epgx_launch_prune_read(hipStream_t stream, const epgx::PruneReadArgs &a);
hipError_t epgx_launch_coords_widen(hipStream_t stream, const epgx::CoordsWidenArgs &a);

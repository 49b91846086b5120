// epgx_launch_tiled.h -- launchers of the tiled kernels for state matrices of any length (epgx_tiled.hip); included by
// epgx_api.hip and epgx_tiled.hip only.  Not part of the public ABI.
#pragma once
#include "epgx_launch.h"

namespace epgx {
// one launch of tiled_kernel<M, H, NSP>: records [rec0, rec1) of `recs` on `tiles` tiles of every voxel of the slab
struct TiledArgs {
    const d2 *in;                       // [nvox][3][Kbuf]: the state before the block
    d2 *out;                            // [nvox][3][Kbuf]: the interiors of the launched tiles after it
    double *dens;                       // [nvox]: density, read and written by tile 0
    int64_t nvox;
    const Rec *recs;                    // fused records (device), two padding records behind the last
    const double *coef;
    d2 *signal;                         // &signal[0][signal_col0 + first voxel of the slab], or null
    int64_t signal_ld;
    int32_t rec0, rec1, Kbuf, tiles;
    RunTail t;                          // vidx (offset to the slab), vidx_ld, vox0, dense_spaces
};
// one launch of tiled_deriv_kernel<M, H, NSP, V>: as above with `in` / `out` [nvox][1 + V][3][Kbuf] (the state, then the V
// derivative states of a voxel) and 1 + V signal rows per ADC
struct TiledDerivArgs {
    TiledArgs a;
    const DRec *drecs;                  // parallel to a.recs (device), two padding records behind the last
    int32_t through_plain;              // SPOILER also acts on the derivative states (EPGX_DERIV_THROUGH_PLAIN_OPS)
};
}  // namespace epgx

// orders per lane of the tiled kernel and its halo: (8, 32) or (16, 64); hipErrorInvalidValue for another pair
hipError_t epgx_launch_tiled(hipStream_t stream, const epgx::TiledArgs &a, int M, int H, int n_spaces);
// a shift by n (|n| > H) of orders [0, kcov) with the k = 0 fold and the truncation above kmax: in -> out
hipError_t epgx_launch_tiled_shift(hipStream_t stream, const epgx::d2 *in, epgx::d2 *out, int64_t nvox, int32_t Kbuf, int32_t kcov,
                                   int32_t n, int32_t kmax);
// equilibrium: Z_0 = density (dens_in, or 1 where null) into a zeroed buffer, the density into dens
// (`windows`: state windows [3][Kbuf] per voxel -- 1, or 1 + V of a derivative plan, whose first is the state)
hipError_t epgx_launch_tiled_equilibrium(hipStream_t stream, epgx::d2 *buf, double *dens, const double *dens_in, int64_t nvox,
                                         int32_t Kbuf, int32_t windows);
// a block of a derivative plan with n_vars = 1 or 2 derivative states: (M, H) = (8, 32) only
hipError_t epgx_launch_tiled_deriv(hipStream_t stream, const epgx::TiledDerivArgs &da, int M, int H, int n_spaces, int n_vars);

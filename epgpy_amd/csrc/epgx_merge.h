// epgx_merge.h -- arguments and host-side launchers of the two device primitives behind the float-wavenumber shift
// (epgx_merge.hip): per-order reductions of a state over all voxels, and the multi-source gather.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"

namespace epgx {

constexpr int STATS_WAVES = 4;             // wavefronts per block, each with its own slab of voxels
constexpr int STATS_MIN_SLAB = 64;         // voxels per wavefront at least
constexpr int STATS_MAX_BLOCKS = 2048;     // blocks per 64 orders at most (the partials of one call: 2048 x 4 x K doubles)
constexpr int STATS_UNROLL = 4;            // voxels whose three lines a lane has in flight
constexpr int STATS_FINAL_Y = 16;         // wavefronts of the second pass, each over every sixteenth block
constexpr int MERGE_WAVES = 4;             // wavefronts (= voxels in flight) per block
constexpr int MERGE_MAX_ROWS = 1024;       // stored orders of a merge destination
constexpr int MERGE_ORDER_MASK = 0xffff;   // a source entry: order | component << 16 | conjugate << 30
constexpr int MERGE_COMP_SHIFT = 16;
constexpr int MERGE_CONJ = 1 << 30;        // (= GS_CONJ of the single-source gather)

// voxels per wavefront and blocks of a row_stats launch: functions of nvox ALONE, so that the association order of every
// sum -- and with it every bit of the result -- is the same in every call on a state of that size
inline int64_t stats_slab(int64_t nvox) {
    const int64_t per = (int64_t)STATS_MAX_BLOCKS * STATS_WAVES;
    const int64_t s = (nvox + per - 1) / per;
    return s < STATS_MIN_SLAB ? STATS_MIN_SLAB : s;
}
inline int64_t stats_blocks(int64_t nvox) {
    const int64_t per = stats_slab(nvox) * STATS_WAVES;
    return (nvox + per - 1) / per;
}

struct RowStatsArgs {
    const d2 *state;      // [nvox][3][K]
    int32_t K;
    int64_t nvox, slab;   // slab = stats_slab(nvox)
    int32_t nblocks;      // stats_blocks(nvox)
    double *partial;      // device scratch [nblocks][4][K]: per block sum |A|, sum |B|, sum |Z|, max modulus of every order
    double *out;          // device [4][K]: the same over all voxels
};

struct MergeArgs {
    d2 *dst;              // [nvox][3][Kd]
    const d2 *src;        // [nvox][3][Ks]
    int32_t Kd, Ks, nrow;
    int64_t nvox;
    const int32_t *offsets;   // device [3][nrow + 1]: sources[offsets[c][j] .. offsets[c][j + 1]) feed component c of order j
    const int32_t *sources;   // device
};

}  // namespace epgx

// every field validated by the caller (epgx_state_row_stats / epgx_state_merge)
hipError_t epgx_launch_row_stats(hipStream_t stream, const epgx::RowStatsArgs &a);
hipError_t epgx_launch_merge(hipStream_t stream, const epgx::MergeArgs &a);

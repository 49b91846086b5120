// epgx_grow_lanes_odd.hip -- instantiates epgx::rows_grow_lanes_kernel_odd<NSP, C> (an echo train with one voxel per lane, the
// orders whose parity reaches an echo alone: epgx_grow_lanes_odd_kernels.hip.h) for one NSP (compile with -DEPGX_NSP=0|1|2|4)
// and exports its launcher.
#include <utility>

#define EPGX_SUMDIFF 1   // as in epgx_grow_lanes.hip: rotations about x in the sum / difference form
#include "epgx_grow_lanes_odd_kernels.hip.h"
#include "epgx_launch_grow.h"

#ifndef EPGX_NSP
#error "compile with -DEPGX_NSP=<index spaces>"
#endif
#define EPGX_CAT2(a, b) a##b
#define EPGX_CAT(a, b) EPGX_CAT2(a, b)

using namespace epgx;

#if EPGX_NSP == 1
int epgx_lanes_odd_cells() { return LANES_ODD_CELLS; }   // (one definition for the four units)
#endif

// rem0: shifts up to the last probe; L: the largest live count (lanes_plan), 1 <= L <= 24.  The host sends LanesPlan::odd lists only
hipError_t EPGX_CAT(epgx_launch_rows_grow_lanes_odd_nsp, EPGX_NSP)(hipStream_t stream, const RunArgs &a, int rem0, int L) {
    if (L < 1 || lanes_odd_cells(L) > LANES_ODD_CELLS) return hipErrorInvalidValue;
    const unsigned groups = (unsigned)((a.nvox + 63) / 64);   // one wave of 64 voxels per workgroup
    RunTail t = a.t;
    t.n_blocks = groups;
    hipLaunchKernelGGL((rows_grow_lanes_kernel_odd<EPGX_NSP, LANES_ODD_CELLS>), dim3(groups), dim3(64), 0, stream, a.nvox, a.recs, a.coef, a.signal,
                       a.signal_ld, t, rem0);
    return hipGetLastError();
}

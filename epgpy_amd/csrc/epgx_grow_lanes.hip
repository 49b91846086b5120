// epgx_grow_lanes.hip -- instantiates epgx::rows_grow_lanes_kernel<NSP, TRAIN> (the growing launch of an echo train with one voxel
// per lane: epgx_grow_lanes_kernels.hip.h) for one NSP (compile with -DEPGX_NSP=0|1|2|4), both values of TRAIN, and exports its launcher.
#include <utility>

#define EPGX_SUMDIFF 1   // as in epgx_grow.hip: the unit this kernel is bit-identical to runs rotations about x in the sum / difference form
#include "epgx_grow_lanes_kernels.hip.h"
#include "epgx_launch_grow.h"

#ifndef EPGX_NSP
#error "compile with -DEPGX_NSP=<index spaces>"
#endif
#define EPGX_CAT2(a, b) a##b
#define EPGX_CAT(a, b) EPGX_CAT2(a, b)

using namespace epgx;

#if EPGX_NSP == 1
int epgx_lanes_deck(bool train) { return train ? EPGX_LANES_TRAIN_DECK : EPGX_LANES_DECK; }   // (one definition for the four units)
#endif

// rem0: shifts up to the last probe; L: the largest live count (lanes_plan, epgx_planner.cpp), 1 <= L <= 24; body: Knobs::lanes_body;
// train: the instantiation without a generic body (LanesPlan::train and the knobs: epgx_launch_rows_grow)
hipError_t EPGX_CAT(epgx_launch_rows_grow_lanes_nsp, EPGX_NSP)(hipStream_t stream, const RunArgs &a, int rem0, int L, int body, bool train) {
    if (L < 1 || L > LANES_CAP) return hipErrorInvalidValue;
    const unsigned groups = (unsigned)((a.nvox + 63) / 64);   // one wave of 64 voxels per workgroup
    RunTail t = a.t;
    t.n_blocks = groups;
    const size_t lds = epgx_lanes_lds_bytes(L, train ? EPGX_LANES_TRAIN_DECK : EPGX_LANES_DECK);   // the slots above the chosen kernel's deck
    if (train)
        hipLaunchKernelGGL((rows_grow_lanes_kernel<EPGX_NSP, true>), dim3(groups), dim3(64), lds, stream, a.nvox, a.recs, a.coef, a.signal, a.signal_ld, t, rem0, L, body);
    else
        hipLaunchKernelGGL((rows_grow_lanes_kernel<EPGX_NSP, false>), dim3(groups), dim3(64), lds, stream, a.nvox, a.recs, a.coef, a.signal, a.signal_ld, t, rem0, L, body);
    return hipGetLastError();
}

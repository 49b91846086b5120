// epgx_xrun.hip -- instantiates epgx::xrun_kernel<EPGX_NC, M, HAS_IN> for one number of compartments (compile with
// -DEPGX_NC=2|3|4): M in {1, 2, 4} with NC * M <= 8, each for resident (HAS_IN false) and stream (HAS_IN true) launches.
#include "epgx_xrun_kernels.hip.h"

#ifndef EPGX_NC
#error "compile with -DEPGX_NC=<compartments>"
#endif
#define EPGX_CAT2(a, b) a##b
#define EPGX_CAT(a, b) EPGX_CAT2(a, b)

using namespace epgx;

template <int M, bool HAS_IN>
static hipError_t launch_xrun(hipStream_t stream, const XRunArgs &a, int64_t ngroups) {
    hipLaunchKernelGGL((xrun_kernel<EPGX_NC, M, HAS_IN>), dim3((unsigned)ngroups), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// M = orders per lane (K / 64); hipErrorInvalidValue for a shape this unit does not instantiate
hipError_t EPGX_CAT(epgx_launch_xrun_nc, EPGX_NC)(hipStream_t stream, const XRunArgs &a, int64_t ngroups, int M) {
    const bool has_in = a.in != nullptr;
    switch (M) {
    case 1: return has_in ? launch_xrun<1, true>(stream, a, ngroups) : launch_xrun<1, false>(stream, a, ngroups);
    case 2: return has_in ? launch_xrun<2, true>(stream, a, ngroups) : launch_xrun<2, false>(stream, a, ngroups);
#if EPGX_NC <= 2
    case 4: return has_in ? launch_xrun<4, true>(stream, a, ngroups) : launch_xrun<4, false>(stream, a, ngroups);
#endif
    default: return hipErrorInvalidValue;
    }
}

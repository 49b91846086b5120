// epgx_dxrun.hip -- instantiates epgx::dxrun_kernel<EPGX_NC, M, V> for one number of compartments (compile with
// -DEPGX_NC=2|3|4): exactly the shapes with NC * M * (1 + V) <= 8 -- NC = 2: (M, V) = (1, 1 .. 3), (2, 1); NC = 3, 4: (1, 1).
#include "epgx_dxrun_kernels.hip.h"

#ifndef EPGX_NC
#error "compile with -DEPGX_NC=<compartments>"
#endif
#define EPGX_CAT2(a, b) a##b
#define EPGX_CAT(a, b) EPGX_CAT2(a, b)

using namespace epgx;

template <int M, int V>
static hipError_t launch_dxrun(hipStream_t stream, const DXRunArgs &a, int64_t ngroups) {
    hipLaunchKernelGGL((dxrun_kernel<EPGX_NC, M, V>), dim3((unsigned)ngroups), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// M = orders per lane (K / 64), V = derivative states; hipErrorInvalidValue for a shape this unit does not instantiate
hipError_t EPGX_CAT(epgx_launch_dxrun_nc, EPGX_NC)(hipStream_t stream, const DXRunArgs &a, int64_t ngroups, int M, int V) {
    if (M == 1 && V == 1) return launch_dxrun<1, 1>(stream, a, ngroups);
#if EPGX_NC == 2
    if (M == 1 && V == 2) return launch_dxrun<1, 2>(stream, a, ngroups);
    if (M == 1 && V == 3) return launch_dxrun<1, 3>(stream, a, ngroups);
    if (M == 2 && V == 1) return launch_dxrun<2, 1>(stream, a, ngroups);
#endif
    return hipErrorInvalidValue;
}

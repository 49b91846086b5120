// epgx_hess.hip -- instantiates epgx::hess_kernel<M, NSP, DIAG> (M = 1, 2, 4, 8: the capacities at which a launch carries three
// derivative states) and exports its launcher.
#include "epgx_hess_kernels.hip.h"
#include "epgx_launch_hess.h"

using namespace epgx;

template <int M, int NSP, bool DIAG>
static hipError_t launch(hipStream_t stream, const DerivArgs &a) {
    const unsigned blocks = (unsigned)(((a.nvox + 3) / 4 + 15) / 16 * 16);
    const size_t lds = sizeof(d2) * 4 * (size_t)a.t.use_lds * 64 * M;      // four wavefronts x (2 | 3) arrays of K complex, or nothing
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)hess_kernel<M, NSP, DIAG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((hess_kernel<M, NSP, DIAG>), dim3(blocks), dim3(256), lds, stream, a);
    return hipGetLastError();
}

template <int M, bool DIAG>
static hipError_t launch_nsp(hipStream_t stream, const DerivArgs &a, int n_spaces) {
    if constexpr (M == 8 && !DIAG) {
        // hess_kernel<8, 1, false> is the one instantiation the compiler gives scratch (32 bytes per lane): a plan with one index space
        // runs the two-space kernel, its missing space marked dense (no index row is read for it, no record refers to it)
        if (n_spaces == 1) {
            DerivArgs b = a;
            b.t.dense_spaces |= 2u;
            return launch<M, 2, DIAG>(stream, b);
        }
    }
    switch (n_spaces) {
    case 0: return launch<M, 0, DIAG>(stream, a);
    case 1:
        if constexpr (M == 8 && !DIAG) return hipErrorInvalidValue; else return launch<M, 1, DIAG>(stream, a);
    case 2: return launch<M, 2, DIAG>(stream, a);
    default: return launch<M, 4, DIAG>(stream, a);
    }
}

template <bool DIAG>
static hipError_t launch_k(hipStream_t stream, const DerivArgs &a, int K, int n_spaces) {
    if (K == 64) return launch_nsp<1, DIAG>(stream, a, n_spaces);
    if (K == 128) return launch_nsp<2, DIAG>(stream, a, n_spaces);
    if (K == 256) return launch_nsp<4, DIAG>(stream, a, n_spaces);
    if (K == 512) return launch_nsp<8, DIAG>(stream, a, n_spaces);
    return hipErrorInvalidValue;
}

hipError_t epgx_launch_hess(hipStream_t stream, const DerivArgs &a, int K, int n_spaces, bool diag) {
    return diag ? launch_k<true>(stream, a, K, n_spaces) : launch_k<false>(stream, a, K, n_spaces);
}

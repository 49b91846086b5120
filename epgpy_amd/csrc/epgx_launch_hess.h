// epgx_launch_hess.h -- host-side launcher of hess_kernel (epgx_hess.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace epgx { struct DerivArgs; }
// one-pair second-order passes (EPGX_DERIV_SECOND): K = 64, 128, 256, 512; diag: the pair (a, a), three states instead of four
hipError_t epgx_launch_hess(hipStream_t stream, const epgx::DerivArgs &a, int K, int n_spaces, bool diag);

// epgx_chain.h -- arguments and host-side launcher of chain_kernel (epgx_chain.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"

namespace epgx {

struct ChainArgs {
    double *pool;                    // the plan's coefficient pool (sources and destination)
    const epgx_chain_step *steps;    // device copy of the chain's steps, offsets final
    int64_t dst_off, n_entries;
    int32_t n_steps, ndim;
    int64_t shape[EPGX_MAX_DIMS], dst_str[EPGX_MAX_DIMS];
    int64_t sp_str[EPGX_MAX_SPACES][EPGX_MAX_DIMS];   // strides of every index space of the plan
};

}  // namespace epgx

hipError_t epgx_launch_chain(hipStream_t stream, const epgx::ChainArgs &a);

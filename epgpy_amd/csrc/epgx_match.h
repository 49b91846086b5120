// epgx_match.h -- arguments and host-side launchers of the dictionary-matching kernels (epgx_match.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"
#include "epgx_signal_limits.h"   // the MATCH_ constants and MatchPartial

namespace epgx {

struct MatchArgs {
    const d2 *dict;               // D[t][a] at dict[t * dict_stride + a]
    int64_t dict_stride;
    const double *norms;          // n_a
    int64_t natoms;
    const d2 *sig;                // S[t][m] at sig[t * sig_stride + m]
    int64_t sig_stride;
    int64_t nmeas, nvt;           // nvt = voxel tiles of MATCH_VOX; block b: voxel tile b % nvt, split b / nvt
    int32_t nrec, nsplit;
    int32_t chunk, nchunk;        // records per LDS chunk (a multiple of MATCH_STEP, <= MATCH_CHUNK) and their number
    MatchPartial *part;           // [nsplit][nmeas]
};

struct MatchMergeArgs {
    const MatchPartial *part;
    const double *norms;
    const d2 *sig;
    int64_t sig_stride, nmeas;
    int32_t nrec, nsplit;
    int64_t *index;
    d2 *scale;
    double *score;
};

// atoms [*a0, *a1) of split s: natoms / nsplit each, the first natoms % nsplit splits one more
__host__ __device__ inline void match_split(int64_t natoms, int32_t nsplit, int32_t s, int64_t *a0, int64_t *a1) {
    const int64_t q = natoms / nsplit, r = natoms % nsplit;
    *a0 = s * q + (s < r ? s : r);
    *a1 = *a0 + q + (s < r ? 1 : 0);
}

}  // namespace epgx

// every field validated by the caller (epgx_signal_norms / epgx_signal_match)
hipError_t epgx_launch_norms(hipStream_t stream, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, double *out);
hipError_t epgx_launch_match(hipStream_t stream, const epgx::MatchArgs &a);
hipError_t epgx_launch_match_merge(hipStream_t stream, const epgx::MatchMergeArgs &a);

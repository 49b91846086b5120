// epgx_match32.h -- arguments and host-side launchers of the single-precision matching kernels (epgx_match32.hip).  Not part of the
// public ABI.  MatchPartial, match_split and the tile constants are those of epgx_match.h: the splits and their reduction follow
// one rule in both precisions.
#pragma once
#include "epgx_match.h"

namespace epgx {

typedef float f2 __attribute__((ext_vector_type(2)));      // (MATCH32_CHUNK: epgx_signal_limits.h)

struct Match32Args {
    const f2 *dict;               // D32[t][a] at dict[t * dict_stride + a]
    int64_t dict_stride;
    const double *norms;          // n_a (fp64)
    int64_t natoms;
    const f2 *sig;                // S32[t][m] at sig[t * sig_stride + m]
    int64_t sig_stride;
    int64_t nmeas, nvt;           // nvt = voxel tiles of MATCH_VOX; block b: voxel tile b % nvt, split b / nvt
    int32_t nrec, nsplit;
    int32_t chunk, nchunk;        // records per LDS chunk (a multiple of MATCH_STEP, <= MATCH32_CHUNK) and their number
    MatchPartial *part;           // [nsplit][nmeas]
};

struct Match32MergeArgs {
    const MatchPartial *part;
    const double *norms;
    const f2 *sig;
    int64_t sig_stride, nmeas;
    int32_t nrec, nsplit;
    int64_t *index;
    d2 *scale;
    double *score;
};

}  // namespace epgx

// every field validated by the caller (epgx_signal_norms_c64 / epgx_signal_match_c64)
hipError_t epgx_launch_norms32(hipStream_t stream, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, double *out);
hipError_t epgx_launch_match32(hipStream_t stream, const epgx::Match32Args &a);
hipError_t epgx_launch_match32_merge(hipStream_t stream, const epgx::Match32MergeArgs &a);

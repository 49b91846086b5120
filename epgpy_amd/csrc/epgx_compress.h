// epgx_compress.h -- arguments and host-side launchers of the dictionary-compression kernels (epgx_compress.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_match.h"

namespace epgx {

// (GRAM_TILE, GRAM_WAVES, GRAM_BLOCK, gram_nblock and the library's own choice of nsplit, gram_default_nsplit: epgx_signal_limits.h)
constexpr int GRAM_STEP = 4;               // atoms one MFMA consumes; the atoms of a split are taken in steps from its first atom
constexpr int GRAM_KC = 16;                // atoms of a record block that LDS holds at a time
constexpr int GRAM_LD = GRAM_KC + 1;       // row pitch of the LDS image in elements (the pad: see epgx_compress.hip)

struct GramArgs {
    const d2 *dict;               // D[t][a] at dict[t * dict_stride + a]
    int64_t dict_stride;
    const double *norms;          // n_a: atoms whose n_a is not a finite number > 0 are staged as zeros
    int64_t natoms;
    int32_t nrec, nsplit;
    int32_t nblock, npair;        // record blocks of GRAM_BLOCK; block b: pair b % npair (I <= J, row by row), split b / npair
    d2 *part;                     // [nsplit][nrec][nrec]; only the entries s <= t are written and read
};

struct GramReduceArgs {
    const d2 *part;
    int32_t nrec, nsplit;
    d2 *out;                      // G [nrec][nrec]
};

// (PROJ_TILE, PROJ_WAVES, PROJ_MAX_RANK: epgx_signal_limits.h)
constexpr int PROJ_STEP = 4;               // records one MFMA consumes, from t = 0, the tail padded with zeros
constexpr int PROJ_TILES = 4;              // accumulator tiles of a wavefront: NR rank tiles x NC column tiles, NR * NC = 4
constexpr int PROJ_UNROLL = 4;             // steps whose loads are issued before their MFMAs

struct ProjectArgs {
    const d2 *basis;              // B[t][r] at basis[t * rank + r]
    const d2 *src;                // X[t][c] at src[t * src_stride + c]
    int64_t src_stride, ncol;
    d2 *out;                      // out[r][c] at out[r * out_stride + c]
    int64_t out_stride;
    int32_t nrec, rank;
};

}  // namespace epgx

// every field validated by the caller (epgx_signal_gram / epgx_signal_project)
hipError_t epgx_launch_gram(hipStream_t stream, const epgx::GramArgs &a);
hipError_t epgx_launch_gram_reduce(hipStream_t stream, const epgx::GramReduceArgs &a);
hipError_t epgx_launch_project(hipStream_t stream, const epgx::ProjectArgs &a);

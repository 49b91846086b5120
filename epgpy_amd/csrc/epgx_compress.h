// epgx_compress.h -- arguments and host-side launchers of the dictionary-compression kernels (epgx_compress.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_match.h"

namespace epgx {

constexpr int GRAM_TILE = 16;              // records (rows and columns) of one v_mfma_f64_16x16x4_f64 tile of G
constexpr int GRAM_STEP = 4;               // atoms one MFMA consumes; the atoms of a split are taken in steps from its first atom
constexpr int GRAM_WAVES = 4;              // wavefronts of a workgroup: wavefront w owns row tile w of the workgroup's record block
constexpr int GRAM_BLOCK = GRAM_WAVES * GRAM_TILE;      // records of a record block: a workgroup computes a 64 x 64 block of G
constexpr int GRAM_KC = 16;                // atoms of a record block that LDS holds at a time
constexpr int GRAM_LD = GRAM_KC + 1;       // row pitch of the LDS image in elements (the pad: see epgx_compress.hip)
// The library's own choice of nsplit (epgx_signal_gram with nsplit = 0), a function of (nrec, natoms) alone:
//      nblock = ceil(nrec / 64),  npair = nblock (nblock + 1) / 2      (the 64 x 64 blocks I <= J of G, one workgroup each per split)
//      nsplit = min(ceil(GRAM_WORKGROUPS / npair), max(natoms / GRAM_MIN_ATOMS, 1))
// i.e. about GRAM_WORKGROUPS workgroups as long as every split keeps GRAM_MIN_ATOMS atoms.  Neither the number of compute
// units nor the state of the pool enters: the same dictionary gives the same bits of G on every machine.
constexpr int GRAM_WORKGROUPS = 2048;
constexpr int GRAM_MIN_ATOMS = 1024;

__host__ __device__ inline int32_t gram_nblock(int32_t nrec) { return (nrec + GRAM_BLOCK - 1) / GRAM_BLOCK; }

inline int32_t gram_default_nsplit(int32_t nrec, int64_t natoms) {
    const int64_t nblock = gram_nblock(nrec), npair = nblock * (nblock + 1) / 2;
    const int64_t want = (GRAM_WORKGROUPS + npair - 1) / npair, most = natoms / GRAM_MIN_ATOMS > 1 ? natoms / GRAM_MIN_ATOMS : 1;
    return (int32_t)(want < most ? want : most);
}

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

constexpr int PROJ_TILE = 16;              // basis vectors (rows) and columns of one MFMA tile
constexpr int PROJ_STEP = 4;               // records one MFMA consumes, from t = 0, the tail padded with zeros
constexpr int PROJ_TILES = 4;              // accumulator tiles of a wavefront: NR rank tiles x NC column tiles, NR * NC = 4
constexpr int PROJ_WAVES = 4;              // wavefronts of a workgroup, each with column tiles of its own
constexpr int PROJ_UNROLL = 4;             // steps whose loads are issued before their MFMAs
constexpr int PROJ_MAX_RANK = 64;

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

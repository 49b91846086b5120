// epgx_signal_limits.h -- what the kernels that read a signal, a dictionary or a Jacobian left in HBM and the argument checks in
// front of them (epgx_signal_check.h) must agree on: the limits an entry point refuses beyond, and the tile and split constants a
// launch shape follows from.  Plain C++, no HIP; each kernel header includes this one and keeps what only its kernels read.
#pragma once
#include <cstdint>

namespace epgx {

// Cramer-Rao bounds (epgx_stats.h) and Gauss-Newton refinement (epgx_refine.h)
constexpr int CRLB_MAX_P = 4;              // columns of a Jacobian on the device: 1 + EPGX_MAX_VARS rows per record
constexpr int REFINE_MAX_P = 4;            // columns of the Jacobian one call takes (the limit of epgx_signal_crlb)

// dictionary matching (epgx_match.h, epgx_match32.h)
constexpr int MATCH_TILE = 16;             // atoms (rows) and voxels (columns) of one v_mfma_f64_16x16x4_f64 tile
constexpr int MATCH_STEP = 4;              // records one MFMA consumes; the records of a voxel are taken in steps from t = 0
constexpr int MATCH_VT = 4;                // voxel tiles a wavefront keeps accumulators for: a workgroup owns MATCH_VT * 16 voxels
constexpr int MATCH_VOX = MATCH_VT * MATCH_TILE;
constexpr int MATCH_WAVES = 4;             // wavefronts of a workgroup, one atom tile each per pass
constexpr int MATCH_CHUNK = 32;            // records of the voxel tile that LDS holds at a time (32 KiB); nrec <= 32: staged once per workgroup
constexpr int MATCH32_CHUNK = 64;          // records of the voxel tile that LDS holds at a time: [64][MATCH_VOX] complex64, 32 KiB

// what one (split, voxel) leaves in scratch: the best atom of the split's range (a < 0: none), 32 bytes
struct MatchPartial {
    double q;
    int64_t a;
    double cr, ci;
};
static_assert(sizeof(MatchPartial) == 32, "the scratch of epgx_signal_match is [nsplit][nmeas] blocks of 32 bytes");

// dictionary compression (epgx_compress.h)
constexpr int GRAM_TILE = 16;              // records (rows and columns) of one v_mfma_f64_16x16x4_f64 tile of G
constexpr int GRAM_WAVES = 4;              // wavefronts of a workgroup: wavefront w owns row tile w of the workgroup's record block
constexpr int GRAM_BLOCK = GRAM_WAVES * GRAM_TILE;      // records of a record block: a workgroup computes a 64 x 64 block of G
// The library's own choice of nsplit (epgx_signal_gram with nsplit = 0), a function of (nrec, natoms) alone:
//      nblock = ceil(nrec / 64),  npair = nblock (nblock + 1) / 2      (the 64 x 64 blocks I <= J of G, one workgroup each per split)
//      nsplit = min(ceil(GRAM_WORKGROUPS / npair), max(natoms / GRAM_MIN_ATOMS, 1))
// i.e. about GRAM_WORKGROUPS workgroups as long as every split keeps GRAM_MIN_ATOMS atoms.  Neither the number of compute
// units nor the state of the pool enters: the same dictionary gives the same bits of G on every machine.
constexpr int GRAM_WORKGROUPS = 2048;
constexpr int GRAM_MIN_ATOMS = 1024;

inline int32_t gram_nblock(int32_t nrec) { return (int32_t)(((int64_t)nrec + GRAM_BLOCK - 1) / GRAM_BLOCK); }

inline int32_t gram_default_nsplit(int32_t nrec, int64_t natoms) {
    const int64_t nblock = gram_nblock(nrec), npair = nblock * (nblock + 1) / 2;
    const int64_t want = (GRAM_WORKGROUPS + npair - 1) / npair, most = natoms / GRAM_MIN_ATOMS > 1 ? natoms / GRAM_MIN_ATOMS : 1;
    return (int32_t)(want < most ? want : most);
}

constexpr int PROJ_TILE = 16;              // basis vectors (rows) and columns of one MFMA tile
constexpr int PROJ_WAVES = 4;              // wavefronts of a workgroup, each with column tiles of its own
constexpr int PROJ_MAX_RANK = 64;

// non-negative mixtures (epgx_nnls.h)
constexpr int NNLS_MAX_A = 64;             // atoms along the component axis: one lane of a wavefront each
constexpr int NNLS_CHI2_EVALS = 40;        // fits after which a voxel's chi^2 search ends (DESIGN 4.17 has the count's origin)

}  // namespace epgx

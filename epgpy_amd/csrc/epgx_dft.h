// epgx_dft.h -- arguments and host-side launcher of the spatial read-out (epgx_dft.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "epgx_kernels.hip.h"

namespace epgx {

constexpr int DFT_WAVES = 16;                  // wavefronts per block = stored orders per staged chunk of phasors
constexpr int DFT_VW = 16;                     // voxels per wavefront (accumulators: 2 x DFT_VW doubles per lane)
constexpr int DFT_TV = DFT_WAVES * DFT_VW;     // voxels per block
constexpr int DFT_TP = 64;                     // positions per block: one per lane

struct DftArgs {
    const d2 *state;      // [..][3][K] complex128 (the epgx_state's storage)
    int32_t K, nrow;      // capacity; stored orders used (<= K)
    int64_t vox0, nvox;   // voxel range of the state
    const double *k;      // device [nrow][3]: wavenumber of stored order j (columns beyond d are zero)
    const double *w;      // device [nrow]: voxel factor of stored order j
    const double *pos;    // device [npos][3] (columns beyond d are zero)
    int64_t npos;
    double *table;        // device scratch [nvox rounded up to DFT_VW][nrow][4]: the folded, weighted coefficients
    double phase_re, phase_im;
    d2 *out;              // device [nvox][npos]
};

__host__ __device__ inline int64_t dft_table_voxels(int64_t nvox) { return (nvox + DFT_VW - 1) / DFT_VW * DFT_VW; }

}  // namespace epgx

hipError_t epgx_launch_dft(hipStream_t stream, const epgx::DftArgs &a);

// epgx_exchange_kernels.hip.h -- EPGX_OP_X (multi-compartment exchange, epgpy/exchange.py:89-120) on states in HBM;
// included by epgx_api.hip only (one definition in the library).
//
// One lane per (compartment group, order k): it loads the N x 3 values of order k of the group's N voxels, applies the cell
// of include/epgx.h (EPGX_OP_X) and stores them back in place.  Consecutive lanes take consecutive orders of one voxel, so
// every load and store of a wavefront is one contiguous run of [3][K]; the group's table entry (3 N^2 doubles) is the same
// for the K lanes of the group and comes from the cache.  Memory-bound: 2 x 48 N bytes per lane against 16 N^2 fp64 fma.
#pragma once
#include "epgx_kernels.hip.h"

namespace epgx {

struct XArgs {
    d2 *__restrict__ state;            // [nvox][3][K] of the voxel range (in place)
    const double *__restrict__ dens;   // [nvox] densities of the range
    const double *__restrict__ tab;    // pool + coef_off of the operator
    int64_t ngroups;                   // groups in the range (nvox / N)
    int64_t stride;                    // compartment stride in voxels (epgx_op.ib)
    int64_t vox0;                      // grid voxel of the range's first voxel
    int32_t log2K, ndim, space, reserved;   // space < 0: one table entry for every group
    int64_t shape[EPGX_MAX_DIMS];
    int64_t strides[EPGX_MAX_DIMS];    // the operator's index space
};

template <int N>
__global__ void __launch_bounds__(256) exchange_kernel(const XArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (a.ngroups << a.log2K)) return;
    const int K = 1 << a.log2K;
    const int k = (int)(t & (K - 1));
    const int64_t g = t >> a.log2K;
    // the groups of the range: `stride` of them per block of N * stride voxels, compartment c of group g at v0 + c * stride
    const int64_t outer = g / a.stride, inner = g - outer * a.stride;
    const int64_t v0 = outer * N * a.stride + inner;
    int64_t entry = 0;
    if (a.space >= 0) {
        int64_t rem = a.vox0 + v0;
        for (int d = a.ndim - 1; d >= 0; --d) {
            const int64_t c = rem % a.shape[d];
            rem /= a.shape[d];
            entry += c * a.strides[d];
        }
    }
    const double *__restrict__ mT = a.tab + entry * (3 * N * N);   // Re/Im, row-major
    const double *__restrict__ mL = mT + 2 * N * N;                // real, row-major
    d2 x[3][N];
    double rho[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const d2 *s = a.state + (size_t)(v0 + c * a.stride) * 3 * K + k;
        x[0][c] = s[0];
        x[1][c] = s[K];
        x[2][c] = s[2 * K];
        rho[c] = k == 0 ? a.dens[v0 + c * a.stride] : 0.0;
        x[2][c].x -= rho[c];
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        d2 A = {0.0, 0.0}, B = {0.0, 0.0}, Z = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double mr = mT[2 * (c * N + j)], mi = mT[2 * (c * N + j) + 1], ml = mL[c * N + j];
            A.x = fma(mr, x[0][j].x, fma(-mi, x[0][j].y, A.x));
            A.y = fma(mr, x[0][j].y, fma(mi, x[0][j].x, A.y));
            B.x = fma(mr, x[1][j].x, fma(mi, x[1][j].y, B.x));
            B.y = fma(mr, x[1][j].y, fma(-mi, x[1][j].x, B.y));
            Z.x = fma(ml, x[2][j].x, Z.x);
            Z.y = fma(ml, x[2][j].y, Z.y);
        }
        Z.x += rho[c];
        d2 *s = a.state + (size_t)(v0 + c * a.stride) * 3 * K + k;
        s[0] = A;
        s[K] = B;
        s[2 * K] = Z;
    }
}

}  // namespace epgx

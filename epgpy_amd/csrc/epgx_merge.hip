// epgx_merge.hip -- the two device primitives of the float-wavenumber shift (epgpy/shift.py:367-449 `shiftmerge`;
// include/epgx.h epgx_state_row_stats / epgx_state_merge).
//
// row_stats_kernel: per stored order j the sums over all voxels of |A_j|, |B_j|, |Z_j| and the largest of the three moduli --
// the weights of the merged coordinates (shift.py:420) and the pruning test (:432-434).  The state is [nvox][3][K]: lanes are
// orders, so every load of a wavefront is one 1 KiB line (64 orders x 16 bytes); a wavefront walks its own slab of voxels with
// the three lines of STATS_UNROLL voxels in flight and adds in voxel order.  The four wavefronts of a block meet in LDS (added in
// wavefront order), the blocks' partials in a second kernel (every sixteenth block per wavefront in block order, the wavefronts
// in LDS).  No atomics; slab and grid depend on nvox alone: the same bits in every call.  HBM-bound: 48 K bytes per voxel, every
// byte once.
// A modulus is sqrt(re re + im im) with every operation rounded on its own (no fused multiply-add): NumPy's
// np.sqrt(re * re + im * im) gives the same bits.
//
// merge_kernel: dst[v][c][j] = sum over the sources listed for (c, j) of (conj?) src[v][c_s][i_s], added in the order listed
// from +0 (the bits of np.add.at on zeros); an empty list and every order from nrow on give exact zero.  One wavefront per voxel
// (grid-stride over the voxels), lanes over destination orders, Kd / 64 per lane: loads gather inside the voxel's 48 Ks bytes,
// stores are whole lines.  The table is the same for every voxel and stays in cache.  Plain vector stores only.
#include "epgx_merge.h"

namespace epgx {

__device__ __forceinline__ double modulus(const d2 z) {
#pragma clang fp contract(off)
    const double a = z.x * z.x;
    const double b = z.y * z.y;
    return __builtin_sqrt(a + b);
}

__device__ __forceinline__ void stats_add(double (&s)[3], double &m, const d2 a, const d2 b, const d2 z) {
    const double ma = modulus(a), mb = modulus(b), mz = modulus(z);
    s[0] += ma;
    s[1] += mb;
    s[2] += mz;
    m = fmax(m, fmax(ma, fmax(mb, mz)));
}

__global__ void __launch_bounds__(STATS_WAVES * 64) row_stats_kernel(const RowStatsArgs a) {
    __shared__ double part[STATS_WAVES - 1][4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int K = a.K;
    const int order = (int)blockIdx.y * 64 + lane;      // (K is a multiple of 64: every lane has an order)
    const int64_t v0 = ((int64_t)blockIdx.x * STATS_WAVES + wave) * a.slab;
    const int64_t v1 = v0 + a.slab < a.nvox ? v0 + a.slab : a.nvox;
    const int64_t vstride = (int64_t)3 * K;

    double s[3] = {0.0, 0.0, 0.0}, m = 0.0;
    if (v0 < v1) {      // (wave-uniform)
        const d2 *p = a.state + v0 * vstride + order;
        int64_t v = v0;
        for (; v + STATS_UNROLL <= v1; v += STATS_UNROLL) {
            d2 x[STATS_UNROLL][3];
#pragma unroll
            for (int u = 0; u < STATS_UNROLL; ++u)
#pragma unroll
                for (int c = 0; c < 3; ++c) x[u][c] = p[u * vstride + c * K];
            p += STATS_UNROLL * vstride;
#pragma unroll
            for (int u = 0; u < STATS_UNROLL; ++u) stats_add(s, m, x[u][0], x[u][1], x[u][2]);
        }
        for (; v < v1; ++v) {
            const d2 xa = p[0], xb = p[K], xz = p[2 * K];
            p += vstride;
            stats_add(s, m, xa, xb, xz);
        }
    }

    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) part[wave - 1][q][lane] = s[q];
        part[wave - 1][3][lane] = m;
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < STATS_WAVES - 1; ++w) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += part[w][q][lane];
        m = fmax(m, part[w][3][lane]);
    }
    double *out = a.partial + (int64_t)blockIdx.x * 4 * K + order;
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q * K] = s[q];
    out[3 * K] = m;
}

// out[q][j] = the blocks' partials of (q, j): sums for q < 3, the maximum for q = 3.  A block owns 64 consecutive outputs (one
// q: 3 K is a multiple of 64); its STATS_FINAL_Y wavefronts each take every STATS_FINAL_Y-th block in ascending order (loads of
// 512 contiguous bytes), then meet in LDS in wavefront order: a fixed association order for a given nvox.
__global__ void __launch_bounds__(64 * STATS_FINAL_Y) row_stats_final_kernel(const RowStatsArgs a) {
    __shared__ double part[STATS_FINAL_Y][64];
    const int x = threadIdx.x, y = threadIdx.y;
    const int i = (int)blockIdx.x * 64 + x;      // q * K + j < 4 K
    const bool is_max = (int)blockIdx.x * 64 >= 3 * a.K;
    const int64_t stride = (int64_t)4 * a.K;
    double acc = 0.0;
    for (int b = y; b < a.nblocks; b += STATS_FINAL_Y) {
        const double v = a.partial[b * stride + i];
        acc = is_max ? fmax(acc, v) : acc + v;
    }
    part[y][x] = acc;
    __syncthreads();
    if (y > 0) return;
    for (int w = 1; w < STATS_FINAL_Y; ++w) acc = is_max ? fmax(acc, part[w][x]) : acc + part[w][x];
    a.out[i] = acc;
}

__global__ void __launch_bounds__(MERGE_WAVES * 64) merge_kernel(const MergeArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * MERGE_WAVES;
    for (int64_t v = (int64_t)blockIdx.x * MERGE_WAVES + wave; v < a.nvox; v += step) {
        const d2 *src = a.src + v * 3 * a.Ks;
        d2 *dst = a.dst + v * 3 * a.Kd;
        for (int c = 0; c < 3; ++c) {
            const int32_t *off = a.offsets + c * (a.nrow + 1);
            for (int j = lane; j < a.Kd; j += 64) {
                d2 acc = {0.0, 0.0};
                if (j < a.nrow) {
                    const int32_t end = off[j + 1];
                    for (int32_t s = off[j]; s < end; ++s) {
                        const int32_t ent = a.sources[s];
                        const d2 x = src[((ent >> MERGE_COMP_SHIFT) & 3) * a.Ks + (ent & MERGE_ORDER_MASK)];
                        acc.x += x.x;
                        acc.y += (ent & MERGE_CONJ) ? -x.y : x.y;
                    }
                }
                dst[c * a.Kd + j] = acc;
            }
        }
    }
}

}  // namespace epgx

hipError_t epgx_launch_row_stats(hipStream_t stream, const epgx::RowStatsArgs &a) {
    using namespace epgx;
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)a.nblocks, (unsigned)(a.K / 64)), dim3(STATS_WAVES * 64), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(row_stats_final_kernel, dim3((unsigned)(4 * a.K / 64)), dim3(64, STATS_FINAL_Y), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_merge(hipStream_t stream, const epgx::MergeArgs &a) {
    using namespace epgx;
    const int64_t want = (a.nvox + MERGE_WAVES - 1) / MERGE_WAVES;
    const int64_t cap = (int64_t)256 * 8 * 16;      // (a few blocks per CU in flight; the rest by the grid-stride loop)
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(MERGE_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

// epgx_stats.hip -- Cramer-Rao lower bounds from a Jacobian that stays in HBM (include/epgx.h epgx_signal_crlb):
//      I(v) = 1 / sigma2 * Re( J(v)^H J(v) )          J(v) [nrec][P]: column c of record r at row rows[c] of the record
//      lb(v) = I(v)^-1       cost(v) = sum_p W_p lb_pp(v)   or the P values  W_p lb_pp(v)   (epgpy/stats.py:6-54)
//
// One lane per voxel: consecutive lanes read consecutive voxels of a row, 16 bytes each -- a wavefront reads whole 1 KiB lines.
// Per record a lane loads P complex128 values and adds Re(conj(a) b) = a_r b_r + a_i b_i to the P (P + 1) / 2 entries of the
// lower triangle (fp64 registers, two fma per entry); CRLB_UNROLL records are loaded before the first is used, so a lane keeps
// CRLB_UNROLL * P loads in flight.  HBM-bound: nrec * P * 16 bytes per voxel, every byte once.
//
// Long trains over few voxels (1000 TR, a few hundred voxels) would leave the device empty with one lane per voxel alone: the
// records of a voxel are cut into 1, 2, 4 or 8 slices (crlb_slices: by nrec ALONE), one wavefront of the block per slice; the
// partial triangles meet in LDS and the wavefront of slice 0 adds them in slice order.  No atomics: the association order of a
// voxel's sum depends on nrec only, so its bits do not depend on nvox, vox0 or its neighbours.
//
// The lane of slice 0 then scales by 1 / sigma2, takes the Cholesky factor L, inverts it (M = L^-1, lb_pp = sum_k M_kp^2),
// applies the weights and log10.  A pivot that is <= 0 or not finite makes every output of the voxel NaN (the reference:
// cond(I) > 1e30).  Everything is unrolled over the compile-time P: no scratch.  Plain vector stores only.
#include "epgx_stats.h"

namespace epgx {

template <int P>
__device__ __forceinline__ void crlb_add(double (&g)[P * (P + 1) / 2], const d2 (&x)[P]) {
    int i = 0;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q, ++i) {
            g[i] = fma(x[p].x, x[q].x, g[i]);
            g[i] = fma(x[p].y, x[q].y, g[i]);
        }
}

template <int P>
__global__ void __launch_bounds__(CRLB_MAX_SLICES * 64) crlb_kernel(const CrlbArgs a) {
    constexpr int NG = P * (P + 1) / 2;
    extern __shared__ double crlb_part[];      // [slices - 1][NG][groups * 64]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int groups = (int)(blockDim.x >> 6) / a.slices;
    const int grp = wave % groups, slice = wave / groups;
    const int64_t j = ((int64_t)blockIdx.x * groups + grp) * 64 + lane;
    const int64_t jc = j < a.nvox ? j : a.nvox - 1;     // lanes beyond the range read the last voxel and store nothing

    const int r0 = slice * a.slice_len;
    const int r1 = r0 + a.slice_len < a.nrec ? r0 + a.slice_len : a.nrec;
    const d2 *col[P];
#pragma unroll
    for (int c = 0; c < P; ++c) col[c] = a.signal + (int64_t)r0 * a.record_stride + a.rows[c] * a.row_stride + a.vox0 + jc;

    double g[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.0;

    int r = r0;
    for (; r + CRLB_UNROLL <= r1; r += CRLB_UNROLL) {
        d2 x[CRLB_UNROLL][P];
#pragma unroll
        for (int u = 0; u < CRLB_UNROLL; ++u)
#pragma unroll
            for (int c = 0; c < P; ++c) x[u][c] = col[c][u * a.record_stride];
#pragma unroll
        for (int c = 0; c < P; ++c) col[c] += CRLB_UNROLL * a.record_stride;
#pragma unroll
        for (int u = 0; u < CRLB_UNROLL; ++u) crlb_add<P>(g, x[u]);
    }
    for (; r < r1; ++r) {
        d2 x[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            x[c] = *col[c];
            col[c] += a.record_stride;
        }
        crlb_add<P>(g, x);
    }

    if (a.slices > 1) {      // (wave-uniform)
        const int width = groups * 64, at = grp * 64 + lane;
        if (slice > 0) {
#pragma unroll
            for (int i = 0; i < NG; ++i) crlb_part[((slice - 1) * NG + i) * width + at] = g[i];
        }
        __syncthreads();
        if (slice > 0) return;
        for (int s = 1; s < a.slices; ++s) {
#pragma unroll
            for (int i = 0; i < NG; ++i) g[i] += crlb_part[((s - 1) * NG + i) * width + at];
        }
    }
    if (j >= a.nvox) return;

    // I = G / sigma2 = L L^T
    double L[P][P];
    bool ok = true;
    {
        int i = 0;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int q = 0; q <= p; ++q, ++i) L[p][q] = g[i] * a.inv_sigma2;
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double d = L[q][q];
#pragma unroll
        for (int k = 0; k < q; ++k) d = fma(-L[q][k], L[q][k], d);
        ok = ok && d > 0.0 && __builtin_isfinite(d);
        const double piv = sqrt(d);
        L[q][q] = piv;
#pragma unroll
        for (int p = q + 1; p < P; ++p) {
            double s = L[p][q];
#pragma unroll
            for (int k = 0; k < q; ++k) s = fma(-L[p][k], L[q][k], s);
            L[p][q] = s / piv;
        }
    }
    // M = L^-1 (lower triangle), lb_pp = sum_{k >= p} M_kp^2
    double M[P][P], lb[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        M[q][q] = 1.0 / L[q][q];
#pragma unroll
        for (int p = q + 1; p < P; ++p) {
            double s = 0.0;
#pragma unroll
            for (int k = q; k < p; ++k) s = fma(L[p][k], M[k][q], s);
            M[p][q] = -s / L[p][p];
        }
        double acc = 0.0;
#pragma unroll
        for (int p = P - 1; p >= q; --p) acc = fma(M[p][q], M[p][q], acc);
        lb[q] = acc;
    }

    const double nan = __builtin_nan("");
    const bool lg = (a.flags & CRLB_FLAG_LOG10) != 0;
    if (a.flags & CRLB_FLAG_SPLIT) {
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double v = lb[c] * a.w[c];
            if (lg) v = log10(v);
            a.out[c * a.nvox + j] = ok ? v : nan;
        }
    } else {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) v = fma(a.w[c], lb[c], v);
        if (lg) v = log10(v);
        a.out[j] = ok ? v : nan;
    }
}

template <int P>
static hipError_t launch(hipStream_t stream, const CrlbArgs &a) {
    const int groups = crlb_voxel_groups(a.slices);
    const int64_t blocks = (a.nvox + groups * 64 - 1) / (groups * 64);
    const size_t lds = sizeof(double) * (size_t)(a.slices - 1) * (P * (P + 1) / 2) * groups * 64;
    hipLaunchKernelGGL(crlb_kernel<P>, dim3((unsigned)blocks), dim3((unsigned)(a.slices * groups * 64)), lds, stream, a);
    return hipGetLastError();
}

}  // namespace epgx

hipError_t epgx_launch_crlb(hipStream_t stream, int nparam, const epgx::CrlbArgs &a) {
    switch (nparam) {
    case 1: return epgx::launch<1>(stream, a);
    case 2: return epgx::launch<2>(stream, a);
    case 3: return epgx::launch<3>(stream, a);
    case 4: return epgx::launch<4>(stream, a);
    }
    return hipErrorInvalidValue;
}

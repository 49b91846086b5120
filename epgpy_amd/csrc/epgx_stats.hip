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
//
// crlb_grad_kernel (epgx_signal_crlb_grad) adds the gradient of the cost with respect to nx design variables, from second
// derivatives H that stay in HBM as well (epgpy/stats.py:31-33):
//      grad_x(v) = -2 / sigma2 * sum_ab S_ab G_x[a][b]      S = lb diag(W) lb      G_x[a][b] = sum_k Re( conj(H_kax) J_kb )
// G_x does not depend on lb, so the one pass over the records that sums the triangle sums G_x of CRLB_GRAD_XB design variables
// too (P^2 fp64 registers each); one launch per chunk of CRLB_GRAD_XB variables, each of which reads J again.  Where a lane
// stands (crlb_lane), the triangle's sum (crlb_add), the meeting of the slices (crlb_meet) and the factorisation (crlb_invert)
// are the functions crlb_kernel is made of: the cost of crlb_grad_kernel has the bits of crlb_kernel's.
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

// where a lane stands: its voxel (j; jc clamped into the range -- lanes beyond it read the last voxel and store nothing),
// its slice [r0, r1) of the records, and its place `at` in a row of `width` partial sums
struct CrlbLane {
    int slice, width, at, r0, r1;
    int64_t j, jc;
};

__device__ __forceinline__ CrlbLane crlb_lane(const CrlbArgs &a) {
    CrlbLane l;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int groups = (int)(blockDim.x >> 6) / a.slices;
    const int grp = wave % groups;
    l.slice = wave / groups;
    l.j = ((int64_t)blockIdx.x * groups + grp) * 64 + lane;
    l.jc = l.j < a.nvox ? l.j : a.nvox - 1;
    l.r0 = l.slice * a.slice_len;
    l.r1 = l.r0 + a.slice_len < a.nrec ? l.r0 + a.slice_len : a.nrec;
    l.width = groups * 64;
    l.at = grp * 64 + lane;
    return l;
}

// the N partial sums of slices 1 .. slices - 1 meet in LDS (part [slices - 1][N][width]); the wavefront of slice 0 adds them
// in slice order.  Block-wide (a barrier inside); only the lanes of slice 0 hold the sums afterwards.  A second meeting
// through the same `part` needs a barrier of its own in between.
template <int N>
__device__ __forceinline__ void crlb_meet(double (&g)[N], double *part, const CrlbLane &l, int slices) {
    if (l.slice > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[((l.slice - 1) * N + i) * l.width + l.at] = g[i];
    }
    __syncthreads();
    if (l.slice > 0) return;
    for (int s = 1; s < slices; ++s) {
#pragma unroll
        for (int i = 0; i < N; ++i) g[i] += part[((s - 1) * N + i) * l.width + l.at];
    }
}

// I = G / sigma2 = L L^T;  M = L^-1 (lower triangle), lb_pp = sum_{k >= p} M_kp^2.  false: a pivot <= 0 or not finite
template <int P>
__device__ __forceinline__ bool crlb_invert(const double (&g)[P * (P + 1) / 2], double inv_sigma2, double (&M)[P][P], double (&lb)[P]) {
    double L[P][P];
    bool ok = true;
    {
        int i = 0;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int q = 0; q <= p; ++q, ++i) L[p][q] = g[i] * inv_sigma2;
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
    return ok;
}

// sum_p W_p lb_pp, the cost before log10
template <int P>
__device__ __forceinline__ double crlb_cost(const CrlbArgs &a, const double (&lb)[P]) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < P; ++c) v = fma(a.w[c], lb[c], v);
    return v;
}

template <int P>
__global__ void __launch_bounds__(CRLB_MAX_SLICES * 64) crlb_kernel(const CrlbArgs a) {
    constexpr int NG = P * (P + 1) / 2;
    extern __shared__ double crlb_part[];      // [slices - 1][NG][groups * 64]
    const CrlbLane l = crlb_lane(a);

    const d2 *col[P];
#pragma unroll
    for (int c = 0; c < P; ++c) col[c] = a.signal + (int64_t)l.r0 * a.record_stride + a.rows[c] * a.row_stride + a.vox0 + l.jc;

    double g[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.0;

    int r = l.r0;
    for (; r + CRLB_UNROLL <= l.r1; r += CRLB_UNROLL) {
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
    for (; r < l.r1; ++r) {
        d2 x[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            x[c] = *col[c];
            col[c] += a.record_stride;
        }
        crlb_add<P>(g, x);
    }

    if (a.slices > 1) {      // (wave-uniform)
        crlb_meet<NG>(g, crlb_part, l, a.slices);
        if (l.slice > 0) return;
    }
    if (l.j >= a.nvox) return;

    double M[P][P], lb[P];
    const bool ok = crlb_invert<P>(g, a.inv_sigma2, M, lb);

    const double nan = __builtin_nan("");
    const bool lg = (a.flags & CRLB_FLAG_LOG10) != 0;
    if (a.flags & CRLB_FLAG_SPLIT) {
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double v = lb[c] * a.w[c];
            if (lg) v = log10(v);
            a.out[c * a.nvox + l.j] = ok ? v : nan;
        }
    } else {
        double v = crlb_cost<P>(a, lb);
        if (lg) v = log10(v);
        a.out[l.j] = ok ? v : nan;
    }
}

// One chunk of h.nx <= CRLB_GRAD_XB design variables.  The records are summed one at a time: P + nx * P loads of 16 bytes
// are in flight per record, and the triangle's sum has the order of crlb_kernel's (record by record inside a slice).
// Entries of H that are identically zero (off < 0) and the variables beyond h.nx are not read: wave-uniform branches
// around the loads, the value 0 in their place.
template <int P>
__global__ void __launch_bounds__(CRLB_MAX_SLICES * 64) crlb_grad_kernel(const CrlbArgs a, const CrlbGradArgs h) {
    constexpr int NG = P * (P + 1) / 2, NH = P * P, XB = CRLB_GRAD_XB;
    extern __shared__ double crlb_part[];      // [slices - 1][max(NG, NH) = NH][groups * 64], one meeting after the other
    const CrlbLane l = crlb_lane(a);

    const d2 *col[P];
#pragma unroll
    for (int c = 0; c < P; ++c) col[c] = a.signal + (int64_t)l.r0 * a.record_stride + a.rows[c] * a.row_stride + a.vox0 + l.jc;
    const d2 *hvox = h.hess + a.vox0 + l.jc;

    double g[NG], G[XB][NH];
#pragma unroll
    for (int i = 0; i < NG; ++i) g[i] = 0.0;
#pragma unroll
    for (int x = 0; x < XB; ++x)
#pragma unroll
        for (int i = 0; i < NH; ++i) G[x][i] = 0.0;

    for (int r = l.r0; r < l.r1; ++r) {
        d2 jx[P], hx[XB][P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            jx[c] = *col[c];
            col[c] += a.record_stride;
        }
#pragma unroll
        for (int x = 0; x < XB; ++x)
#pragma unroll
            for (int c = 0; c < P; ++c) {
                hx[x][c] = d2{0.0, 0.0};
                if (x < h.nx && h.off[x][c] >= 0) hx[x][c] = hvox[h.off[x][c] + (int64_t)r * h.stride[x][c]];      // (wave-uniform)
            }
        crlb_add<P>(g, jx);
#pragma unroll
        for (int x = 0; x < XB; ++x)
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    G[x][p * P + q] = fma(hx[x][p].x, jx[q].x, G[x][p * P + q]);
                    G[x][p * P + q] = fma(hx[x][p].y, jx[q].y, G[x][p * P + q]);
                }
    }

    if (a.slices > 1) {      // (wave-uniform)
        crlb_meet<NG>(g, crlb_part, l, a.slices);
#pragma unroll
        for (int x = 0; x < XB; ++x) {
            __syncthreads();
            crlb_meet<NH>(G[x], crlb_part, l, a.slices);
        }
        if (l.slice > 0) return;
    }
    if (l.j >= a.nvox) return;

    double M[P][P], lb[P];
    const bool ok = crlb_invert<P>(g, a.inv_sigma2, M, lb);
    const double cost = crlb_cost<P>(a, lb);

    // lbw = lb diag(W) with lb = M^T M (M lower triangular), then S = lbw lb
    double full[P][P], S[P][P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        full[p][p] = lb[p];
#pragma unroll
        for (int q = 0; q < p; ++q) {
            double acc = 0.0;
#pragma unroll
            for (int k = P - 1; k >= p; --k) acc = fma(M[k][p], M[k][q], acc);
            full[p][q] = full[q][p] = acc;
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < P; ++q) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc = fma(full[p][k] * a.w[k], full[k][q], acc);
            S[p][q] = acc;
        }

    const double nan = __builtin_nan("");
    const bool lg = (a.flags & CRLB_FLAG_LOG10) != 0;
    // d log10(c) = dc / (c ln 10)
    const double scale = lg ? -2.0 * a.inv_sigma2 / (cost * 2.302585092994045684) : -2.0 * a.inv_sigma2;
    if (h.write_cost) a.out[l.j] = ok ? (lg ? log10(cost) : cost) : nan;
#pragma unroll
    for (int x = 0; x < XB; ++x) {
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int q = 0; q < P; ++q) acc = fma(S[p][q], G[x][p * P + q], acc);
        if (x < h.nx) h.grad[x * a.nvox + l.j] = ok ? scale * acc : nan;
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

template <int P>
static hipError_t launch_grad(hipStream_t stream, const CrlbArgs &a, const CrlbGradArgs &h) {
    const int groups = crlb_voxel_groups(a.slices);
    const int64_t blocks = (a.nvox + groups * 64 - 1) / (groups * 64);
    const size_t lds = sizeof(double) * (size_t)(a.slices - 1) * (P * P) * groups * 64;      // <= 7 * 16 * 64 * 8 = 56 KiB
    hipLaunchKernelGGL(crlb_grad_kernel<P>, dim3((unsigned)blocks), dim3((unsigned)(a.slices * groups * 64)), lds, stream, a, h);
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

hipError_t epgx_launch_crlb_grad(hipStream_t stream, int nparam, const epgx::CrlbArgs &a, const epgx::CrlbGradArgs &h) {
    switch (nparam) {
    case 1: return epgx::launch_grad<1>(stream, a, h);
    case 2: return epgx::launch_grad<2>(stream, a, h);
    case 3: return epgx::launch_grad<3>(stream, a, h);
    case 4: return epgx::launch_grad<4>(stream, a, h);
    }
    return hipErrorInvalidValue;
}

// epgx_refine.hip -- one variable-projection Gauss-Newton step off the grid, from a dictionary and its Jacobian that stay in HBM
// (include/epgx.h epgx_signal_refine).  For measured voxel m with atom a = index[m], d_t = D[t,a], j_pt = J_p[t,a], s_t = S[t,m]:
//      n = sum |d|^2    E = sum |s|^2    c = sum conj(d) s    b_p = sum conj(j_p) s    h_p = sum conj(d) j_p    M_pq = sum conj(j_p) j_q
// of which only Re M_pq enters the formulas of the header: 4 + 4 P + P (P + 1) / 2 fp64 sums per lane, 30 for P = 4.
//
// One lane per measured voxel.  Per record a lane gathers 1 + P values of 16 bytes from the columns of its atom (neighbouring
// lanes hold unrelated atoms: every gather touches a line of its own) and loads S[t,m] coalesced; REFINE_UNROLL records are
// loaded before the first is used.  Lanes whose index lies outside [0, natoms), and the lanes beyond nmeas, load nothing.
//
// The records of a voxel are cut into 1, 2, 4 or 8 slices (refine_slices: by nrec ALONE), one wavefront of the block per slice;
// the partial sums meet in LDS, REFINE_MEET of them at a time, and the wavefront of slice 0 adds them in ascending slice order.
// No atomics: the association order of a voxel's sums depends on nrec only, so its bits do not depend on nmeas, on its place in
// the call or on its neighbours.
//
// The lane of slice 0 then forms the projected normal equations, equilibrates them by the unprojected column norms, factors
// (Cholesky, pivots in [0, 1] against rcond), solves, clips and evaluates scale' and score' of the linearised atom.  Everything
// is unrolled over the compile-time P: no scratch.  Plain vector stores only.
#include "epgx_refine.h"

namespace epgx {

template <int P>
__device__ __forceinline__ void refine_add(double (&g)[refine_sums(P)], d2 d, d2 s, const d2 (&x)[P]) {
    g[0] = fma(d.x, d.x, g[0]);
    g[0] = fma(d.y, d.y, g[0]);
    g[1] = fma(s.x, s.x, g[1]);
    g[1] = fma(s.y, s.y, g[1]);
    g[2] = fma(d.x, s.x, g[2]);
    g[2] = fma(d.y, s.y, g[2]);
    g[3] = fma(d.x, s.y, g[3]);
    g[3] = fma(-d.y, s.x, g[3]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double *b = &g[4 + 2 * p], *h = &g[4 + 2 * P + 2 * p];
        b[0] = fma(x[p].x, s.x, b[0]);
        b[0] = fma(x[p].y, s.y, b[0]);
        b[1] = fma(x[p].x, s.y, b[1]);
        b[1] = fma(-x[p].y, s.x, b[1]);
        h[0] = fma(d.x, x[p].x, h[0]);
        h[0] = fma(d.y, x[p].y, h[0]);
        h[1] = fma(d.x, x[p].y, h[1]);
        h[1] = fma(-d.y, x[p].x, h[1]);
    }
    int i = 4 + 4 * P;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q, ++i) {
            g[i] = fma(x[p].x, x[q].x, g[i]);
            g[i] = fma(x[p].y, x[q].y, g[i]);
        }
}

// the N partial sums of slices 1 .. slices - 1 meet in LDS, REFINE_MEET at a time (part [slices - 1][REFINE_MEET][width]); the
// wavefront of slice 0 adds them in slice order.  Block-wide (barriers inside); only the lanes of slice 0 hold the sums afterwards
template <int N>
__device__ __forceinline__ void refine_meet(double (&g)[N], double *part, int slice, int slices, int width, int at) {
#pragma unroll
    for (int i0 = 0; i0 < N; i0 += REFINE_MEET) {
        if (i0 > 0) __syncthreads();      // (the round before has been read)
        if (slice > 0) {
#pragma unroll
            for (int i = i0; i < i0 + REFINE_MEET && i < N; ++i) part[((slice - 1) * REFINE_MEET + (i - i0)) * width + at] = g[i];
        }
        __syncthreads();
        if (slice == 0) {
            for (int s = 1; s < slices; ++s) {
#pragma unroll
                for (int i = i0; i < i0 + REFINE_MEET && i < N; ++i) g[i] += part[((s - 1) * REFINE_MEET + (i - i0)) * width + at];
            }
        }
    }
}

template <int P>
__global__ void __launch_bounds__(REFINE_MAX_SLICES * 64) refine_kernel(const RefineArgs a) {
    constexpr int N = refine_sums(P);
    extern __shared__ double refine_part[];      // [slices - 1][REFINE_MEET][groups * 64]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int groups = (int)(blockDim.x >> 6) / a.slices;
    const int grp = wave % groups, slice = wave / groups;
    const int64_t m = ((int64_t)blockIdx.x * groups + grp) * 64 + lane;
    const int r0 = slice * a.slice_len;
    const int r1 = r0 + a.slice_len < a.nrec ? r0 + a.slice_len : a.nrec;

    int64_t atom = -1;
    if (m < a.nmeas) atom = a.index[m];
    const bool valid = atom >= 0 && atom < a.natoms;

    double g[N];
#pragma unroll
    for (int i = 0; i < N; ++i) g[i] = 0.0;

    if (valid) {
        const d2 *dcol = a.jac + atom, *scol = a.sig + m;
        const d2 *jcol[P];
#pragma unroll
        for (int c = 0; c < P; ++c) jcol[c] = dcol + a.rows[c] * a.row_stride;
        int r = r0;
        for (; r + REFINE_UNROLL <= r1; r += REFINE_UNROLL) {
            d2 d[REFINE_UNROLL], s[REFINE_UNROLL], x[REFINE_UNROLL][P];
#pragma unroll
            for (int u = 0; u < REFINE_UNROLL; ++u) {
                const int64_t at = (int64_t)(r + u) * a.record_stride;
                d[u] = dcol[at];
#pragma unroll
                for (int c = 0; c < P; ++c) x[u][c] = jcol[c][at];
                s[u] = scol[(int64_t)(r + u) * a.sig_stride];
            }
#pragma unroll
            for (int u = 0; u < REFINE_UNROLL; ++u) refine_add<P>(g, d[u], s[u], x[u]);
        }
        for (; r < r1; ++r) {
            const int64_t at = (int64_t)r * a.record_stride;
            d2 x[P];
            const d2 d = dcol[at];
#pragma unroll
            for (int c = 0; c < P; ++c) x[c] = jcol[c][at];
            refine_add<P>(g, d, scol[(int64_t)r * a.sig_stride], x);
        }
    }

    if (a.slices > 1) {      // (block-uniform)
        refine_meet<N>(g, refine_part, slice, a.slices, groups * 64, grp * 64 + lane);
        if (slice > 0) return;
    }
    if (m >= a.nmeas) return;

    const double nan = __builtin_nan("");
    if (!valid) {
#pragma unroll
        for (int p = 0; p < P; ++p) a.delta[p * a.nmeas + m] = nan;
        a.scale[m] = d2{0.0, 0.0};
        a.score[m] = 0.0;
        return;
    }

    const double n = g[0], E = g[1];
    const d2 c = d2{g[2], g[3]};
    const double *b = &g[4], *h = &g[4 + 2 * P], *M = &g[4 + 4 * P];      // M: lower triangle, entry (p, q <= p) at p (p + 1) / 2 + q
    const d2 rho = d2{c.x / n, c.y / n};
    const double rho2 = fma(rho.x, rho.x, rho.y * rho.y);
    const double root_e = sqrt(E);
    const double score0 = E == 0.0 ? 0.0 : sqrt(fma(c.x, c.x, c.y * c.y)) / (sqrt(n) * root_e);
    // |rho|^2 = 0 (or not finite) makes every pivot of N / |rho|^2 the quotient 0 / 0: not finite
    bool ok = n > 0.0 && __builtin_isfinite(n) && rho2 > 0.0 && __builtin_isfinite(rho2);

    double sd[P], L[P][P], z[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double mpp = M[p * (p + 1) / 2 + p];
        ok = ok && mpp > 0.0 && __builtin_isfinite(mpp);
        sd[p] = sqrt(mpp);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int q = 0; q <= p; ++q) {
            const double hh = fma(h[2 * p], h[2 * q], h[2 * p + 1] * h[2 * q + 1]);      // Re(conj(h_p) h_q)
            L[p][q] = (M[p * (p + 1) / 2 + q] - hh / n) / (sd[p] * sd[q]);
        }
        // t = b_p - rho conj(h_p),  y_p = Re(conj(rho) t)
        const double tx = b[2 * p] - fma(rho.x, h[2 * p], rho.y * h[2 * p + 1]);
        const double ty = b[2 * p + 1] - fma(rho.y, h[2 * p], -rho.x * h[2 * p + 1]);
        z[p] = fma(rho.x, tx, rho.y * ty) / (rho2 * sd[p]);
    }
    // Nhat = L L^T in place; a pivot <= rcond or not finite: unresolved
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double piv = L[q][q];
#pragma unroll
        for (int k = 0; k < q; ++k) piv = fma(-L[q][k], L[q][k], piv);
        ok = ok && piv > a.rcond && __builtin_isfinite(piv);
        const double root = sqrt(piv);
        L[q][q] = root;
#pragma unroll
        for (int p = q + 1; p < P; ++p) {
            double v = L[p][q];
#pragma unroll
            for (int k = 0; k < q; ++k) v = fma(-L[p][k], L[q][k], v);
            L[p][q] = v / root;
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {      // L w = z
        double v = z[p];
#pragma unroll
        for (int k = 0; k < p; ++k) v = fma(-L[p][k], z[k], v);
        z[p] = v / L[p][p];
    }
    double delta[P];
#pragma unroll
    for (int p = P - 1; p >= 0; --p) {      // L^T x = w,  delta_p = x_p / sqrt(M_pp)
        double v = z[p];
#pragma unroll
        for (int k = p + 1; k < P; ++k) v = fma(-L[k][p], z[k], v);
        z[p] = v / L[p][p];
        double dp = z[p] / sd[p];
        if (dp > a.limit[p]) dp = a.limit[p];
        if (dp < -a.limit[p]) dp = -a.limit[p];
        delta[p] = dp;
    }

    if (!ok) {
#pragma unroll
        for (int p = 0; p < P; ++p) a.delta[p * a.nmeas + m] = nan;
        a.scale[m] = rho;
        a.score[m] = score0;
        return;
    }
    d2 num = c;
    double den = n;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        num.x = fma(delta[p], b[2 * p], num.x);
        num.y = fma(delta[p], b[2 * p + 1], num.y);
        den = fma(2.0 * delta[p], h[2 * p], den);
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) den = fma((p == q ? 1.0 : 2.0) * delta[p] * delta[q], M[p * (p + 1) / 2 + q], den);
#pragma unroll
    for (int p = 0; p < P; ++p) a.delta[p * a.nmeas + m] = delta[p];
    a.scale[m] = d2{num.x / den, num.y / den};
    a.score[m] = E == 0.0 ? 0.0 : sqrt(fma(num.x, num.x, num.y * num.y)) / (sqrt(den) * root_e);
}

template <int P>
static hipError_t launch(hipStream_t stream, const RefineArgs &a) {
    const int groups = refine_voxel_groups(a.slices);
    const int64_t blocks = (a.nmeas + groups * 64 - 1) / (groups * 64);
    const size_t lds = sizeof(double) * (size_t)(a.slices - 1) * REFINE_MEET * groups * 64;      // <= 7 * 8 * 64 * 8 = 28 KiB
    hipLaunchKernelGGL(refine_kernel<P>, dim3((unsigned)blocks), dim3((unsigned)(a.slices * groups * 64)), lds, stream, a);
    return hipGetLastError();
}

}  // namespace epgx

hipError_t epgx_launch_refine(hipStream_t stream, int nparam, const epgx::RefineArgs &a) {
    switch (nparam) {
    case 1: return epgx::launch<1>(stream, a);
    case 2: return epgx::launch<2>(stream, a);
    case 3: return epgx::launch<3>(stream, a);
    case 4: return epgx::launch<4>(stream, a);
    }
    return hipErrorInvalidValue;
}

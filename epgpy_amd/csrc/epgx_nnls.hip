// epgx_nnls.hip -- non-negative mixtures of the atoms along one grid axis of a dictionary that stays in HBM (include/epgx.h
// epgx_signal_component_gram, epgx_signal_nnls).  With D[t,a,g] (records t, atoms a < A <= 64 of the component axis, groups g) and
// S[t,m]:
//      H_g[a,b] = Re sum_t conj(D[t,a,g]) D[t,b,g]      f[a] = Re sum_t conj(D[t,a,g]) S[t,m]      E = sum_t |S[t,m]|^2
//      x* = argmin over x >= 0 of  x^T (H_g + mu_g I) x - 2 f^T x + E,      mu_g = reg * mean over the valid atoms of H_g[a,a]
//
// component_gram_kernel: one block per group; every entry of H_g is one sequential sum over the records (so H_g is symmetric to
// the bit), and the first wavefront votes the validity mask.
//
// nnls_kernel: Lawson and Hanson's active set on the Gram form, ONE WAVEFRONT PER VOXEL, lane a owning atom a: f_a, w_a, the
// threshold and the position of the atom in the passive set stay in registers.  The same lanes, counted as POSITIONS 0 .. k - 1 of
// the passive set in the order the atoms entered, hold the atom at each position, its weight and the inverse diagonal of the
// Cholesky factor of (H_g + mu_g I)[P,P]; the strict lower triangle of the factor lies in LDS, one per wavefront, and grows by one
// row when an atom enters.  When atoms leave, the rows from the first vacated position on are rebuilt.  A passive-set solve is a
// forward and a backward substitution of k steps each: the pivot lane's value goes round by v_readlane and every later lane
// takes one fused multiply-add against a column (forward) or a row (backward) of the factor.
// The block stages H_g in LDS once per group.  In the group search the 4 wavefronts of a block (4 voxels) walk the groups together,
// in ascending order, and each keeps the best group so far in registers: J < best replaces, so the lowest g wins among equal J
// and nothing depends on the order in which anything finishes.  With fixed groups a block is one wavefront and stages the H_g of
// its voxel.  No atomics; every sum runs in a fixed order (records ascending, passive positions ascending, atoms ascending) that
// depends on the voxel's own data alone, so a voxel's bits do not depend on the other voxels or on the launch.  Plain vector stores.
#include "epgx_nnls_active.hip.h"

namespace epgx {

__global__ void __launch_bounds__(NNLS_WAVES * 64) nnls_kernel(const NnlsArgs a) {
    extern __shared__ double nnls_lds[];
    const int A = a.c.ncomp;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)(blockDim.x >> 6);
    double *Hs = nnls_lds;                                                     // [A][A]
    double *Lw = Hs + A * A + wave * (A * (A - 1) / 2);                        // this wavefront's factor
    int *tmp = (int *)(Hs + A * A + waves * (A * (A - 1) / 2)) + wave * 64;    // this wavefront's scratch
    const int64_t m = (int64_t)blockIdx.x * waves + wave;
    const bool live = m < a.nmeas;
    const int64_t G = a.c.nouter * a.c.ninner;
    const int cap = 3 * A;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    int64_t g0 = 0, g1 = G;
    if (a.group) {      // (a block is one wavefront)
        const int64_t g = live ? a.group[m] : -1;
        g0 = g >= 0 && g < G ? g : 0;
        g1 = g >= 0 && g < G ? g + 1 : 0;
    }

    const double E = live && g1 > g0 ? nnls_energy(a.sig, a.sig_stride, a.c.nrec, m) : 0.0;

    double best_j = inf, best_x = nan, best_res = nan;
    int64_t best_g = -1;
    int best_status = 2;

    for (int64_t g = g0; g < g1; ++g) {
        __syncthreads();      // (the H of the group before has been read)
        for (int idx = threadIdx.x; idx < A * A; idx += blockDim.x) Hs[idx] = a.gram[g * A * A + idx];
        __syncthreads();
        if (!live) continue;

        const unsigned long long mask = a.mask[g];
        const bool valid = lane < A && ((mask >> lane) & 1ull);
        const double diag = valid ? Hs[lane * A + lane] : 0.0;
        const double mu = nnls_ridge(Hs, A, mask, a.reg);
        const double f = nnls_project(a.c, a.sig, a.sig_stride, m, g, valid, lane);

        int status = 0;
        if (!__builtin_isfinite(E) || __ballot(valid && !__builtin_isfinite(f))) status = 2;
        const double thr = a.tol * sqrt(diag * E);

        double xa, J, n2;
        status = nnls_active_set(Hs, Lw, tmp, A, lane, valid, f, E, thr, mu, cap, status, xa, J, n2);
        if (status == 2) continue;
        if (J < best_j) {
            const double data = fma(-mu, n2, J);
            best_j = J;
            best_g = g;
            best_x = xa;
            best_res = sqrt(data > 0.0 ? data : 0.0);
            best_status = status;
        }
    }

    if (!live) return;
    if (lane < A) a.weights[(int64_t)lane * a.nmeas + m] = best_x;
    if (lane == 0) {
        a.out_group[m] = best_g;
        a.residual[m] = best_res;
        a.status[m] = best_status;
    }
}

__global__ void __launch_bounds__(NNLS_GRAM_THREADS) component_gram_kernel(const ComponentGramArgs a) {
    const int A = a.c.ncomp;
    const int64_t g = blockIdx.x;
    const d2 *base = a.c.dict + (g / a.c.ninner) * A * a.c.axis_stride + g % a.c.ninner;
    for (int idx = threadIdx.x; idx < A * A; idx += NNLS_GRAM_THREADS) {
        const d2 *ca = base + (idx / A) * a.c.axis_stride, *cb = base + (idx % A) * a.c.axis_stride;
        double h = 0.0;
        for (int t = 0; t < a.c.nrec; ++t) {
            const d2 x = ca[(int64_t)t * a.c.row_stride], y = cb[(int64_t)t * a.c.row_stride];
            h = fma(x.x, y.x, h);      // (the same bits for (a, b) and (b, a))
            h = fma(x.y, y.y, h);
        }
        a.gram[g * A * A + idx] = h;
    }
    if (threadIdx.x < 64) {      // the first wavefront: the diagonal once more, by the same sums, and the vote
        const int lane = threadIdx.x;
        double n = 0.0;
        if (lane < A) {
            const d2 *ca = base + lane * a.c.axis_stride;
            for (int t = 0; t < a.c.nrec; ++t) {
                const d2 x = ca[(int64_t)t * a.c.row_stride];
                n = fma(x.x, x.x, n);
                n = fma(x.y, x.y, n);
            }
        }
        const unsigned long long ok = __ballot(lane < A && n > 0.0 && __builtin_isfinite(n));
        if (lane == 0) a.mask[g] = ok;
    }
}

}  // namespace epgx

hipError_t epgx_launch_component_gram(hipStream_t stream, const epgx::ComponentGramArgs &a) {
    const int64_t G = a.c.nouter * a.c.ninner;
    hipLaunchKernelGGL(epgx::component_gram_kernel, dim3((unsigned)G), dim3(epgx::NNLS_GRAM_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_nnls(hipStream_t stream, const epgx::NnlsArgs &a) {
    const int waves = a.group ? 1 : epgx::NNLS_WAVES;
    const int64_t blocks = (a.nmeas + waves - 1) / waves;
    const size_t lds = epgx::nnls_lds_bytes(a.c.ncomp, waves);
    if (lds > 160 * 1024) return hipErrorInvalidValue;      // (A <= 64: 95.5 KiB at most)
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)epgx::nnls_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(epgx::nnls_kernel, dim3((unsigned)blocks), dim3((unsigned)(waves * 64)), lds, stream, a);
    return hipGetLastError();
}

// epgx_nnls_chi2.hip -- the chi^2-driven ridge of the non-negative mixtures (include/epgx.h epgx_signal_nnls_chi2): per voxel, in the
// group that the unregularised fit chose, the ridge mu >= mu_0 at which the data misfit Jd(mu) = J - mu |x|^2 has grown to
// chi2 * Jd(mu_0), and the smooth weights there.
//
// nnls_chi2_kernel runs behind nnls_kernel (or alone, with the caller's groups): ONE WAVEFRONT AND ONE BLOCK PER VOXEL, lane a
// owning atom a, H_g of the voxel's group staged in LDS once, the factor in the wavefront's triangle -- the layout of nnls_kernel's
// fixed-group form.  Every evaluation of Jd(mu) is one cold call of nnls_active_set (epgx_nnls_active.hip.h), the same code as
// nnls_kernel's fit: the factor is rebuilt since the diagonal changed.  The search state (the two ends of the bracket, their
// misfits, the best point so far) is wave-uniform: every lane computes it from values that readlane / the ordered sums made
// uniform, and every branch of the search is taken on a readfirstlane of its condition.
//   1. mu_0 = reg * mean valid H_aa; x_0, Jd_0 its fit (status 1 and 2 of that fit pass through, nothing is searched)
//   2. Jd_0 <= 0 or Jd_0 < 32 (nrec + A) 2^-53 E / rtol: status 4.   T = chi2 Jd_0; |Jd_0 / T - 1| <= rtol: status 0 at mu_0.
//      T >= E or mu_0 = 0: status 3 at mu_0
//   3. mu = 16 mu_lo while Jd(mu) < T (the bracket), then Illinois regula falsi in log mu on r(mu) = Jd(mu) / T - 1 between the
//      ends; |r| <= rtol ends it with status 0; max_evals fits, a fit that is not status 0 or a mu that is not finite end it with
//      status 3 at the evaluated point of the largest Jd <= T
// No atomics; the sums are those of nnls_active_set; a voxel's bits depend on its own signal, the dictionary and the arguments
// only (a block is a voxel, so the launch has no shape to depend on).  Plain vector stores.
#include "epgx_nnls_active.hip.h"

namespace epgx {

// a wave-uniform condition as a scalar: the branch on it is uniform for the compiler too
__device__ __forceinline__ bool nnls_uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

__global__ void __launch_bounds__(64) nnls_chi2_kernel(const NnlsChi2Args a) {
    extern __shared__ double nnls_lds[];
    const NnlsArgs &n = a.n;
    const int A = n.c.ncomp;
    const int lane = threadIdx.x;
    double *Hs = nnls_lds;                       // [A][A]
    double *Lw = Hs + A * A;                     // the factor
    int *tmp = (int *)(Lw + A * (A - 1) / 2);    // scratch of the compactions
    const int64_t m = blockIdx.x;
    const int64_t G = n.c.nouter * n.c.ninner;
    const int cap = 3 * A;
    const double nan = __builtin_nan("");

    double out_x = nan, out_res = nan, out_mu = nan, out_ratio = nan;
    int64_t out_g = -1;
    int out_status = 2, evals = 0;

    const int64_t g = n.group[m];
    if (g >= 0 && g < G) {
        for (int idx = lane; idx < A * A; idx += 64) Hs[idx] = n.gram[g * A * A + idx];
        __syncthreads();
        const double E = nnls_energy(n.sig, n.sig_stride, n.c.nrec, m);
        const unsigned long long mask = n.mask[g];
        const bool valid = lane < A && ((mask >> lane) & 1ull);
        const double diag = valid ? Hs[lane * A + lane] : 0.0;
        const double mu0 = nnls_ridge(Hs, A, mask, n.reg);
        const double f = nnls_project(n.c, n.sig, n.sig_stride, m, g, valid, lane);
        int status = 0;
        if (!__builtin_isfinite(E) || __ballot(valid && !__builtin_isfinite(f))) status = 2;
        const double thr = n.tol * sqrt(diag * E);

        double xa, J, n2;
        status = nnls_active_set(Hs, Lw, tmp, A, lane, valid, f, E, thr, mu0, cap, status, xa, J, n2);
        if (status != 2) {
            const double Jd0 = fma(-mu0, n2, J);
            out_x = xa;
            out_g = g;
            out_res = sqrt(Jd0 > 0.0 ? Jd0 : 0.0);
            out_status = status;
            out_mu = mu0;
            out_ratio = 1.0;
            const double T = a.chi2 * Jd0;
            const double floor = 32.0 * (double)(n.c.nrec + A) * 0x1p-53 * E / a.rtol;
            if (status != 0) {
                // the cap of the unregularised fit passes through
            } else if (nnls_uniform(!(Jd0 > 0.0) || Jd0 < floor)) {
                out_status = 4;
            } else if (nnls_uniform(fabs(Jd0 / T - 1.0) <= a.rtol)) {
                // met where it stands
            } else if (nnls_uniform(!(T < E) || !(mu0 > 0.0))) {
                out_status = 3;
            } else {
                out_status = 3;
                double mu_lo = mu0, r_lo = Jd0 / T - 1.0, mu_hi = 0.0, r_hi = 0.0, best = Jd0;
                bool bracket = false;
                int side = 0;      // the end that the last evaluation replaced, once there is a bracket: -1 lo, +1 hi
                while (evals < a.max_evals) {
                    double mu = mu_lo * NNLS_CHI2_FACTOR;
                    if (bracket) mu = mu_lo * exp(r_lo / (r_lo - r_hi) * log(mu_hi / mu_lo));
                    if (nnls_uniform(!__builtin_isfinite(mu))) break;
                    ++evals;
                    nnls_wave_sync();      // (the factor of the evaluation before has been read)
                    status = nnls_active_set(Hs, Lw, tmp, A, lane, valid, f, E, thr, mu, cap, 0, xa, J, n2);
                    if (status != 0) break;
                    const double Jd = fma(-mu, n2, J);
                    const double r = Jd / T - 1.0;
                    const bool hit = nnls_uniform(fabs(r) <= a.rtol);
                    if (hit || nnls_uniform(r < 0.0 && Jd > best)) {
                        best = Jd;
                        out_x = xa;
                        out_res = sqrt(Jd > 0.0 ? Jd : 0.0);
                        out_mu = mu;
                        out_ratio = Jd / Jd0;
                    }
                    if (hit) {
                        out_status = 0;
                        break;
                    }
                    if (nnls_uniform(r < 0.0)) {
                        mu_lo = mu;
                        r_lo = r;
                        if (bracket) {
                            if (side < 0) r_hi *= 0.5;
                            side = -1;
                        }
                    } else {
                        mu_hi = mu;
                        r_hi = r;
                        if (bracket && side > 0) r_lo *= 0.5;
                        bracket = true;
                        side = 1;
                    }
                }
            }
        }
    }

    if (lane < A) n.weights[(int64_t)lane * n.nmeas + m] = out_x;
    if (lane == 0) {
        n.out_group[m] = out_g;
        n.residual[m] = out_res;
        n.status[m] = out_status;
        a.mu[m] = out_mu;
        a.ratio[m] = out_ratio;
        a.evals[m] = evals;
    }
}

}  // namespace epgx

hipError_t epgx_launch_nnls_chi2(hipStream_t stream, const epgx::NnlsChi2Args &a) {
    const size_t lds = epgx::nnls_lds_bytes(a.n.c.ncomp, 1);      // 47.8 KiB at A = 64
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(epgx::nnls_chi2_kernel, dim3((unsigned)a.n.nmeas), dim3(64), lds, stream, a);
    return hipGetLastError();
}

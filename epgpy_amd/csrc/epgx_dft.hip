// epgx_dft.hip -- spatial read-out of a device-resident state matrix (include/epgx.h epgx_state_dft):
//      im[v][p] = phase * sum_r  w_r F_r(v) exp(i k_r . x_p)                      (epgpy/utils.py:12-115, probe.py:168-219)
//
// The state stores the half representation A_j = F_k, B_j = conj(F_-k) (j = 0 .. nrow-1); row -k carries the wavenumber -k_j and
// the same voxel factor (sinc is even), so the 2 n + 1 rows fold onto the stored orders.  With c + i s = exp(i k_j . x_p):
//      Re im = sum_j  P_j c - Q_j s        P = w (a_r + b_r)   Q = w (a_i + b_i)
//      Im im = sum_j  R_j s + S_j c        R = w (a_r - b_r)   S = w (a_i - b_i)         (j = 0: A_0 alone, b = 0)
// four multiply-adds per (voxel, stored order, position): a real [2 nvox x 2 nrow] . [2 nrow x npos] product whose right-hand
// side is generated here.
//
// Two kernels.  dft_fold_kernel reads the state once and writes (P, Q, R, S) per (voxel, order): the table is wave-uniform in
// the main kernel, where it travels through scalar loads and enters v_fma_f64 as an SGPR operand -- no vector register and no
// LDS traffic for the left-hand side.  dft_kernel: a block of DFT_WAVES wavefronts owns 64 positions (one per lane) x DFT_TV
// voxels (DFT_VW per wavefront, accumulators in registers).  The phasors of DFT_WAVES orders x 64 positions are staged through
// LDS, double-buffered: wavefront w evaluates sincos for order j0 + w at its lane's position -- ONE full-precision fp64 sincos
// per lane and chunk against 4 * DFT_VW * DFT_WAVES multiply-adds -- and every wavefront then reads one (c, s) pair per order.
// No fast-math, no float phasors (|theta| reaches hundreds of radians); fp64 VALU rather than v_mfma_f64: the matrix pipe adds
// no fp64 rate on this part and the voxel side may be as short as three rows.  Plain vector stores only.
#include "epgx_dft.h"

namespace epgx {

__global__ void __launch_bounds__(256) dft_fold_kernel(const DftArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = dft_table_voxels(a.nvox) * a.nrow;
    if (idx >= total) return;
    const int64_t v = idx / a.nrow;
    const int32_t j = (int32_t)(idx - v * a.nrow);
    d2 lo = {0.0, 0.0}, hi = {0.0, 0.0};
    if (v < a.nvox) {     // (the voxels that round the table up to a multiple of DFT_VW hold zeros)
        const d2 *st = a.state + (a.vox0 + v) * 3 * (int64_t)a.K;
        const d2 fa = st[j];
        d2 fb = {0.0, 0.0};
        if (j > 0) fb = st[a.K + j];
        const double w = a.w[j];
        lo.x = w * (fa.x + fb.x);
        lo.y = w * (fa.y + fb.y);
        hi.x = w * (fa.x - fb.x);
        hi.y = w * (fa.y - fb.y);
    }
    d2 *dst = (d2 *)(a.table + idx * 4);
    dst[0] = lo;
    dst[1] = hi;
}

__global__ void __launch_bounds__(DFT_WAVES * 64) dft_kernel(const DftArgs a) {
    __shared__ d2 phasor[2][DFT_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t p = (int64_t)blockIdx.x * DFT_TP + lane;
    const int64_t pc = p < a.npos ? p : a.npos - 1;
    const double x0 = a.pos[pc * 3], x1 = a.pos[pc * 3 + 1], x2 = a.pos[pc * 3 + 2];
    const int64_t v0 = (int64_t)blockIdx.y * DFT_TV + (int64_t)wave * DFT_VW;
    const bool active = v0 < a.nvox;     // wave-uniform; the table covers v0 .. v0 + DFT_VW - 1 of every active wavefront
    const const_f64_t kvec = (const_f64_t)(uintptr_t)a.k;
    const const_f64_t tab = (const_f64_t)(uintptr_t)a.table + v0 * a.nrow * 4;
    const int64_t vstride = (int64_t)a.nrow * 4;
    const int nrow = a.nrow;

    double re[DFT_VW], im[DFT_VW];
#pragma unroll
    for (int i = 0; i < DFT_VW; ++i) re[i] = im[i] = 0.0;

    auto stage = [&](int j0, int buf) {
        const int j = j0 + wave;
        d2 cs = {1.0, 0.0};
        if (j < nrow) {
            const double theta = fma(kvec[j * 3 + 2], x2, fma(kvec[j * 3 + 1], x1, kvec[j * 3] * x0));
            double s, c;
            sincos(theta, &s, &c);
            cs.x = c;
            cs.y = s;
        }
        phasor[buf][wave][lane] = cs;
    };

    stage(0, 0);
    __syncthreads();
    for (int j0 = 0, buf = 0; j0 < nrow; j0 += DFT_WAVES, buf ^= 1) {
        if (j0 + DFT_WAVES < nrow) stage(j0 + DFT_WAVES, buf ^ 1);
        if (active) {
            const int jn = nrow - j0 < DFT_WAVES ? nrow - j0 : DFT_WAVES;
            for (int jj = 0; jj < jn; ++jj) {
                const d2 cs = phasor[buf][jj][lane];
                const const_f64_t t = tab + (int64_t)(j0 + jj) * 4;
#pragma unroll
                for (int i = 0; i < DFT_VW; ++i) {
                    const f64x4 q = *(const EPGX_CONSTANT f64x4 *)(t + i * vstride);
                    re[i] = fma(q.x, cs.x, re[i]);
                    re[i] = fma(-q.y, cs.y, re[i]);
                    im[i] = fma(q.z, cs.y, im[i]);
                    im[i] = fma(q.w, cs.x, im[i]);
                }
            }
        }
        __syncthreads();   // every read of `buf` is done before the next round stages into it
    }

    if (!active || p >= a.npos) return;
#pragma unroll
    for (int i = 0; i < DFT_VW; ++i) {
        if (v0 + i < a.nvox) {
            d2 val;
            val.x = re[i] * a.phase_re - im[i] * a.phase_im;
            val.y = re[i] * a.phase_im + im[i] * a.phase_re;
            a.out[(v0 + i) * a.npos + p] = val;
        }
    }
}

}  // namespace epgx

hipError_t epgx_launch_dft(hipStream_t stream, const epgx::DftArgs &a) {
    using namespace epgx;
    const int64_t entries = dft_table_voxels(a.nvox) * a.nrow;
    hipLaunchKernelGGL(dft_fold_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((a.npos + DFT_TP - 1) / DFT_TP), (unsigned)((a.nvox + DFT_TV - 1) / DFT_TV));
    hipLaunchKernelGGL(dft_kernel, grid, dim3(DFT_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

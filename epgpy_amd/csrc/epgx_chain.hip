// epgx_chain.hip -- chain_kernel: a run of state-wise operators collapsed into ONE EPGX_OP_MAT0 table entry per voxel
// (include/epgx.h epgx_chain) and its launcher.
//
// A run without a shift and without a probe is one affine map x -> M x + o (density) at every order of a voxel, M of the EPG
// symmetry.  One lane owns one destination entry and keeps the running map in registers in the EPGX_OP_MAT0 parametrisation
//      row 0 = (u, p, q)    row 1 = (conj p, conj u, conj q)    row 2 = (t, conj t, c22)      o = (o0, conj o0, o2)
// (u, p, q, t, o0 complex, c22, o2 real: 12 doubles); a step multiplies from the left, (M, o) <- (A M, A o + a).  Sources with
// one entry for all voxels travel through scalar loads; a per-entry relaxation that a group repeats is loaded once per group.
// Plain fp64 multiply-adds, no LDS, no scratch.
#include "epgx_chain.h"

namespace epgx {

struct Affine {
    double ur, ui, pr, pi, qr, qi, tr, ti, c, o0r, o0i, o2;
};

// the general symmetric 3x3 (+ constant term) of one step, from an EPGX_OP_T / MAT / MAT0 entry
struct StepMat {
    double ur, ui, pr, pi, qr, qi, tr, ti, c, ar, ai, a2;
};

template <typename P>   // P: const double * (per lane) or const_f64_t (scalar loads)
__device__ __forceinline__ StepMat load_mat(P src, int kind) {
    StepMat m;
    if (kind == EPGX_OP_T) {   // m00, Re/Im m01, Re/Im m02, Re/Im m20, m22
        m.ur = src[0]; m.ui = 0.0;
        m.pr = src[1]; m.pi = src[2]; m.qr = src[3]; m.qi = src[4]; m.tr = src[5]; m.ti = src[6]; m.c = src[7];
        m.ar = 0.0; m.ai = 0.0; m.a2 = 0.0;
    } else {                   // Re/Im m00, m01, m02, m20, m22, pad [, Re/Im o0, o2, pad]
        m.ur = src[0]; m.ui = src[1];
        m.pr = src[2]; m.pi = src[3]; m.qr = src[4]; m.qi = src[5]; m.tr = src[6]; m.ti = src[7]; m.c = src[8];
        const bool has0 = kind == EPGX_OP_MAT0;
        m.ar = has0 ? src[10] : 0.0; m.ai = has0 ? src[11] : 0.0; m.a2 = has0 ? src[12] : 0.0;
    }
    return m;
}

// (M, o) <- (A M, A o + a); the same order of operations as Collapsed.host_table (epgpy_amd/collapse.py)
__device__ __forceinline__ void apply_mat(Affine &s, const StepMat &a) {
    Affine n;
    // row 0 of A: (u, p, q) times the columns of M
    n.ur = a.ur * s.ur - a.ui * s.ui + (a.pr * s.pr + a.pi * s.pi) + (a.qr * s.tr - a.qi * s.ti);
    n.ui = a.ur * s.ui + a.ui * s.ur + (a.pi * s.pr - a.pr * s.pi) + (a.qr * s.ti + a.qi * s.tr);
    n.pr = a.ur * s.pr - a.ui * s.pi + (a.pr * s.ur + a.pi * s.ui) + (a.qr * s.tr + a.qi * s.ti);
    n.pi = a.ur * s.pi + a.ui * s.pr + (a.pi * s.ur - a.pr * s.ui) + (a.qi * s.tr - a.qr * s.ti);
    n.qr = a.ur * s.qr - a.ui * s.qi + (a.pr * s.qr + a.pi * s.qi) + a.qr * s.c;
    n.qi = a.ur * s.qi + a.ui * s.qr + (a.pi * s.qr - a.pr * s.qi) + a.qi * s.c;
    // row 2 of A: (t, conj t, c22)
    n.tr = a.tr * s.ur - a.ti * s.ui + (a.tr * s.pr - a.ti * s.pi) + a.c * s.tr;
    n.ti = a.tr * s.ui + a.ti * s.ur - (a.tr * s.pi + a.ti * s.pr) + a.c * s.ti;
    n.c = 2.0 * (a.tr * s.qr - a.ti * s.qi) + a.c * s.c;
    n.o0r = a.ur * s.o0r - a.ui * s.o0i + (a.pr * s.o0r + a.pi * s.o0i) + a.qr * s.o2 + a.ar;
    n.o0i = a.ur * s.o0i + a.ui * s.o0r + (a.pi * s.o0r - a.pr * s.o0i) + a.qi * s.o2 + a.ai;
    n.o2 = 2.0 * (a.tr * s.o0r - a.ti * s.o0i) + a.c * s.o2 + a.a2;
    s = n;
}

// diagonal (e0, conj e0, e2) with the recovery r on Z_0
__device__ __forceinline__ void apply_e(Affine &s, double er, double ei, double e2, double r) {
    double x;
    x = er * s.ur - ei * s.ui; s.ui = er * s.ui + ei * s.ur; s.ur = x;
    x = er * s.pr - ei * s.pi; s.pi = er * s.pi + ei * s.pr; s.pr = x;
    x = er * s.qr - ei * s.qi; s.qi = er * s.qi + ei * s.qr; s.qr = x;
    x = er * s.o0r - ei * s.o0i; s.o0i = er * s.o0i + ei * s.o0r; s.o0r = x;
    s.tr *= e2; s.ti *= e2; s.c *= e2;
    s.o2 = e2 * s.o2 + r;
}

__device__ __forceinline__ int ncoef_of(int kind) {
    return kind == EPGX_OP_E ? 4 : (kind == EPGX_OP_T ? 8 : (kind == EPGX_OP_MAT ? 10 : 14));
}

__global__ void __launch_bounds__(256) chain_kernel(const ChainArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_entries) return;
    // this entry's index in every index space of the plan (validated: a source only varies where the destination does)
    int64_t i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    for (int d = 0; d < a.ndim; ++d) {
        if (a.dst_str[d] == 0) continue;
        const int64_t c = (idx / a.dst_str[d]) % a.shape[d];
        i0 += c * a.sp_str[0][d];
        i1 += c * a.sp_str[1][d];
        i2 += c * a.sp_str[2][d];
        i3 += c * a.sp_str[3][d];
    }
    const EPGX_CONSTANT epgx_chain_step *steps = (const EPGX_CONSTANT epgx_chain_step *)(uintptr_t)a.steps;
    const const_f64_t cpool = (const_f64_t)(uintptr_t)a.pool;
    const double *pool = a.pool;
    Affine s = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    for (int first = 0; first < a.n_steps;) {
        const int group = steps[first].group, count = steps[first].count;
        // the group's steps (wave-uniform: SGPRs), and a per-entry relaxation that every repetition reads: loaded once
        int64_t off[EPGX_CHAIN_GROUP], stride[EPGX_CHAIN_GROUP], at[EPGX_CHAIN_GROUP];
        int kind[EPGX_CHAIN_GROUP], space[EPGX_CHAIN_GROUP];
        double keep[EPGX_CHAIN_GROUP][4];
#pragma unroll
        for (int j = 0; j < EPGX_CHAIN_GROUP; ++j) {
            if (j >= group) continue;
            off[j] = steps[first + j].off; stride[j] = steps[first + j].stride;
            kind[j] = steps[first + j].kind; space[j] = steps[first + j].space;
            const int64_t ix = space[j] == 0 ? i0 : (space[j] == 1 ? i1 : (space[j] == 2 ? i2 : i3));
            at[j] = space[j] < 0 ? 0 : ix * ncoef_of(kind[j]);
            if (kind[j] == EPGX_OP_E && stride[j] == 0 && space[j] >= 0) {
                const double *src = pool + off[j] + at[j];
                keep[j][0] = src[0]; keep[j][1] = src[1]; keep[j][2] = src[2]; keep[j][3] = src[3];
            }
        }
        for (int r = 0; r < count; ++r) {
#pragma unroll
            for (int j = 0; j < EPGX_CHAIN_GROUP; ++j) {
                if (j >= group) continue;
                const int64_t from = off[j] + (int64_t)r * stride[j];
                if (kind[j] == EPGX_OP_E) {
                    if (space[j] < 0) {
                        const const_f64_t src = cpool + from;
                        apply_e(s, src[0], src[1], src[2], src[3]);
                    } else if (stride[j] == 0) {
                        apply_e(s, keep[j][0], keep[j][1], keep[j][2], keep[j][3]);
                    } else {
                        const double *src = pool + from + at[j];
                        apply_e(s, src[0], src[1], src[2], src[3]);
                    }
                } else if (space[j] < 0) {
                    apply_mat(s, load_mat(cpool + from, kind[j]));
                } else {
                    apply_mat(s, load_mat(pool + from + at[j], kind[j]));
                }
            }
        }
        first += group;
    }
    double *dst = a.pool + a.dst_off + idx * 14;   // EPGX_OP_MAT0 layout
    dst[0] = s.ur; dst[1] = s.ui; dst[2] = s.pr; dst[3] = s.pi; dst[4] = s.qr; dst[5] = s.qi; dst[6] = s.tr; dst[7] = s.ti;
    dst[8] = s.c; dst[9] = 0.0; dst[10] = s.o0r; dst[11] = s.o0i; dst[12] = s.o2; dst[13] = 0.0;
}

}  // namespace epgx

hipError_t epgx_launch_chain(hipStream_t stream, const epgx::ChainArgs &a) {
    hipLaunchKernelGGL(epgx::chain_kernel, dim3((unsigned)((a.n_entries + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

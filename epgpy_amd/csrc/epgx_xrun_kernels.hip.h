// epgx_xrun_kernels.hip.h -- xrun_kernel<NC, M, HAS_IN>: a range with exchange (EPGX_OP_X) in ONE launch, the state in
// registers.  Included by epgx_xrun.hip (one translation unit per NC) and, for XRunArgs, by epgx_api.hip.
//
// One wavefront owns one compartment group: the NC voxels v0, v0 + stride, .. of the grid.  It holds the State<M> of every
// compartment (order 64 m + lane, the layout of run_kernel) and walks the primitive operator list: T / T0 / MAT / MAT0 / E /
// S(n) / ADC / SPOILER / RESET / PD act on each compartment with that compartment voxel's table entries and density
// (apply_T, apply_MAT, apply_E, shift_one / shift_lds, truncate: the per-state code of run_kernel); X mixes the compartments
// order by order inside each lane (no cross-lane traffic), with the group's table entry.  D and gather shifts are not
// handled: epgx_run runs such ranges as pieces (split path).
#pragma once
#include "epgx_kernels.hip.h"

namespace epgx {

struct XRunArgs {
    const epgx_op *__restrict__ ops;   // device copy of the plan's operators
    int32_t op_begin, op_end;
    const double *__restrict__ coef;   // the plan's pool
    const d2 *__restrict__ in;         // [nvox][3][K] of the range, or NULL (equilibrium)
    const double *__restrict__ dens_in;
    d2 *__restrict__ out;              // or NULL (state-resident)
    double *__restrict__ dens_out;
    d2 *__restrict__ signal;           // column j = voxel vox0 + j of the range
    int64_t signal_ld;
    int64_t vox0, stride;              // first voxel of the range (grid); compartment stride (voxels)
    int32_t ndim, n_spaces;
    int64_t shape[EPGX_MAX_DIMS];
    int64_t strides[EPGX_MAX_SPACES][EPGX_MAX_DIMS];
};

// table entry of operator `op` for the voxel whose index-space coordinates are `ix` (selects, no dynamic indexing)
__device__ __forceinline__ const double *xrun_entry(const XRunArgs &a, const epgx_op &op, const int64_t (&ix)[EPGX_MAX_SPACES]) {
    int64_t e = 0;
#pragma unroll
    for (int s = 0; s < EPGX_MAX_SPACES; ++s) e = (op.space == s) ? ix[s] : e;
    return a.coef + op.coef_off + e * op.ncoef;
}

// lane-local exchange of the NC compartments at every order: EPGX_OP_X of include/epgx.h
template <int NC, int M>
__device__ __forceinline__ void xrun_exchange(State<M> (&st)[NC], const double *__restrict__ tab, const double (&rho)[NC], int lane) {
    const double *mT = tab, *mL = tab + 2 * NC * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) st[c].Zr[0] -= (lane == 0) ? rho[c] : 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double ar[NC], ai[NC], br[NC], bi[NC], zr[NC], zi[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double Ar = 0.0, Ai = 0.0, Br = 0.0, Bi = 0.0, Zr = 0.0, Zi = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double mr = mT[2 * (c * NC + j)], mi = mT[2 * (c * NC + j) + 1], ml = mL[c * NC + j];
                const State<M> &s = st[j];
                Ar = fma(mr, s.Ar[m], fma(-mi, s.Ai[m], Ar));
                Ai = fma(mr, s.Ai[m], fma(mi, s.Ar[m], Ai));
                Br = fma(mr, s.Br[m], fma(mi, s.Bi[m], Br));
                Bi = fma(mr, s.Bi[m], fma(-mi, s.Br[m], Bi));
                Zr = fma(ml, s.Zr[m], Zr);
                Zi = fma(ml, s.Zi[m], Zi);
            }
            ar[c] = Ar; ai[c] = Ai; br[c] = Br; bi[c] = Bi; zr[c] = Zr; zi[c] = Zi;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            st[c].Ar[m] = ar[c]; st[c].Ai[m] = ai[c];
            st[c].Br[m] = br[c]; st[c].Bi[m] = bi[c];
            st[c].Zr[m] = zr[c]; st[c].Zi[m] = zi[c];
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) st[c].Zr[0] += (lane == 0) ? rho[c] : 0.0;
}

template <int NC, int M, bool HAS_IN>
__global__ void __launch_bounds__(64) xrun_kernel(const XRunArgs a) {
    constexpr int K = 64 * M;
    __shared__ d2 wl[2 * K];                      // staging of shifts by |n| >= 2
    const int lane = (int)threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t outer = g / a.stride, inner = g - outer * a.stride;
    const int64_t v0 = outer * NC * a.stride + inner;      // compartment 0 of this group (voxel of the range)
    // index-space coordinates of every compartment voxel
    int64_t ix[NC][EPGX_MAX_SPACES];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int s = 0; s < EPGX_MAX_SPACES; ++s) ix[c][s] = 0;
        int64_t rem = a.vox0 + v0 + c * a.stride;
        for (int d = a.ndim - 1; d >= 0; --d) {
            const int64_t q = rem / a.shape[d], co = rem - q * a.shape[d];
            rem = q;
#pragma unroll
            for (int s = 0; s < EPGX_MAX_SPACES; ++s) ix[c][s] += co * a.strides[s][d];
        }
    }
    State<M> st[NC];
    double dens[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int64_t v = v0 + c * a.stride;
        if (HAS_IN) {
            const d2 *src = a.in + (size_t)v * 3 * K;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const d2 x = src[64 * m + lane], y = src[K + 64 * m + lane], z = src[2 * K + 64 * m + lane];
                st[c].Ar[m] = x.x; st[c].Ai[m] = x.y;
                st[c].Br[m] = y.x; st[c].Bi[m] = y.y;
                st[c].Zr[m] = z.x; st[c].Zi[m] = z.y;
            }
            dens[c] = a.dens_in[v];
        } else {
            dens[c] = 1.0;
            set_equilibrium(st[c], lane, 1.0);
        }
    }
    const double oh0 = lane == 0 ? 1.0 : 0.0;
    const uint32_t voff0 = lane == 0 ? 0u : 16u;
    for (int i = a.op_begin; i < a.op_end; ++i) {
        const epgx_op op = a.ops[i];
        switch (op.opcode) {
        case EPGX_OP_T: case EPGX_OP_T0: case EPGX_OP_MAT: case EPGX_OP_MAT0: {
            const bool mat = op.opcode == EPGX_OP_MAT || op.opcode == EPGX_OP_MAT0;
            const bool konst = op.opcode == EPGX_OP_T0 || op.opcode == EPGX_OP_MAT0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double *e = xrun_entry(a, op, ix[c]);
                double tc[10];
#pragma unroll
                for (int j = 0; j < 8; ++j) tc[j] = e[j];
                tc[8] = mat ? e[8] : 0.0;
                tc[9] = mat ? e[9] : 0.0;
                if (mat) apply_MAT(st[c], tc);
                else apply_T(st[c], tc);
                if (konst) {   // (o0, conj o0, o2) * density on the k = 0 order
                    const double *o = e + (mat ? 10 : 8);
                    const double eqv = lane == 0 ? dens[c] : 0.0;
                    st[c].Ar[0] = fma(o[0], eqv, st[c].Ar[0]);
                    st[c].Ai[0] = fma(o[1], eqv, st[c].Ai[0]);
                    st[c].Br[0] = fma(o[0], eqv, st[c].Br[0]);
                    st[c].Bi[0] = fma(-o[1], eqv, st[c].Bi[0]);
                    st[c].Zr[0] = fma(o[2], eqv, st[c].Zr[0]);
                }
            }
            break;
        }
        case EPGX_OP_E:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double *e = xrun_entry(a, op, ix[c]);
                const double ec[4] = {e[0], e[1], e[2], e[3]};
                apply_E(st[c], ec, lane == 0 ? dens[c] : 0.0);
            }
            break;
        case EPGX_OP_S:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (op.ia == 1) shift_one<M, false>(st[c], lane, oh0);
                else if (op.ia == -1) shift_one<M, true>(st[c], lane, oh0);
                else if (op.ia > 0) shift_lds<M, false>(st[c], op.ia, wl, lane);
                else shift_lds<M, true>(st[c], -op.ia, wl, lane);
                if (op.ib < K - 1) truncate(st[c], op.ib, lane);
            }
            break;
        case EPGX_OP_ADC:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double zr = st[c].Zr[0], zi = st[c].Zi[0];
                asm volatile("" : "+v"(zr), "+v"(zi));
                d2 val;
                val.x = op.ib ? zr : st[c].Ar[0];
                val.y = op.ib ? zi : st[c].Ai[0];
                store_lane0(a.signal + (int64_t)op.ia * a.signal_ld + v0 + c * a.stride, val, voff0);
            }
            break;
        case EPGX_OP_SPOIL:
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int m = 0; m < M; ++m) st[c].Ar[m] = st[c].Ai[m] = st[c].Br[m] = st[c].Bi[m] = 0.0;
            break;
        case EPGX_OP_RESET:
#pragma unroll
            for (int c = 0; c < NC; ++c) set_equilibrium(st[c], lane, dens[c]);
            break;
        case EPGX_OP_PD:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                dens[c] = xrun_entry(a, op, ix[c])[0];
                if (op.ia) set_equilibrium(st[c], lane, dens[c]);
            }
            break;
        case EPGX_OP_X: {
            const double *tab = xrun_entry(a, op, ix[0]);
            xrun_exchange<NC, M>(st, tab, dens, lane);
            break;
        }
        default: break;      // NOP (D / gather shifts never reach this kernel)
        }
    }
    if (a.out) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int64_t v = v0 + c * a.stride;
            d2 *dst = a.out + (size_t)v * 3 * K;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                d2 x, y, z;
                x.x = st[c].Ar[m]; x.y = st[c].Ai[m];
                y.x = st[c].Br[m]; y.y = st[c].Bi[m];
                z.x = st[c].Zr[m]; z.y = st[c].Zi[m];
                dst[64 * m + lane] = x;
                dst[K + 64 * m + lane] = y;
                dst[2 * K + 64 * m + lane] = z;
            }
            if (lane == 0) a.dens_out[v] = dens[c];
        }
    }
}

}  // namespace epgx

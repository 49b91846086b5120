// epgx_dxrun_kernels.hip.h -- dxrun_kernel<NC, M, V>: a range with exchange (EPGX_OP_X) and V first-order derivative states in
// ONE launch, the state and the derivative states in registers.  Included by epgx_dxrun.hip (one translation unit per NC)
// and, for DXRunArgs, by epgx_api.hip.
//
// xrun_kernel with derivative states: one wavefront owns one compartment group and holds, per compartment, the State<M> and
// V derivative states (12 M fp64 registers each: NC M (1 + V) <= 8, the footprint of xrun_kernel<4, 2>).  It walks the
// primitive operator list with the parallel epgx_dop list; the records have the semantics of deriv_kernel
// (epgx_deriv_kernels.hip.h):  dS_v <- Op(dS_v, no equilibrium term) + (dOp/dv)(S),  S <- Op(S);  SPOILER acts on the
// derivative states only under EPGX_DERIV_THROUGH_PLAIN_OPS, RESET and PD-with-reset always clear them.  X is a
// differentiable operator here: it always acts on the derivative states, and where its epgx_dop names a table
// (3 NC^2 doubles per group: Re/Im of d mT, then d mL) the partial acts on the state before the update (include/epgx.h,
// EPGX_OP_X).  State-resident from equilibrium only; every ADC writes 1 + V rows per compartment column.
#pragma once
#include "epgx_deriv_kernels.hip.h"
#include "epgx_xrun_kernels.hip.h"

namespace epgx {

struct DXRunArgs {
    XRunArgs x;                          // as for xrun_kernel; in / out are NULL
    const epgx_dop *__restrict__ dops;   // device copy of the plan's partials, parallel to x.ops
    int32_t through_plain;               // EPGX_DERIV_THROUGH_PLAIN_OPS
    int32_t reserved;
};

// table entry (`ncoef` doubles) of the partial of variable v for the voxel whose index-space coordinates are `ix`
__device__ __forceinline__ const double *dxrun_entry(const XRunArgs &a, int64_t off, int32_t space, int ncoef,
                                                     const int64_t (&ix)[EPGX_MAX_SPACES]) {
    int64_t e = 0;
#pragma unroll
    for (int s = 0; s < EPGX_MAX_SPACES; ++s) e = (space == s) ? ix[s] : e;
    return a.coef + off + e * ncoef;
}

// d <- X d + dX s at every order, s the state BEFORE its own update (Z_0 of s already without its density);
// dtab == NULL: X does not depend on the variable
template <int NC, int M>
__device__ __forceinline__ void dxrun_exchange(State<M> (&d)[NC], const State<M> (&st)[NC], const double *__restrict__ tab,
                                               const double *__restrict__ dtab) {
    const double *mT = tab, *mL = tab + 2 * NC * NC;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double ar[NC], ai[NC], br[NC], bi[NC], zr[NC], zi[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double Ar = 0.0, Ai = 0.0, Br = 0.0, Bi = 0.0, Zr = 0.0, Zi = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double mr = mT[2 * (c * NC + j)], mi = mT[2 * (c * NC + j) + 1], ml = mL[c * NC + j];
                const State<M> &s = d[j];
                Ar = fma(mr, s.Ar[m], fma(-mi, s.Ai[m], Ar));
                Ai = fma(mr, s.Ai[m], fma(mi, s.Ar[m], Ai));
                Br = fma(mr, s.Br[m], fma(mi, s.Bi[m], Br));
                Bi = fma(mr, s.Bi[m], fma(-mi, s.Br[m], Bi));
                Zr = fma(ml, s.Zr[m], Zr);
                Zi = fma(ml, s.Zi[m], Zi);
            }
            if (dtab) {      // wave-uniform
                const double *dT = dtab, *dL = dtab + 2 * NC * NC;
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const double mr = dT[2 * (c * NC + j)], mi = dT[2 * (c * NC + j) + 1], ml = dL[c * NC + j];
                    const State<M> &s = st[j];
                    Ar = fma(mr, s.Ar[m], fma(-mi, s.Ai[m], Ar));
                    Ai = fma(mr, s.Ai[m], fma(mi, s.Ar[m], Ai));
                    Br = fma(mr, s.Br[m], fma(mi, s.Bi[m], Br));
                    Bi = fma(mr, s.Bi[m], fma(-mi, s.Br[m], Bi));
                    Zr = fma(ml, s.Zr[m], Zr);
                    Zi = fma(ml, s.Zi[m], Zi);
                }
            }
            ar[c] = Ar; ai[c] = Ai; br[c] = Br; bi[c] = Bi; zr[c] = Zr; zi[c] = Zi;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            d[c].Ar[m] = ar[c]; d[c].Ai[m] = ai[c];
            d[c].Br[m] = br[c]; d[c].Bi[m] = bi[c];
            d[c].Zr[m] = zr[c]; d[c].Zi[m] = zi[c];
        }
    }
}

template <int NC, int M, int V>
__global__ void __launch_bounds__(64) dxrun_kernel(const DXRunArgs da) {
    static_assert(NC * M * (1 + V) <= 8, "the state and its derivative states stay within 96 fp64 registers per lane");
    constexpr int K = 64 * M;
    __shared__ d2 wl[2 * K];                      // staging of shifts by |n| >= 2
    const XRunArgs &a = da.x;
    const int lane = (int)threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t outer = g / a.stride, inner = g - outer * a.stride;
    const int64_t v0 = outer * NC * a.stride + inner;      // compartment 0 of this group (voxel of the range)
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
    State<M> dst[V][NC];
    double dens[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        dens[c] = 1.0;
        set_equilibrium(st[c], lane, 1.0);
#pragma unroll
        for (int v = 0; v < V; ++v) set_zero(dst[v][c]);
    }
    const double oh0 = lane == 0 ? 1.0 : 0.0;
    const uint32_t voff0 = lane == 0 ? 0u : 16u;
    for (int i = a.op_begin; i < a.op_end; ++i) {
        const epgx_op op = a.ops[i];
        const epgx_dop dp = da.dops[i];
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
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (mat) apply_MAT(dst[v][c], tc);
                    else apply_T(dst[v][c], tc);
                    if (dp.coef_off[v] >= 0) {     // the partial acts on the state before its update
                        const double *p = dxrun_entry(a, dp.coef_off[v], dp.space[v], 10, ix[c]);
                        double dc[10];
#pragma unroll
                        for (int j = 0; j < 10; ++j) dc[j] = p[j];
                        acc_MAT(dst[v][c], st[c], dc);
                    }
                }
                if (mat) apply_MAT(st[c], tc);
                else apply_T(st[c], tc);
                if (konst) {   // (o0, conj o0, o2) * density on the k = 0 order; no such term in the derivative states
                    const double *o = e + (mat ? 10 : 8);
                    acc_C(st[c], o[0], o[1], o[2], lane == 0 ? dens[c] : 0.0);
                }
            }
            break;
        }
        case EPGX_OP_E:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double *e = xrun_entry(a, op, ix[c]);
                const double ec[4] = {e[0], e[1], e[2], e[3]};
                const double eqv = lane == 0 ? dens[c] : 0.0;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    apply_E(dst[v][c], ec, 0.0);
                    if (dp.coef_off[v] >= 0) {
                        const double *p = dxrun_entry(a, dp.coef_off[v], dp.space[v], 4, ix[c]);
                        const double dc[4] = {p[0], p[1], p[2], p[3]};
                        acc_E(dst[v][c], st[c], dc, eqv);
                    }
                }
                apply_E(st[c], ec, eqv);
            }
            break;
        case EPGX_OP_S:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                shift_any(st[c], op.ia, wl, lane, oh0);
                if (op.ib < K - 1) truncate(st[c], op.ib, lane);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    shift_any(dst[v][c], op.ia, wl, lane, oh0);
                    if (op.ib < K - 1) truncate(dst[v][c], op.ib, lane);
                }
            }
            break;
        case EPGX_OP_ADC:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                d2 *row = a.signal + (int64_t)op.ia * a.signal_ld + v0 + c * a.stride;
                double zr = st[c].Zr[0], zi = st[c].Zi[0];
                asm volatile("" : "+v"(zr), "+v"(zi));
                d2 val;
                val.x = op.ib ? zr : st[c].Ar[0];
                val.y = op.ib ? zi : st[c].Ai[0];
                store_lane0(row, val, voff0);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    double dzr = dst[v][c].Zr[0], dzi = dst[v][c].Zi[0];
                    asm volatile("" : "+v"(dzr), "+v"(dzi));
                    val.x = op.ib ? dzr : dst[v][c].Ar[0];
                    val.y = op.ib ? dzi : dst[v][c].Ai[0];
                    store_lane0(row + (int64_t)(1 + v) * a.signal_ld, val, voff0);
                }
            }
            break;
        case EPGX_OP_SPOIL:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
#pragma unroll
                for (int m = 0; m < M; ++m) st[c].Ar[m] = st[c].Ai[m] = st[c].Br[m] = st[c].Bi[m] = 0.0;
                if (da.through_plain) {
#pragma unroll
                    for (int v = 0; v < V; ++v)
#pragma unroll
                        for (int m = 0; m < M; ++m) dst[v][c].Ar[m] = dst[v][c].Ai[m] = dst[v][c].Br[m] = dst[v][c].Bi[m] = 0.0;
                }
            }
            break;
        case EPGX_OP_RESET:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                set_equilibrium(st[c], lane, dens[c]);
#pragma unroll
                for (int v = 0; v < V; ++v) set_zero(dst[v][c]);
            }
            break;
        case EPGX_OP_PD:
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                dens[c] = xrun_entry(a, op, ix[c])[0];
                if (op.ia) {
                    set_equilibrium(st[c], lane, dens[c]);
#pragma unroll
                    for (int v = 0; v < V; ++v) set_zero(dst[v][c]);
                }
            }
            break;
        case EPGX_OP_X: {
            const double *tab = xrun_entry(a, op, ix[0]);
            // Z_0 - rho is what X exchanges; the derivative states read the state before its own update
#pragma unroll
            for (int c = 0; c < NC; ++c) st[c].Zr[0] -= (lane == 0) ? dens[c] : 0.0;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double *dtab = dp.coef_off[v] >= 0 ? dxrun_entry(a, dp.coef_off[v], dp.space[v], 3 * NC * NC, ix[0]) : nullptr;
                dxrun_exchange<NC, M>(dst[v], st, tab, dtab);
            }
            dxrun_exchange<NC, M>(st, st, tab, nullptr);      // the arithmetic of xrun_exchange (its sums are complete before it writes)
#pragma unroll
            for (int c = 0; c < NC; ++c) st[c].Zr[0] += (lane == 0) ? dens[c] : 0.0;
            break;
        }
        default: break;      // NOP (D / gather shifts never reach this kernel)
        }
    }
}

}  // namespace epgx

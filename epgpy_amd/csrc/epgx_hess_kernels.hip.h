// epgx_hess_kernels.hip.h -- second-order derivatives, one variable pair per launch (EPGX_DERIV_SECOND, include/epgx.h).
//
// The reference propagates, next to S and the first-order states S_v, one state matrix per variable pair
// (DiffOperator._apply_order2, epgpy/diff.py:290-379).  For the pair (a, b) every T / E stage is
//     H_ab <- Op H_ab + (dOp/da) S_b + (dOp/db) S_a + (d2Op/da db) S
//     S_a  <- Op S_a + (dOp/da) S          S_b <- Op S_b + (dOp/db) S          S <- Op S (+ recovery)
// with S, S_a, S_b on the right-hand sides taken BEFORE the stage.  Pairs do not couple, so a Hessian is a sequence of
// one-pair passes.  A wavefront keeps S, S_a, S_b, H_ab of its voxel in VGPRs -- the four states of deriv_kernel<M, NSP, 3>,
// whose stage code (apply_*, acc_*, shifts, truncation) runs here unchanged -- and walks the same fused records; the three
// slots of DRec name the tables of dOp/da, dOp/db and the combined second-order table.  H is updated first, while the
// first-order states and S still hold their values from before the stage.
// DIAG: the pair (a, a) -- three states S, S_a, H_aa; slot 0 = dOp/da, slot 1 = the second-order table, cross term
// 2 (dOp/da) S_a.
// Which cross terms enter at a stage is the host's decision (DRec.pad0, HESS_*: the reference's term selection is per
// operator); the second-order term enters where the H slot has a table (DRec.present).
// Lane-strided order layout (order k = 64 m + lane), state-resident from equilibrium, (1 + NV) signal rows per ADC:
// the probe of S, of the first-order states, of H.
#pragma once
#include "epgx_deriv_kernels.hip.h"

namespace epgx {

__device__ __forceinline__ DRec load_hrec(const EPGX_CONSTANT u32x8 *drecs, int i) {
    const u32x8 a = drecs[2 * i], b = drecs[2 * i + 1];
    DRec r;
    r.t_off[0] = a[0]; r.t_off[1] = a[1]; r.t_off[2] = a[2];
    r.t_ix[0] = a[3]; r.t_ix[1] = a[4]; r.t_ix[2] = a[5];
    r.present = a[6]; r.pad0 = a[7];
    r.e_off[0] = b[0]; r.e_off[1] = b[1]; r.e_off[2] = b[2];
    r.e_ix[0] = b[3]; r.e_ix[1] = b[4]; r.e_ix[2] = b[5];
    r.pad1[0] = r.pad1[1] = 0;
    return r;
}

template <int M, int NSP, bool DIAG>
__global__ void __launch_bounds__(256) hess_kernel(const DerivArgs a) {
    constexpr int NV = DIAG ? 2 : 3;   // derivative states: the first-order ones, then H
    constexpr int NF = NV - 1;         // first-order states
    constexpr int HS = NV - 1;         // H's state, DRec slot and signal row (1 + HS)
    extern __shared__ __attribute__((aligned(16))) d2 smem[];
    constexpr int K = 64 * M;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    d2 *wl = smem + (size_t)wib * a.t.use_lds * K;
    const const_rec_t recs = (const_rec_t)(uintptr_t)a.recs;
    const EPGX_CONSTANT u32x8 *drecs = (const EPGX_CONSTANT u32x8 *)(uintptr_t)a.drecs;
    const const_f64_t pool = (const_f64_t)(uintptr_t)a.coef;
    const const_i32_t vidx = (const_i32_t)(uintptr_t)a.t.vidx;
    const uint32_t b = blockIdx.x;
    const uint32_t quad = (b & ~15u) | ((b & 7u) << 1) | ((b >> 3) & 1u);
    const int64_t v = (int64_t)quad * 4 + wib;
    if (v >= a.nvox) return;

    const uint32_t gv = (uint32_t)(a.t.vox0 + v);
    uint32_t p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;
    if (NSP > 0) p0 = (a.t.dense_spaces & 1u) ? gv : (uint32_t)vidx[v];
    if (NSP > 1) p1 = (a.t.dense_spaces & 2u) ? gv : (uint32_t)vidx[a.t.vidx_ld + v];
    if (NSP > 2) p2 = (a.t.dense_spaces & 4u) ? gv : (uint32_t)vidx[2 * a.t.vidx_ld + v];
    if (NSP > 2) p3 = (a.t.dense_spaces & 8u) ? gv : (uint32_t)vidx[3 * a.t.vidx_ld + v];
    double dens = a.dens_in ? a.dens_in[v] : 1.0;
    double eqv = (lane == 0) ? dens : 0.0;
    const double oh0 = (lane == 0) ? 1.0 : 0.0;
    const uint32_t voff0 = (lane == 0) ? 0u : 16u;
    State<M> s;
    State<M> ds[NV];
    set_equilibrium(s, lane, dens);
#pragma unroll
    for (int j = 0; j < NV; ++j) set_zero(ds[j]);
    d2 *sig_base = a.signal + v;

    // the 10 coefficients of a rotation partial / the 4 of a relaxation partial of slot j, times `scale` (1 or 2: exact)
    auto load_dt = [&](const DRec &dr, int j, double scale, double (&dc)[10]) __attribute__((always_inline)) {
        const_f64_t src = entry<NSP>(pool, dr.t_off[j], dr.t_ix[j], p0, p1, p2, p3);
        const f64x8 lo = *(const EPGX_CONSTANT f64x8 *)src;
        const f64x2 hi = *(const EPGX_CONSTANT f64x2 *)(src + 8);
#pragma unroll
        for (int q = 0; q < 8; ++q) dc[q] = lo[q] * scale;
        dc[8] = hi[0] * scale;
        dc[9] = hi[1] * scale;
    };
    auto load_de = [&](const DRec &dr, int j, double scale, double (&dc)[4]) __attribute__((always_inline)) {
        const f64x4 e = *(const EPGX_CONSTANT f64x4 *)entry<NSP>(pool, dr.e_off[j], dr.e_ix[j], p0, p1, p2, p3);
#pragma unroll
        for (int q = 0; q < 4; ++q) dc[q] = e[q] * scale;
    };

    for (int i = 0; i < a.t.n_rec; ++i) {
        const Rec r = load_rec(recs, i);
        const DRec dr = load_hrec(drecs, i);
        const uint32_t f = r.flags;
        if (f & (F_GS | F_D)) {
            const uint32_t off = entry_offset<NSP>(r.t_off, r.t_ix, p0, p1, p2, p3);
            if (f & F_GS) {
                gather_shift(s, (const int32_t *)((const char *)a.coef + off), wl, lane);
#pragma unroll
                for (int j = 0; j < NV; ++j) gather_shift(ds[j], (const int32_t *)((const char *)a.coef + off), wl, lane);
            }
            if (f & F_D) {
                apply_D(s, (const double *)((const char *)a.coef + off), lane);
                if (a.through_plain) {
#pragma unroll
                    for (int j = 0; j < NV; ++j) apply_D(ds[j], (const double *)((const char *)a.coef + off), lane);
                }
            }
            continue;
        }
        double tc[10], ec[4];
        if (f & (F_T | F_MAT)) {
            const_f64_t src = entry<NSP>(pool, r.t_off, r.t_ix, p0, p1, p2, p3);
            const f64x8 lo = *(const EPGX_CONSTANT f64x8 *)src;
            const f64x2 hi = *(const EPGX_CONSTANT f64x2 *)(src + 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) tc[j] = lo[j];
            tc[8] = hi[0];
            tc[9] = hi[1];
        }
        if (f & (F_E | F_PD)) {
            const f64x4 e = *(const EPGX_CONSTANT f64x4 *)entry<NSP>(pool, r.e_off, r.e_ix, p0, p1, p2, p3);
#pragma unroll
            for (int j = 0; j < 4; ++j) ec[j] = e[j];
        }
        if (f & (F_SPOIL | F_RESET | F_PD)) {
            if (f & F_SPOIL) {
#pragma unroll
                for (int m = 0; m < M; ++m) s.Ar[m] = s.Ai[m] = s.Br[m] = s.Bi[m] = 0.0;
                if (a.through_plain) {
#pragma unroll
                    for (int j = 0; j < NV; ++j)
#pragma unroll
                        for (int m = 0; m < M; ++m) ds[j].Ar[m] = ds[j].Ai[m] = ds[j].Br[m] = ds[j].Bi[m] = 0.0;
                }
            }
            if (f & F_PD) {
                dens = ec[0];
                eqv = (lane == 0) ? dens : 0.0;
            }
            if (f & (F_RESET | F_PD_RESET)) {   // a reset clears the derivative states, H included (cf. deriv_kernel)
                set_equilibrium(s, lane, dens);
#pragma unroll
                for (int j = 0; j < NV; ++j) set_zero(ds[j]);
            }
        }
        if (f & F_S0) {
            shift_plain<M, false, NoSplit>(s, lane, oh0);
#pragma unroll
            for (int j = 0; j < NV; ++j) shift_plain<M, false, NoSplit>(ds[j], lane, oh0);
        }
        if (f & (F_T | F_MAT)) {
            auto rotate = [&](State<M> &x) __attribute__((always_inline)) {
                if (f & F_TX) apply_TX(x, tc); else if (f & F_TY) apply_TY(x, tc); else if (f & F_T) apply_T(x, tc); else apply_MAT(x, tc);
            };
            // H first: the cross terms read S_a, S_b and the second-order term S from BEFORE the stage
            rotate(ds[HS]);
            if (dr.pad0 & HESS_T_XA) {          // (dT/da) S_b; diagonal pair: 2 (dT/da) S_a
                double dc[10];
                load_dt(dr, 0, DIAG ? 2.0 : 1.0, dc);
                if (dr.present & 256u) acc_TX(ds[HS], ds[DIAG ? 0 : 1], dc); else acc_MAT(ds[HS], ds[DIAG ? 0 : 1], dc);
            }
            if (!DIAG && (dr.pad0 & HESS_T_XB)) {   // (dT/db) S_a
                double dc[10];
                load_dt(dr, 1, 1.0, dc);
                if (dr.present & (256u << 1)) acc_TX(ds[HS], ds[0], dc); else acc_MAT(ds[HS], ds[0], dc);
            }
            if (dr.present & (1u << HS)) {      // (d2T/da db) S
                double dc[10];
                load_dt(dr, HS, 1.0, dc);
                if (dr.present & (256u << HS)) acc_TX(ds[HS], s, dc); else acc_MAT(ds[HS], s, dc);
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                rotate(ds[j]);
                if (dr.present & (1u << j)) {
                    double dc[10];
                    load_dt(dr, j, 1.0, dc);
                    if (dr.present & (256u << j)) acc_TX(ds[j], s, dc); else acc_MAT(ds[j], s, dc);
                }
            }
            rotate(s);
            if (f & (F_MAT0 | F_T0)) {
                const f64x4 o = *(const EPGX_CONSTANT f64x4 *)(entry<NSP>(pool, r.t_off, r.t_ix, p0, p1, p2, p3) +
                                                              ((f & F_T0) ? 8 : 10));
                s.Ar[0] = __builtin_fma(o[0], eqv, s.Ar[0]);
                s.Ai[0] = __builtin_fma(o[1], eqv, s.Ai[0]);
                s.Br[0] = __builtin_fma(o[0], eqv, s.Br[0]);
                s.Bi[0] = __builtin_fma(-o[1], eqv, s.Bi[0]);
                s.Zr[0] = __builtin_fma(o[2], eqv, s.Zr[0]);
            }
        }
        if (f & F_E) {
            // derivative states have no equilibrium term (diff.py:103-109): the cross terms act on S_a / S_b without a
            // recovery, the second-order term acts on S with the second partial of the recovery
            if (f & F_ER) apply_ER(ds[HS], ec, 0.0); else apply_E(ds[HS], ec, 0.0);
            if (dr.pad0 & HESS_E_XA) {
                double dc[4];
                load_de(dr, 0, DIAG ? 2.0 : 1.0, dc);
                if (dr.present & 4096u) acc_ER(ds[HS], ds[DIAG ? 0 : 1], dc, 0.0); else acc_E(ds[HS], ds[DIAG ? 0 : 1], dc, 0.0);
            }
            if (!DIAG && (dr.pad0 & HESS_E_XB)) {
                double dc[4];
                load_de(dr, 1, 1.0, dc);
                if (dr.present & (4096u << 1)) acc_ER(ds[HS], ds[0], dc, 0.0); else acc_E(ds[HS], ds[0], dc, 0.0);
            }
            if (dr.present & (16u << HS)) {
                double dc[4];
                load_de(dr, HS, 1.0, dc);
                if (dr.present & (4096u << HS)) acc_ER(ds[HS], s, dc, eqv); else acc_E(ds[HS], s, dc, eqv);
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                if (f & F_ER) apply_ER(ds[j], ec, 0.0); else apply_E(ds[j], ec, 0.0);
                if (dr.present & (16u << j)) {
                    double dc[4];
                    load_de(dr, j, 1.0, dc);
                    if (dr.present & (4096u << j)) acc_ER(ds[j], s, dc, eqv); else acc_E(ds[j], s, dc, eqv);
                }
            }
            if (f & F_ER) apply_ER(s, ec, eqv); else apply_E(s, ec, eqv);
        }
        if (f & F_S) {
            shift_any(s, r.shift, wl, lane, oh0);
#pragma unroll
            for (int j = 0; j < NV; ++j) shift_any(ds[j], r.shift, wl, lane, oh0);
            if (f & F_TRUNC) {
                truncate_x<M, NoSplit>(s, r.kmax, lane);
#pragma unroll
                for (int j = 0; j < NV; ++j) truncate_x<M, NoSplit>(ds[j], r.kmax, lane);
            }
        }
        if (f & F_ADC) {
            d2 *dst = sig_base + (int64_t)r.slot * a.signal_ld;
            const bool z0 = (f & F_ADC_Z) != 0;
            d2 val;
            double zr = s.Zr[0], zi = s.Zi[0];
            asm volatile("" : "+v"(zr), "+v"(zi));
            val.x = z0 ? zr : s.Ar[0];
            val.y = z0 ? zi : s.Ai[0];
            store_lane0(dst, val, voff0);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                double dzr = ds[j].Zr[0], dzi = ds[j].Zi[0];
                asm volatile("" : "+v"(dzr), "+v"(dzi));
                val.x = z0 ? dzr : ds[j].Ar[0];
                val.y = z0 ? dzi : ds[j].Ai[0];
                store_lane0(dst + (int64_t)(1 + j) * a.signal_ld, val, voff0);
            }
        }
    }
}

}  // namespace epgx

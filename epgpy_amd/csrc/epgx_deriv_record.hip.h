// epgx_deriv_record.hip.h -- the flag-tested record body of first-order derivative plans with the order layout and the part of
// the voxel's orders as a policy: deriv_kernel's generic record (epgx_deriv_kernels.hip.h, the `generic_record` lambda, which
// stays as it is: its kernels keep their code) restated for tiled_deriv_kernel (epgx_tiled.hip).  Stage for stage the same
// expressions in the same order, so that both walk a record to the same bits.
#pragma once
#include "epgx_deriv_kernels.hip.h"

namespace epgx {

// Every stage behind a test of the record's flags (cf. exec_record).  SX: the order layout and the part of the voxel's orders this
// wavefront holds -- NoSplit / Contig: the whole state matrix; Tile (epgx_tiled.hip): a window, where the k = 0 terms --
// equilibrium, recovery, constant terms, the fold of a shift -- are tile 0's (holds_k0, oh0, eqv) and truncation compares
// ORDERS (order_base).
template <int M, int NSP, int V, class SX>
__device__ __forceinline__ void deriv_record(State<M> &s, State<M> (&ds)[V], const Rec &r, const DRec &dr, const_f64_t pool, uint32_t p0,
                                             uint32_t p1, uint32_t p2, uint32_t p3, double &dens, double &eqv, double oh0, int lane,
                                             uint32_t voff0, d2 *sig_base, int64_t signal_ld, int through_plain, d2 *wl,
                                             const double *__restrict__ gpool, const SX &sx = SX()) {
    const uint32_t f = r.flags;
    if (!SX::contig && (f & (F_GS | F_D))) {
        const uint32_t off = entry_offset<NSP>(r.t_off, r.t_ix, p0, p1, p2, p3);
        if (f & F_GS) {
            gather_shift(s, (const int32_t *)((const char *)gpool + off), wl, lane);
#pragma unroll
            for (int j = 0; j < V; ++j) gather_shift(ds[j], (const int32_t *)((const char *)gpool + off), wl, lane);
        }
        if (f & F_D) {
            apply_D(s, (const double *)((const char *)gpool + off), lane);
            if (through_plain) {
#pragma unroll
                for (int j = 0; j < V; ++j) apply_D(ds[j], (const double *)((const char *)gpool + off), lane);
            }
        }
        return;
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
            if (through_plain) {
#pragma unroll
                for (int j = 0; j < V; ++j)
#pragma unroll
                    for (int m = 0; m < M; ++m) ds[j].Ar[m] = ds[j].Ai[m] = ds[j].Br[m] = ds[j].Bi[m] = 0.0;
            }
        }
        if (f & F_PD) {
            dens = ec[0];
            eqv = (lane == 0 && holds_k0(sx)) ? dens : 0.0;
        }
        if (f & (F_RESET | F_PD_RESET)) {
            // always: after Reset the reference keeps stale derivative states of the OLD size and
            // NumPy-broadcasts the next 1-row partial over all their rows (statematrix.py:257-259),
            // which is an accident, not a definition
            set_equilibrium(s, lane, holds_k0(sx) ? dens : 0.0);
#pragma unroll
            for (int j = 0; j < V; ++j) set_zero(ds[j]);
        }
    }
    if (f & F_S0) {
        shift_plain<M, false, SX>(s, lane, oh0);
#pragma unroll
        for (int j = 0; j < V; ++j) shift_plain<M, false, SX>(ds[j], lane, oh0);
    }
    if (f & (F_T | F_MAT)) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (f & F_TX) apply_TX(ds[j], tc); else if (f & F_TY) apply_TY(ds[j], tc); else if (f & F_T) apply_T(ds[j], tc); else apply_MAT(ds[j], tc);
            if (dr.present & (1u << j)) {
                const_f64_t src = entry<NSP>(pool, dr.t_off[j], dr.t_ix[j], p0, p1, p2, p3);
                const f64x8 lo = *(const EPGX_CONSTANT f64x8 *)src;
                const f64x2 hi = *(const EPGX_CONSTANT f64x2 *)(src + 8);
                double dc[10];
#pragma unroll
                for (int q = 0; q < 8; ++q) dc[q] = lo[q];
                dc[8] = hi[0];
                dc[9] = hi[1];
                if (dr.present & (256u << j)) acc_TX(ds[j], s, dc); else acc_MAT(ds[j], s, dc);
            }
            if ((f & F_T0) && (dr.present & (16u << j))) {   // partial of a fused table's constant term
                const f64x4 o = *(const EPGX_CONSTANT f64x4 *)entry<NSP>(pool, dr.e_off[j], dr.e_ix[j], p0, p1, p2, p3);
                acc_C(ds[j], o[0], o[1], o[2], eqv);
            }
        }
        if (f & F_TX) apply_TX(s, tc); else if (f & F_TY) apply_TY(s, tc); else if (f & F_T) apply_T(s, tc); else apply_MAT(s, tc);
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
#pragma unroll
        for (int j = 0; j < V; ++j) {
            // derivative states have no equilibrium term (diff.py:103-109)
            if (f & F_ER) apply_ER(ds[j], ec, 0.0); else apply_E(ds[j], ec, 0.0);
            if (dr.present & (16u << j)) {
                const f64x4 e = *(const EPGX_CONSTANT f64x4 *)entry<NSP>(pool, dr.e_off[j], dr.e_ix[j], p0, p1, p2, p3);
                double dc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) dc[q] = e[q];
                if (dr.present & (4096u << j)) acc_ER(ds[j], s, dc, eqv); else acc_E(ds[j], s, dc, eqv);
            }
        }
        if (f & F_ER) apply_ER(s, ec, eqv); else apply_E(s, ec, eqv);
    }
    if (f & F_S) {
        if constexpr (SX::contig) {      // (shifts by +-1 only: the host keeps other plans on the lane-strided layout)
            if (r.shift == 1) {
                shift_plain<M, false, SX>(s, lane, oh0);
#pragma unroll
                for (int j = 0; j < V; ++j) shift_plain<M, false, SX>(ds[j], lane, oh0);
            } else {
                shift_plain<M, true, SX>(s, lane, oh0);
#pragma unroll
                for (int j = 0; j < V; ++j) shift_plain<M, true, SX>(ds[j], lane, oh0);
            }
        } else {
            shift_any(s, r.shift, wl, lane, oh0);
#pragma unroll
            for (int j = 0; j < V; ++j) shift_any(ds[j], r.shift, wl, lane, oh0);
        }
        if (f & F_TRUNC) {
            truncate_x<M, SX>(s, r.kmax - order_base(sx), lane);
#pragma unroll
            for (int j = 0; j < V; ++j) truncate_x<M, SX>(ds[j], r.kmax - order_base(sx), lane);
        }
    }
    if (f & F_ADC) {
        d2 *dst = sig_base + (int64_t)r.slot * signal_ld;
        const bool z0 = (f & F_ADC_Z) != 0;
        d2 val;
        double zr = s.Zr[0], zi = s.Zi[0];
        asm volatile("" : "+v"(zr), "+v"(zi));
        val.x = z0 ? zr : s.Ar[0];
        val.y = z0 ? zi : s.Ai[0];
        store_lane0(dst, val, voff0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double dzr = ds[j].Zr[0], dzi = ds[j].Zi[0];
            asm volatile("" : "+v"(dzr), "+v"(dzi));
            val.x = z0 ? dzr : ds[j].Ar[0];
            val.y = z0 ? dzi : ds[j].Ai[0];
            store_lane0(dst + (int64_t)(1 + j) * signal_ld, val, voff0);
        }
    }
}

}  // namespace epgx

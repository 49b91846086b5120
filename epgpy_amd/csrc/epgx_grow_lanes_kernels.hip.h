// epgx_grow_lanes_kernels.hip.h -- the growing launch of an echo train with ONE VOXEL PER LANE: a wave owns 64 consecutive voxels,
// the order axis lies in the lane's own registers (and, above the register deck, in the lane's own column of LDS).
//
// rows_grow_kernel (epgx_grow_kernels.hip.h) gives a voxel the 16 lanes of a DPP row.  Its shifts are DPP moves, its phases are
// re-laid out through the LDS crossbar, the coefficients that start a chain are broadcast, and a row computes all of its lanes
// whatever is alive: of the 40 shifts of a 20-echo train shift s has 1 + min(s, 40 - s) live orders, about 240 order x records
// where the rows layout executes 448.  Here a lane walks the same run-folded record list by itself:
//   * `top` (highest populated order, + 1 per S(+1)) and `rem` (shifts left before the last probe, from the host) are
//     wave-uniform scalars; a record execution computes the orders 0 .. min(top, rem) and nothing else -- the order loop is
//     unrolled over the capacity, one scalar compare and branch per order is the skip;
//   * S(+1) is where a cell puts its results: cell j reads F+ from slot j - (leading shift), F- from slot j + (leading shift)
//     and writes F+ to slot j + (trailing shift), F- to slot j - (trailing shift).  The cells run from the top order down, so
//     F+ is in place; an F- result waits one or two cells until the cell that still reads its slot has done so.  No move, no
//     permute, no re-layout;
//   * the coefficients are the lane's own voxel's, loaded once per run of identical records into plain registers;
//   * a probe is one coalesced store of 64 x 16 bytes.
// Every cell is the multiply / FMA chain of the rows cell it stands for (cell_T, cell_TY, cell_TX_sumdiff, cell_E, cell_ER,
// cell_offset; the folded line of fold_value) on the same operands, with a register where the rows code reads the line
// through row_newbcast: the probes are those of rows_grow_kernel -- and so of rows_kernel<., 4, .> -- bit for bit.
//
// Skipped orders.  Orders above min(top, rem) keep stale values or the zeros they started with.  The argument of
// epgx_grow_kernels.hip.h applies unchanged: a coefficient of order k reaches order 0 through k shifts and through nothing
// else, so an order above `rem` is dead, and a live cell reads slots j - 1, j and j + 1 only, all of them live or unpopulated
// one record earlier (`rem` falls by what `top` rises).  Unpopulated slots start at zero (registers and LDS are cleared per
// voxel group) and are never written before a shift populates them: while the window is bounded by `top` every slot holds
// what the full computation holds.  The zero that stands in for an F- result nobody computed lands in a dead slot.
//
// Register deck: EPGX_LANES_DECK orders (12 VGPRs each) live in VGPRs, the orders from there to L - 1 (L: the launch's largest
// live count, <= 24) in 48 * 64 * (L - deck) bytes of dynamic LDS per wave, read and written with 128-bit LDS operations and
// only by record executions whose window reaches them.  One wave per workgroup; no barrier: a lane only ever touches its own
// column.
//
// Record bodies.  The generic body (lanes_cells) takes the chain kinds tk, t0, ek as wave-uniform run-time values and skips
// order by order: every cell is a handful of basic blocks.  The records a train repeats have bodies specialised on their
// shifts AND kinds (EPGX_LANES_BODIES, epgx_lanes_bodies.h; dispatched once per record), which run the cells IN BLOCKS of B:
// block b holds the orders b B .. b B + B - 1.  With the window 0 .. lim, the block lim / B is partial -- its lim % B + 1
// cells go through a per-cell ladder -- and every block below it is one straight-line region of B cells behind a single
// wave-uniform test, in which the compiler interleaves the chains of neighbouring cells and issues the LDS reads of the
// block ahead of the arithmetic.  A full block touches the slots up to its top order + 1 <= lim <= lcap - 1 only, so its
// slot accesses need no test against lcap.  The cells are those of the generic body -- the same function with the kinds
// as constants -- in the same order, top down, and `pend` carries across blocks exactly as it does across cells.
// Invariant: `pend` is zero when the top cell of a window starts (every skipped cell above leaves it at its initial zeros).
// EPGX_LANES_BODY=0 (kernel argument `body`) sends every record through the generic body: same bits, for A/B runs and tests.
//
// Two instantiations per NSP.  rows_grow_lanes_kernel<NSP, false> is the kernel described so far: any eligible list, the generic
// body as the fallback of the dispatch, and with it a 15-double line live next to the state -- a deck of EPGX_LANES_DECK = 14.
// rows_grow_lanes_kernel<NSP, true> runs TRAINS (LanesPlan::train, epgx_planner.cpp): lists in which every record that is not a
// head record has a specialised body.  A head record executes before any shift (top == 0) and has no leading shift: it touches
// order 0 alone and runs ONE cell, lanes_cell_body<D, 0, O, 0>, with the kinds at run time -- its line is dead before the
// next record's line is loaded.  (With a trailing shift it executes once: a second execution would start at top == 1.)
// No generic body, no fallback switch: a body holds the line entries its kinds read and nothing else, and the deck is EPGX_LANES_TRAIN_DECK = 16 (eight one-wave workgroups per CU at L = 21 where deck 14 has
// seven, and half the cells on LDS slots).  The host never sends this kernel a record without a body; if one arrived it would be
// SKIPPED (top and rem unchanged, every window still capped by lcap): wrong probes, no access outside the slots.  The cells,
// their operands and their order are those of the other instantiation: same bits.
#pragma once
#include "epgx_lanes_bodies.h"
#include "epgx_lanes_odd_cells.h"
#include "epgx_rows_kernels.hip.h"

namespace epgx {

#ifndef EPGX_LANES_DECK
#define EPGX_LANES_DECK 14
#endif
#ifndef EPGX_LANES_TRAIN_DECK
#define EPGX_LANES_TRAIN_DECK 16
#endif
constexpr int LANES_CAP = 24;   // orders the unrolled loop covers (lanes_plan, epgx_planner.cpp: L <= 24)

template <int D>
struct LaneDeck {
    double Ar[D], Ai[D], Br[D], Bi[D], Zr[D], Zi[D];
};

// (LaneLine, the line of a record in this lane's registers: epgx_lanes_odd_cells.h)
typedef double lanes_d2 __attribute__((ext_vector_type(2)));

// slot IDX of component `comp` (0 F+, 1 F-, 2 Z): a register pair below the deck, this lane's 16 bytes of LDS above it; slots
// from `lcap` on do not exist: they read as zero and drop what is written
template <int D, int IDX>
__device__ __forceinline__ void lanes_get(const double (&re)[D], const double (&im)[D], const lanes_d2 *lds, int comp, int lcap, double &xr,
                                          double &xi) {
    if constexpr (IDX < D) {
        xr = re[IDX];
        xi = im[IDX];
    } else if constexpr (IDX < LANES_CAP) {
        xr = xi = 0.0;
        if (IDX < lcap) {
            const lanes_d2 v = lds[((IDX - D) * 3 + comp) * 64];
            xr = v.x;
            xi = v.y;
        }
    } else {
        xr = xi = 0.0;
    }
}
template <int D, int IDX>
__device__ __forceinline__ void lanes_put(double (&re)[D], double (&im)[D], lanes_d2 *lds, int comp, int lcap, double xr, double xi) {
    if constexpr (IDX < 0) {
    } else if constexpr (IDX < D) {
        re[IDX] = xr;
        im[IDX] = xi;
    } else if constexpr (IDX < LANES_CAP) {
        if (IDX < lcap) {
            lanes_d2 v;
            v.x = xr;
            v.y = xi;
            lds[((IDX - D) * 3 + comp) * 64] = v;
        }
    }
}

// order J of one record execution [S(+1)? T? E? S(+1)?]: I = leading shift, O = trailing shift.  tk: 0 no rotation, 1 cell_T,
// 2 cell_TX_sumdiff, 3 cell_TY; t0: constant term on order 0 (cell_offset: Re o0 with tk 1 and 3, Im o0 with tk 1 and 2); ek:
// 0 no relaxation, 1 cell_E, 2 cell_ER.  pend: F- results on their way down (see the header)
template <int D, int I, int O, int J>
__device__ __forceinline__ void lanes_cell_body(LaneDeck<D> &s, lanes_d2 *lds, const int lcap, const int tk, const bool t0, const int ek,
                                                const LaneLine &k, double (&pend)[4]) {
    double ar, ai, br, bi, zr, zi;
    lanes_get<D, J + I>(s.Br, s.Bi, lds, 1, lcap, br, bi);
    if constexpr (I == 1 && J == 0) {   // rows_shift: X_0 <- conj(Y_1)
        ar = br;
        ai = -bi;
    } else {
        lanes_get<D, J - I>(s.Ar, s.Ai, lds, 0, lcap, ar, ai);
    }
    lanes_get<D, J>(s.Zr, s.Zi, lds, 2, lcap, zr, zi);
    // the slot this cell has just read takes the F- result that was waiting for it
    if constexpr (I + O == 1) lanes_put<D, J + I>(s.Br, s.Bi, lds, 1, lcap, pend[0], pend[1]);
    if constexpr (I + O == 2) {
        lanes_put<D, J + I>(s.Br, s.Bi, lds, 1, lcap, pend[2], pend[3]);
        pend[2] = pend[0];
        pend[3] = pend[1];
    }
    if (tk == 2) {   // cell_TX_sumdiff (restated as lanes_tx_sumdiff, epgx_lanes_odd_cells.h: calling that function here changes this kernel's schedule)
        const double ur = ar + br, ui = ai + bi, vr = ar - br, vi = ai - bi;
        const double pr = __builtin_fma(-k.c[4], zi, k.c[1] * vr), pi = __builtin_fma(k.c[4], zr, k.c[1] * vi);
        const double nzr = __builtin_fma(-k.c[6], vi, k.c[7] * zr), nzi = __builtin_fma(k.c[6], vr, k.c[7] * zi);
        ar = __builtin_fma(k.c[0], ur, pr);
        br = __builtin_fma(k.c[0], ur, -pr);
        ai = __builtin_fma(k.c[0], ui, pi);
        bi = __builtin_fma(k.c[0], ui, -pi);
        zr = nzr;
        zi = nzi;
    } else if (tk == 3) {   // cell_TY (k.c[3]: Re m02 starts the chains)
        double o_ar = k.c[3] * zr, o_ai = k.c[3] * zi, o_br = k.c[3] * zr, o_bi = k.c[3] * zi, o_zr = k.c[7] * zr, o_zi = k.c[7] * zi;
        o_ar = __builtin_fma(k.c[1], br, o_ar); o_ar = __builtin_fma(k.c[0], ar, o_ar);
        o_ai = __builtin_fma(k.c[1], bi, o_ai); o_ai = __builtin_fma(k.c[0], ai, o_ai);
        o_br = __builtin_fma(k.c[0], br, o_br); o_br = __builtin_fma(k.c[1], ar, o_br);
        o_bi = __builtin_fma(k.c[0], bi, o_bi); o_bi = __builtin_fma(k.c[1], ai, o_bi);
        o_zr = __builtin_fma(k.c[5], br, o_zr); o_zr = __builtin_fma(k.c[5], ar, o_zr);
        o_zi = __builtin_fma(k.c[5], bi, o_zi); o_zi = __builtin_fma(k.c[5], ai, o_zi);
        ar = o_ar; ai = o_ai; br = o_br; bi = o_bi; zr = o_zr; zi = o_zi;
    } else if (tk == 1) {   // cell_T
        double o_ar = -k.c[4] * zi, o_ai = k.c[4] * zr, o_br = k.c[4] * zi, o_bi = -k.c[4] * zr, o_zr = k.c[7] * zr, o_zi = k.c[7] * zi;
        o_ar = __builtin_fma(k.c[3], zr, o_ar); o_ar = __builtin_fma(-k.c[2], bi, o_ar); o_ar = __builtin_fma(k.c[1], br, o_ar); o_ar = __builtin_fma(k.c[0], ar, o_ar);
        o_ai = __builtin_fma(k.c[3], zi, o_ai); o_ai = __builtin_fma(k.c[2], br, o_ai); o_ai = __builtin_fma(k.c[1], bi, o_ai); o_ai = __builtin_fma(k.c[0], ai, o_ai);
        o_br = __builtin_fma(k.c[3], zr, o_br); o_br = __builtin_fma(k.c[0], br, o_br); o_br = __builtin_fma(k.c[2], ai, o_br); o_br = __builtin_fma(k.c[1], ar, o_br);
        o_bi = __builtin_fma(k.c[3], zi, o_bi); o_bi = __builtin_fma(k.c[0], bi, o_bi); o_bi = __builtin_fma(-k.c[2], ar, o_bi); o_bi = __builtin_fma(k.c[1], ai, o_bi);
        o_zr = __builtin_fma(k.c[6], bi, o_zr); o_zr = __builtin_fma(k.c[5], br, o_zr); o_zr = __builtin_fma(-k.c[6], ai, o_zr); o_zr = __builtin_fma(k.c[5], ar, o_zr);
        o_zi = __builtin_fma(-k.c[6], br, o_zi); o_zi = __builtin_fma(k.c[5], bi, o_zi); o_zi = __builtin_fma(k.c[6], ar, o_zi); o_zi = __builtin_fma(k.c[5], ai, o_zi);
        ar = o_ar; ai = o_ai; br = o_br; bi = o_bi; zr = o_zr; zi = o_zi;
    }
    if constexpr (J == 0) {   // cell_offset: (o0, conj o0, o2) * equilibrium, density 1
        if (t0) {
            if (tk != 2) {
                ar = __builtin_fma(k.c[12], 1.0, ar);
                br = __builtin_fma(k.c[12], 1.0, br);
            }
            if (tk != 3) {
                ai = __builtin_fma(k.c[13], 1.0, ai);
                bi = __builtin_fma(-k.c[13], 1.0, bi);
            }
            zr = __builtin_fma(k.c[14], 1.0, zr);
        }
    }
    if (ek == 1) {   // cell_E
        const double ei = k.c[9], er = k.c[8];
        double o_ar = -ei * ai, o_ai = ei * ar, o_br = ei * bi, o_bi = -ei * br;
        o_ar = __builtin_fma(er, ar, o_ar);
        o_ai = __builtin_fma(er, ai, o_ai);
        o_br = __builtin_fma(er, br, o_br);
        o_bi = __builtin_fma(er, bi, o_bi);
        ar = o_ar; ai = o_ai; br = o_br; bi = o_bi;
    } else if (ek == 2) {   // cell_ER
        ar = k.c[8] * ar; ai = k.c[8] * ai; br = k.c[8] * br; bi = k.c[8] * bi;
    }
    if (ek) {
        zi = k.c[10] * zi;
        if constexpr (J == 0) zr = __builtin_fma(k.c[10], zr, k.c[11] * 1.0); else zr = k.c[10] * zr;
    }
    lanes_put<D, J + O>(s.Ar, s.Ai, lds, 0, lcap, ar, ai);
    lanes_put<D, J>(s.Zr, s.Zi, lds, 2, lcap, zr, zi);
    if constexpr (I + O == 0) {
        lanes_put<D, J>(s.Br, s.Bi, lds, 1, lcap, br, bi);
    } else {
        pend[0] = br;
        pend[1] = bi;
    }
}

// the generic body: one scalar compare and branch per order is the skip
template <int D, int I, int O, int J>
__device__ __forceinline__ void lanes_cell(LaneDeck<D> &s, lanes_d2 *lds, const int lcap, const int lim, const int tk, const bool t0,
                                           const int ek, const LaneLine &k, double (&pend)[4]) {
    if (J > lim) return;
    lanes_cell_body<D, I, O, J>(s, lds, lcap, tk, t0, ek, k, pend);
}

// the blocked body: block BLK = the orders BLK * B .. BLK * B + B - 1, tb = lim / B the partial block.  TK, T0, EK are
// compile-time constants: inlined into the cell, they leave the one chain the record runs and the line entries it reads
template <int D, int I, int O, int TK, bool T0, int EK, int B, int BLK, int... Cs>
__device__ __forceinline__ void lanes_block(LaneDeck<D> &s, lanes_d2 *lds, const int lcap, const int lim, const int tb, const LaneLine &k,
                                            double (&pend)[4], std::integer_sequence<int, Cs...>) {
    if (tb < BLK) return;
    if (B == 1 || tb == BLK) {   // the top of the window: cell by cell, slots tested against lcap
        (lanes_cell<D, I, O, BLK * B + B - 1 - Cs>(s, lds, lcap, lim, TK, T0, EK, k, pend), ...);
    } else {                     // a full block: straight line, every slot exists (header)
        (lanes_cell_body<D, I, O, BLK * B + B - 1 - Cs>(s, lds, LANES_CAP, TK, T0, EK, k, pend), ...);
    }
}
template <int D, int I, int O, int TK, bool T0, int EK, int B, int... Bs>
__device__ __forceinline__ void lanes_blocks(LaneDeck<D> &s, lanes_d2 *lds, int lcap, int lim, const LaneLine &k, double (&pend)[4],
                                             std::integer_sequence<int, Bs...>) {
    static_assert(LANES_CAP % B == 0 && (B & (B - 1)) == 0, "whole blocks, a power of two");
    constexpr int NB = LANES_CAP / B;
    const int tb = lim / B;
    (lanes_block<D, I, O, TK, T0, EK, B, NB - 1 - Bs>(s, lds, lcap, lim, tb, k, pend, std::make_integer_sequence<int, B>()), ...);
}

template <int D, int I, int O, int... Js>
__device__ __forceinline__ void lanes_cells(LaneDeck<D> &s, lanes_d2 *lds, int lcap, int lim, int tk, bool t0, int ek, const LaneLine &k,
                                            double (&pend)[4], std::integer_sequence<int, Js...>) {
    (lanes_cell<D, I, O, LANES_CAP - 1 - Js>(s, lds, lcap, lim, tk, t0, ek, k, pend), ...);   // from the top order down
}

// one record execution on the orders 0 .. lim.  B == 0: the generic body, the kinds tk, t0, ek at run time; B > 0: blocks
// of B cells specialised on TK, T0, EK; B < 0: a head record (no leading shift, top == 0, so lim <= 0): the cell of order 0,
// kinds at run time
template <int D, int I, int O, int B, int TK, bool T0, int EK>
__device__ __forceinline__ void lanes_record(LaneDeck<D> &s, lanes_d2 *lds, int lcap, int lim, int tk, bool t0, int ek, const LaneLine &k) {
    if (lim < 0) return;   // (behind the last probe)
    double pend[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (B < 0) {
        static_assert(I == 0, "a head record has no leading shift");
        lanes_cell_body<D, 0, O, 0>(s, lds, lcap, tk, t0, ek, k, pend);
    } else if constexpr (B == 0)
        lanes_cells<D, I, O>(s, lds, lcap, lim, tk, t0, ek, k, pend, std::make_integer_sequence<int, LANES_CAP>());
    else
        lanes_blocks<D, I, O, TK, T0, EK, B>(s, lds, lcap, lim, k, pend, std::make_integer_sequence<int, LANES_CAP / B>());
    if constexpr (I == 1) {   // the F- result of order O has no reader left: slot 0
        s.Br[0] = pend[2 * O];
        s.Bi[0] = pend[2 * O + 1];
    }
    if constexpr (O == 1) {   // rows_shift: X_0 <- conj(Y_1), the new Y_0
        s.Ar[0] = s.Br[0];
        s.Ai[0] = -s.Bi[0];
    }
}

// this lane's line of record r: the table entries of its voxel, or -- F_FOLD -- E_a . T . E_b computed as fold_value does
template <int NSP>
__device__ __forceinline__ void lanes_line(const Rec &r, const __amdgpu_buffer_rsrc_t pool, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3,
                                           int tk, LaneLine &k) {
    const uint32_t f = r.flags;
#pragma unroll
    for (int j = 0; j < 15; ++j) k.c[j] = 0.0;
    if (f & F_T) {
        const uint32_t te = lane_entry<NSP>(r.t_off, r.t_ix, p0, p1, p2, p3);
        pool_f64x2(pool, te, k.c[0], k.c[1]);
        pool_f64x2(pool, te + 16u, k.c[2], k.c[3]);
        pool_f64x2(pool, te + 32u, k.c[4], k.c[5]);
        pool_f64x2(pool, te + 48u, k.c[6], k.c[7]);
        if ((f & F_T0) && !(f & F_FOLD)) {
            pool_f64x2(pool, te + 64u, k.c[12], k.c[13]);
            k.c[14] = pool_f64(pool, te + 80u);
        }
    }
    if (f & F_FOLD) {
        const uint32_t ae = lane_entry<NSP>(r.e_off, r.e_ix, p0, p1, p2, p3);
        const uint32_t be = lane_entry<NSP>((uint32_t)r.shift, fold_b_ix(f), p0, p1, p2, p3);
        double ae0, ae1, ae2, ae3, be0, be1, be2, be3;
        pool_f64x2(pool, ae, ae0, ae1);
        pool_f64x2(pool, ae + 16u, ae2, ae3);
        pool_f64x2(pool, be, be0, be1);
        pool_f64x2(pool, be + 16u, be2, be3);
        (void)ae1;
        (void)be1;
        // c'_j = fma(E_a[asel_j], T[tsel_j] * E_b[bsel_j], j == 14 ? r_a : 0): the table of fold_selectors
        const double t3 = k.c[3], t4 = k.c[4], t7 = k.c[7];
        k.c[0] = __builtin_fma(ae0, k.c[0] * be0, 0.0);
        k.c[1] = __builtin_fma(ae0, k.c[1] * be0, 0.0);
        k.c[2] = __builtin_fma(ae0, k.c[2] * be0, 0.0);
        k.c[3] = __builtin_fma(ae0, t3 * be2, 0.0);
        k.c[4] = __builtin_fma(ae0, t4 * be2, 0.0);
        k.c[5] = __builtin_fma(ae2, k.c[5] * be0, 0.0);
        k.c[6] = __builtin_fma(ae2, k.c[6] * be0, 0.0);
        k.c[7] = __builtin_fma(ae2, t7 * be2, 0.0);
        k.c[12] = __builtin_fma(ae0, t3 * be3, 0.0);
        k.c[13] = __builtin_fma(ae0, t4 * be3, 0.0);
        k.c[14] = __builtin_fma(ae2, t7 * be3, ae3);
    } else if (f & F_E) {
        const uint32_t ee = lane_entry<NSP>(r.e_off, r.e_ix, p0, p1, p2, p3);
        pool_f64x2(pool, ee, k.c[8], k.c[9]);
        pool_f64x2(pool, ee + 16u, k.c[10], k.c[11]);
    }
    if (tk == 2) {   // line_bcasts: the sum / difference form of a rotation about x
        const double m00 = k.c[0], m01 = k.c[1];
        k.c[0] = 0.5 * (m00 + m01);
        k.c[1] = 0.5 * (m00 - m01);
    }
}

// `rep` executions of record r, probes to consecutive rows.  The line is loaded once, here and not in front of the dispatch:
// a specialised body then holds the entries it reads and nothing else
template <int NSP, int D, int I, int O, int B = 0, int TK = 0, bool T0 = false, int EK = 0>
__device__ __forceinline__ void lanes_run(LaneDeck<D> &s, lanes_d2 *lds, const int lcap, const Rec &r, const int rep, int &top, int &rem, const int tk,
                                          const bool t0, const int ek, const __amdgpu_buffer_rsrc_t pool, const uint32_t p0, const uint32_t p1,
                                          const uint32_t p2, const uint32_t p3, d2 *sig_base, const int64_t signal_ld, const int nvalid,
                                          const uint32_t voff) {
    LaneLine k;
    lanes_line<NSP>(r, pool, p0, p1, p2, p3, tk, k);
    int slot = r.slot;
    for (int e = 0; e < rep; ++e, ++slot) {
        // the cells work between the record's two shifts: top + I orders are populated there, rem - I shifts are left
        int lim = top + I < rem - I ? top + I : rem - I;
        lim = lim < lcap - 1 ? lim : lcap - 1;   // (never beyond the slots the launch has, whatever the host passed)
        lanes_record<D, I, O, B, TK, T0, EK>(s, lds, lcap, lim, tk, t0, ek, k);
        top += I + O;
        rem -= I + O;
        if (r.flags & F_ADC) {
            u32x4 bits;
            bits.x = (uint32_t)__double2loint(s.Ar[0]); bits.y = (uint32_t)__double2hiint(s.Ar[0]);
            bits.z = (uint32_t)__double2loint(s.Ai[0]); bits.w = (uint32_t)__double2hiint(s.Ai[0]);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(sig_base + (int64_t)slot * signal_ld, 0, 16 * nvalid, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(bits, rs, voff, 0, 0);
        }
    }
}

// rem0: the shifts of the list up to its last probe; lcap: L, the slots a lane has (deck + LDS); body: 0 the generic body for
// every record, else the specialised bodies where they exist.  n1, n2 and the capacities of rows_grow_kernel's ranges are not
// used: the window follows top and rem record by record.  TRAIN: head records and specialised bodies only, on its own deck
// (header); `body` is not read there -- the launcher sends EPGX_LANES_BODY=0 to the other instantiation
template <int NSP, bool TRAIN>
__global__ void __launch_bounds__(64, 2) rows_grow_lanes_kernel(const int64_t nvox, const Rec *__restrict__ recs_, const double *__restrict__ coef_,
                                                               d2 *__restrict__ signal, const int64_t signal_ld, const RunTail a, const int rem0,
                                                               const int lcap, const int body) {
    constexpr int D = TRAIN ? EPGX_LANES_TRAIN_DECK : EPGX_LANES_DECK;
    extern __shared__ __attribute__((aligned(16))) lanes_d2 lanes_lds[];
    const int lane = threadIdx.x & 63;
    const const_rec_t recs = (const_rec_t)(uintptr_t)recs_;
    const __amdgpu_buffer_rsrc_t pool = __builtin_amdgcn_make_buffer_rsrc((void *)coef_, 0, 0x7fffffff, 0x00020000);
    lanes_d2 *lds = lanes_lds + lane;
    const int n_rec = a.n_rec;
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const int64_t v0 = (int64_t)b * 64;
        if (v0 >= nvox) break;
        uint32_t p0, p1, p2, p3;
        rows_indices<NSP>(a, nvox, v0, lane, p0, p1, p2, p3);   // (tail lanes shadow the last voxel, never store)
        const int nvalid = (int)(nvox - v0 < 64 ? nvox - v0 : 64);
        const uint32_t voff = 16u * (uint32_t)lane;
        d2 *sig_base = signal + v0;
        LaneDeck<D> s;
#pragma unroll
        for (int j = 0; j < D; ++j) s.Ar[j] = s.Ai[j] = s.Br[j] = s.Bi[j] = s.Zr[j] = s.Zi[j] = 0.0;
        s.Zr[0] = 1.0;
        for (int j = D; j < lcap; ++j) {
            lanes_d2 z;
            z.x = z.y = 0.0;
            lds[((j - D) * 3 + 0) * 64] = z;
            lds[((j - D) * 3 + 1) * 64] = z;
            lds[((j - D) * 3 + 2) * 64] = z;
        }
        int top = 0, rem = rem0, members = 0;
        for (int i = 0; i < n_rec; ++i) {
            const Rec r = load_rec(recs, i);
            const uint32_t f = r.flags, head = f >> 24;
            const int count = (int)((uint32_t)r.kmax >> 16);
            if (!members && (head == LEAF_PAIR || head == LEAF_SINGLE)) {   // a run header: its members follow, one execution each
                members = (head == LEAF_PAIR ? 2 : 1) * count;
                continue;
            }
            const int rep = members ? 1 : (count > 1 ? count : 1);
            if (members) --members;
            // the chains the rows code runs for this record: rows_T / rows_generic (a record without a leaf runs the plain chains)
            const int tk = lanes_tk(f, head);
            const bool t0 = (f & F_T0) != 0;
            const int ek = lanes_ek(f);
            if constexpr (TRAIN) {
                if (top == 0 && !(f & F_S0) && (!(f & F_S) || rep == 1)) {   // a head record (as lanes_plan decides it)
                    if (f & F_S)
                        lanes_run<NSP, D, 0, 1, -1>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff);
                    else
                        lanes_run<NSP, D, 0, 0, -1>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff);
                    continue;
                }
                switch (lanes_body_id(f, head)) {
#define EPGX_LANES_CASE(id, I, O, TK, T0, EK, B, name) \
    case id: lanes_run<NSP, D, I, O, B, TK, T0, EK>(s, lds, lcap, r, rep, top, rem, TK, T0, EK, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); break;
                    EPGX_LANES_BODIES(EPGX_LANES_CASE)
#undef EPGX_LANES_CASE
                default: break;   // (no body: not a train -- skipped, see the header)
                }
                continue;
            }
            switch (body ? lanes_body_id(f, head) : -1) {
#define EPGX_LANES_CASE(id, I, O, TK, T0, EK, B, name) \
    case id: lanes_run<NSP, D, I, O, B, TK, T0, EK>(s, lds, lcap, r, rep, top, rem, TK, T0, EK, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); continue;
                EPGX_LANES_BODIES(EPGX_LANES_CASE)
#undef EPGX_LANES_CASE
            default: break;
            }
            switch (((f & F_S0) ? 2 : 0) | ((f & F_S) ? 1 : 0)) {
            case 0: lanes_run<NSP, D, 0, 0>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); break;
            case 1: lanes_run<NSP, D, 0, 1>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); break;
            case 2: lanes_run<NSP, D, 1, 0>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); break;
            default: lanes_run<NSP, D, 1, 1>(s, lds, lcap, r, rep, top, rem, tk, t0, ek, pool, p0, p1, p2, p3, sig_base, signal_ld, nvalid, voff); break;
            }
        }
    }
}

}  // namespace epgx

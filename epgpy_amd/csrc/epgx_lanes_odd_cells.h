// epgx_lanes_odd_cells.h -- the cells of rows_grow_lanes_kernel_odd (epgx_grow_lanes_odd_kernels.hip.h): one execution of the
// folded echo S(+1) . T0 . S(+1) on the orders that can reach an echo.  Plain C++ next to the device code: the same functions
// compile for the host (tests/host/lanes_odd_cells_check.cpp walks them under a sanitizer), and the line and the chain of a
// rotation about x are those of rows_grow_lanes_kernel (epgx_grow_lanes_kernels.hip.h), which includes this file for the line.
//
// The parity rule.  Between two refocusing pulses of a train that repeats S(+1) . X . S(+1) the F states move by two orders and
// Z by none, and a rotation mixes F+(k), F-(k), Z(k) of one k: the orders that are odd when the pulse acts and the even ones
// never exchange anything.  A probe reads F0 behind the trailing shift -- F-(1) at the pulse -- and the excitation enters the
// odd class through the first shift; the even class holds what recovery feeds into Z0 and its descendants, and no probe sees it.
// In the slots of rows_grow_lanes_kernel, cell j of such a record reads F+ slot j - 1, F- slot j + 1, Z slot j and writes F+
// slot j + 1, Z slot j, F- slot j - 1: the odd cells live on {F slots of even index, Z slots of odd index} and the probe is F+
// slot 0.  Cell 0 is even, and the constant term of the rotation (cell_offset) with it.
//
// Compact state.  Cell m stands for cell j = 2 m + 1; P[m] = F+ slot 2 m, Q[m] = F- slot 2 m, Z[m] = Z slot 2 m + 1.  Cell m
// reads P[m], Q[m + 1], Z[m] and writes P[m + 1], Z[m]; its F- result belongs in Q[m], which cell m - 1 still has to read: it
// waits in `pend` for one cell.  The window 0 .. lim of the full kernel (lim = min(top + 1, rem - 1), odd here: top and rem are
// even) is the cells (lim - 1) / 2 .. 0, from the top down, (lim + 1) / 2 of them where the full kernel runs lim + 1.
// Capacity C: the cells 0 .. C - 1 on P, Q, Z[0 .. C - 1], all in registers.  The slots P[C] and Q[C] do not exist: Q[C] reads
// as zero (only a cell C could have written it), what cell C - 1 would put into P[C] is dropped (only a cell C could read
// it).  A launch whose largest live count is L opens windows up to lim = L - 1 (L even) or L - 2: C >= L / 2 holds them.
// The window is clamped to C whatever the caller passes: no index depends on a run-time value.
//
// Same bits: a cell is the chain of the full kernel's cell 2 m + 1 on the same operands, and the full kernel's even cells
// write nothing an odd cell reads.
#pragma once
#include <utility>

#if defined(__HIPCC__)
#define EPGX_LANES_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EPGX_LANES_HD inline
#endif

namespace epgx {

// the line of a record in this lane's registers, indexed like the coefficient line of the rows layout (epgx_packed_kernels.hip.h):
// 0 c00  1 pr  2 pi  3 qr  4 qi  5 tr  6 ti  7 c22 | 8 er  9 ei  10 e2  11 r0 | 12 Re o0  13 Im o0  14 o2; a rotation about x
// keeps (m00 + m01) / 2 and (m00 - m01) / 2 in slots 0 and 1 (line_bcasts, EPGX_SUMDIFF)
struct LaneLine {
    double c[15];
};

// cell_TX_sumdiff on (F+, F-, Z) of one order: the chain of a rotation about x in the sum / difference form (line entries 0, 1,
// 4, 6, 7).  The statements of lanes_cell_body's tk == 2 branch, verbatim and in its operand order; that kernel keeps its own
// copy: routed through this function its cells compute the same but are scheduled differently, and its listing was to stay
EPGX_LANES_HD void lanes_tx_sumdiff(const LaneLine &k, double &ar, double &ai, double &br, double &bi, double &zr, double &zi) {
    const double ur = ar + br, ui = ai + bi, vr = ar - br, vi = ai - bi;
    const double pr = __builtin_fma(-k.c[4], zi, k.c[1] * vr), pi = __builtin_fma(k.c[4], zr, k.c[1] * vi);
    const double nzr = __builtin_fma(-k.c[6], vi, k.c[7] * zr), nzi = __builtin_fma(k.c[6], vr, k.c[7] * zi);
    ar = __builtin_fma(k.c[0], ur, pr);
    br = __builtin_fma(k.c[0], ur, -pr);
    ai = __builtin_fma(k.c[0], ui, pi);
    bi = __builtin_fma(k.c[0], ui, -pi);
    zr = nzr;
    zi = nzi;
}

constexpr int LANES_ODD_BLOCK = 4;                       // cells per straight-line block
constexpr int lanes_odd_cells(int L) { return L / 2; }   // the cells a launch with L live orders can open (header)

template <int C>
struct LaneOdd {
    double Pr[C], Pi[C], Qr[C], Qi[C], Zr[C], Zi[C];
};

template <int C, int M>
EPGX_LANES_HD void lanes_odd_cell_body(LaneOdd<C> &s, const LaneLine &k, double (&pend)[2]) {
    if constexpr (M < C) {
        double ar = s.Pr[M], ai = s.Pi[M], br = 0.0, bi = 0.0, zr = s.Zr[M], zi = s.Zi[M];
        if constexpr (M + 1 < C) {
            br = s.Qr[M + 1];
            bi = s.Qi[M + 1];
            // the slot this cell has just read takes the F- result that was waiting for it
            s.Qr[M + 1] = pend[0];
            s.Qi[M + 1] = pend[1];
        }
        lanes_tx_sumdiff(k, ar, ai, br, bi, zr, zi);
        if constexpr (M + 1 < C) {
            s.Pr[M + 1] = ar;
            s.Pi[M + 1] = ai;
        }
        s.Zr[M] = zr;
        s.Zi[M] = zi;
        pend[0] = br;
        pend[1] = bi;
    }
}
template <int C, int M>
EPGX_LANES_HD void lanes_odd_cell(LaneOdd<C> &s, const int mtop, const LaneLine &k, double (&pend)[2]) {
    if (M > mtop) return;
    lanes_odd_cell_body<C, M>(s, k, pend);
}

// block BLK = the cells BLK * B .. BLK * B + B - 1, tb = mtop / B the partial block: its cells go through a ladder, every
// block below it is one straight-line region behind a single test
template <int C, int B, int BLK, int... Cs>
EPGX_LANES_HD void lanes_odd_block(LaneOdd<C> &s, const int mtop, const int tb, const LaneLine &k, double (&pend)[2],
                                   std::integer_sequence<int, Cs...>) {
    if (tb < BLK) return;
    if (tb == BLK) {
        (lanes_odd_cell<C, BLK * B + B - 1 - Cs>(s, mtop, k, pend), ...);
    } else {
        (lanes_odd_cell_body<C, BLK * B + B - 1 - Cs>(s, k, pend), ...);
    }
}
template <int C, int B, int... Bs>
EPGX_LANES_HD void lanes_odd_blocks(LaneOdd<C> &s, const int mtop, const LaneLine &k, double (&pend)[2], std::integer_sequence<int, Bs...>) {
    constexpr int NB = (int)sizeof...(Bs);
    const int tb = mtop / B;
    (lanes_odd_block<C, B, NB - 1 - Bs>(s, mtop, tb, k, pend, std::make_integer_sequence<int, B>()), ...);
}

// one execution of the folded echo on the window 0 .. lim of the full kernel.  lim < 1: behind the last probe (or a window the
// parity rule cannot produce): nothing runs.  `pend` is zero when the top cell starts, as in the full kernel
template <int C>
EPGX_LANES_HD void lanes_odd_record(LaneOdd<C> &s, const int lim, const LaneLine &k) {
    constexpr int B = LANES_ODD_BLOCK;
    if (lim < 1) return;
    int mtop = (lim - 1) >> 1;
    mtop = mtop < C - 1 ? mtop : C - 1;   // (never beyond the cells this instantiation has, whatever the host passed)
    double pend[2] = {0.0, 0.0};
    lanes_odd_blocks<C, B>(s, mtop, k, pend, std::make_integer_sequence<int, (C + B - 1) / B>());
    // the F- result of cell 0 has no reader left: F- slot 0; then rows_shift: X_0 <- conj(Y_1), the new Y_0
    s.Qr[0] = pend[0];
    s.Qi[0] = pend[1];
    s.Pr[0] = s.Qr[0];
    s.Pi[0] = -s.Qi[0];
}

}  // namespace epgx

// epgx_grow_kernels.hip.h -- state-resident launches from equilibrium whose state matrix GROWS: the rows layout (four voxels
// per wavefront, R orders per lane) walked in phases of R = 1, 2, 4 -- and of fewer again where fewer orders still matter.
//
// The reference starts simulate() with ONE order and lets every S(+-1) add one (functions.py:135, shift.py:86: the state
// matrix is resized as it grows, `max_nstate` only caps it) -- at echo n of a spin-echo train 2 n + 1 of the 64 orders exist.
// rows_kernel<., 4, .> computes all 64 from the first record on: over a 20-echo train 80 order slots per lane where 43 hold
// anything.  Here the host cuts the (run-length folded) record list where the populated orders outgrow 16 and 32
// (grow_split, epgx_planner.cpp), and a wave walks
//      records [0, n1)  with r0 orders per lane   (1: the rows code at R = 1, 16 orders),
//      records [n1, n2) with r1                   (1 or 2: 32 orders),
//      the rest         with r2                   (1, 2 or 4: 64 orders),
// re-laying the state out between the phases (order k moves from lane k / R, slot k % R to lane k / 2R, slot k % 2R of its
// voxel's row, or back: lane permutations through the LDS crossbar, once per step).  Every record runs the same leaf code as in
// rows_kernel on the orders that exist; orders that do not exist are exactly zero there and stay zero under every operator
// of this kernel (rotations, relaxation: products with zero; the recovery term touches order 0 only), so the results are
// those of rows_kernel<., 4, .> bit for bit.
//
// A range runs BELOW 16 / 32 / 64 orders where the populated orders no longer fit but the orders that can still reach a probe
// do (grow_reach, epgx_planner.cpp).  This kernel writes no state: its outputs are the order-0 probes, and a coefficient of order k
// gets to order 0 through k shifts and through nothing else.  With `rem` shifts left before the last probe the orders above
// `rem` are dead; the host gives a range C orders only if, at every record of it, min(highest populated order, rem) <= C - 1.
// Narrowing drops dead orders only.  Behind it the zero that a shift feeds in at the top lane (row_shr / row_shl) stands for
// order C, which is dead before that shift, and lands in order C - 1, which is dead after it (one shift fewer remains); from
// there a wrong value comes down one order per shift, always above what is left of `rem`.  No live order ever reads a dropped
// one, every live order goes through the same operations on the same operands, and the probes are those of
// rows_kernel<., 4, .> bit for bit still.
#pragma once
#include "epgx_rows_kernels.hip.h"

namespace epgx {

// n1 <= n2 <= a.n_rec: records [0, n1) run with r0 orders per lane (16 r0 per voxel), [n1, n2) with r1, the rest with r2;
// r0, r1, r2 in {1, 2, 4}
#ifndef EPGX_GROW_WPB
#define EPGX_GROW_WPB 4      // wavefronts per workgroup (x 4 voxels each)
#endif
#ifdef EPGX_GROW_TIMING
__device__ unsigned long long g_stamp[(1 << 19) * 8];
#define EPGX_STAMP(i) do { if (lane == 0) g_stamp[(size_t)(v0 >> 2) * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define EPGX_STAMP(i) do { } while (0)
#endif
template <int NSP>
__global__ void __launch_bounds__(64 * EPGX_GROW_WPB, EPGX_R4_RUNS_WAVES) rows_grow_kernel(const int64_t nvox, const Rec *__restrict__ recs_,
                                                                           const double *__restrict__ coef_, d2 *__restrict__ signal,
                                                                           const int64_t signal_ld, const RunTail a, const int n1, const int n2,
                                                                           const int r0, const int r1, const int r2) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k16 = lane & 15, sub = lane >> 4;
    const const_rec_t recs = (const_rec_t)(uintptr_t)recs_;
    const __amdgpu_buffer_rsrc_t pool = __builtin_amdgcn_make_buffer_rsrc((void *)coef_, 0, 0x7fffffff, 0x00020000);
    const bool is_e = k16 >= 8 && k16 < 12;       // (the coefficient line of a row: as in rows_kernel)
    const uint32_t col = 8u * (uint32_t)(k16 < 8 ? k16 : (k16 < 12 ? k16 - 8 : k16 - 4));
    const FoldSel fs = fold_selectors(k16);
    const double oh0 = (k16 == 0) ? 1.0 : 0.0;
    const int n_rec = a.n_rec;
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const int64_t v0 = ((int64_t)b * EPGX_GROW_WPB + wib) * 4;
        if (v0 >= nvox) continue;
        EPGX_STAMP(0);
        uint32_t p0, p1, p2, p3;
        rows_indices<NSP>(a, nvox, v0, lane_now() >> 4, p0, p1, p2, p3);
        double dens = 1.0;
        double eqv = oh0 * dens;
        const int64_t nvalid = nvox - v0 < 4 ? nvox - v0 : 4;
        const uint32_t voff = (k16 == 0) ? (uint32_t)sub * 16u : 0x7fffff00u;
        d2 *sig_base = signal + v0;
        Rec ra = load_rec(recs, 0);     // (handed from phase to phase: only the first record of the list is waited for)
        double cta = load_line_t<NSP>(ra, pool, is_e, col, fs, p0, p1, p2, p3);
#ifdef EPGX_GROW_TIMING
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        EPGX_STAMP(1);
        if (lane == 0) { g_stamp[(size_t)(v0 >> 2) * 8 + 7] = ((unsigned long long)__builtin_amdgcn_s_getreg(63492) << 32) | b; }   // HW_ID[31:0]
#endif
        // The capacities the host can give (grow_reach): r0 = 1, r1 = 1 or 2, r2 = 1, 2 or 4 -- four orders per lane only ever
        // in the LAST range.  So the ranges at one and two orders per lane are walked in a loop over ONE pair of state slots (each
        // R keeps a single call site of the walk, which expands the whole leaf dispatch; a range that keeps the capacity of the
        // one before it converts nothing), and a last range at four follows the loop as it followed the growing phases before:
        // nothing of the loop is alive across it
        State<2> st;
        rows_equilibrium<2>(st, eqv);
        int cur = 1, i0 = 0;
#pragma nounroll
        for (int ph = 0; ph < 3; ++ph) {
            const int i1 = ph == 0 ? n1 : (ph == 1 ? n2 : n_rec);
            const int r = ph == 0 ? r0 : (ph == 1 ? r1 : r2);
            const int want = r < 2 ? r : 2;                  // (r = 4: the state is brought to two orders per lane here)
            if (i1 > i0 && cur != want) {
                if (want == 2) {
                    State<1> s1;
                    rows_slots(st, s1);
                    rows_widen<1>(s1, st, k16);
                } else {
                    State<1> s1;
                    rows_narrow<1>(st, s1, k16);
                    rows_slots(s1, st);
                }
                cur = want;
            }
            if (ph) EPGX_STAMP(1 + 2 * ph);
            if (r == 4) break;
            if (i1 > i0) {
                if (want == 1) {
                    State<1> s1;
                    rows_slots(st, s1);
                    rows_walk_runs<NSP, 1>(s1, i0, i1, ra, cta, recs, pool, is_e, col, fs, p0, p1, p2, p3, dens, eqv, oh0, k16, sig_base, signal_ld, nvalid, voff);
                    rows_slots(s1, st);
                } else {
                    rows_walk_runs<NSP, 2>(st, i0, i1, ra, cta, recs, pool, is_e, col, fs, p0, p1, p2, p3, dens, eqv, oh0, k16, sig_base, signal_ld, nvalid, voff);
                }
                i0 = i1;
            }
            EPGX_STAMP(2 + 2 * ph);
        }
        if (i0 < n_rec) {
            State<4> s4;
            rows_widen<2>(st, s4, k16);
            EPGX_STAMP(5);
            rows_walk_runs<NSP, 4>(s4, i0, n_rec, ra, cta, recs, pool, is_e, col, fs, p0, p1, p2, p3, dens, eqv, oh0, k16, sig_base, signal_ld, nvalid, voff);
            EPGX_STAMP(6);
        }
    }
}

}  // namespace epgx

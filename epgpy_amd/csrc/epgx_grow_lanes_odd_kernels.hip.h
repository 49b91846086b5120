// epgx_grow_lanes_odd_kernels.hip.h -- rows_grow_lanes_kernel_odd: the growing launch of an echo train with one voxel per lane,
// computing ONLY THE ORDERS WHOSE PARITY REACHES AN ECHO (LanesPlan::odd, epgx_planner.h; the rule and the compact state:
// epgx_lanes_odd_cells.h).
//
// The launch is that of rows_grow_lanes_kernel<NSP, true> (epgx_grow_lanes_kernels.hip.h): one wave per workgroup, 64
// consecutive voxels, the grid-stride loop, rows_indices, lanes_line, the probes as buffer stores, `top` and `rem` counted
// record by record.  What differs:
//   * head records (before any shift, no shift of their own: `odd` allows no other) run their one cell of order 0 on
//     (F+0, F-0, Z0) exactly as there -- lanes_cell_body<1, 0, 0, 0>, kinds at run time.  F+0 and F-0 are slot 0 of the
//     compact state; Z0 belongs to the even class and is dead once the head phase ends;
//   * an execution of the folded echo runs lanes_odd_record: half the cells, none of order 0, no constant term -- the line
//     is the five entries cell_TX_sumdiff reads;
//   * the whole state of C cells is 12 C VGPRs.  No LDS, no slot test at run time;
//   * a record that is neither is SKIPPED (top and rem unchanged): the host never sends one; wrong probes, no access anywhere.
// The probes are those of rows_grow_lanes_kernel bit for bit (tests/test_gpu_lanes_odd.py).
#pragma once
#include "epgx_grow_lanes_kernels.hip.h"

namespace epgx {

#ifndef EPGX_LANES_ODD_CELLS
#define EPGX_LANES_ODD_CELLS lanes_odd_cells(LANES_CAP)   // the instantiation that holds every list lanes_plan accepts
#endif
constexpr int LANES_ODD_CELLS = EPGX_LANES_ODD_CELLS;   // (a smaller value refuses the launches it cannot hold: listings, A/B builds)

__device__ __forceinline__ void lanes_odd_probe(const double pr, const double pi, d2 *sig_base, const int64_t signal_ld, const int slot,
                                                const int nvalid, const uint32_t voff) {
    u32x4 bits;
    bits.x = (uint32_t)__double2loint(pr); bits.y = (uint32_t)__double2hiint(pr);
    bits.z = (uint32_t)__double2loint(pi); bits.w = (uint32_t)__double2hiint(pi);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(sig_base + (int64_t)slot * signal_ld, 0, 16 * nvalid, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(bits, rs, voff, 0, 0);
}

// rem0: the shifts of the list up to its last probe (even).  C: the cells a lane holds; windows beyond them are clamped
template <int NSP, int C>
__global__ void __launch_bounds__(64, 2) rows_grow_lanes_kernel_odd(const int64_t nvox, const Rec *__restrict__ recs_, const double *__restrict__ coef_,
                                                                   d2 *__restrict__ signal, const int64_t signal_ld, const RunTail a, const int rem0) {
    const int lane = threadIdx.x & 63;
    const const_rec_t recs = (const_rec_t)(uintptr_t)recs_;
    const __amdgpu_buffer_rsrc_t pool = __builtin_amdgcn_make_buffer_rsrc((void *)coef_, 0, 0x7fffffff, 0x00020000);
    const int n_rec = a.n_rec;
    for (uint32_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x) {
        const int64_t v0 = (int64_t)b * 64;
        if (v0 >= nvox) break;
        uint32_t p0, p1, p2, p3;
        rows_indices<NSP>(a, nvox, v0, lane, p0, p1, p2, p3);   // (tail lanes shadow the last voxel, never store)
        const int nvalid = (int)(nvox - v0 < 64 ? nvox - v0 : 64);
        const uint32_t voff = 16u * (uint32_t)lane;
        d2 *sig_base = signal + v0;
        LaneOdd<C> s;
#pragma unroll
        for (int m = 0; m < C; ++m) s.Pr[m] = s.Pi[m] = s.Qr[m] = s.Qi[m] = s.Zr[m] = s.Zi[m] = 0.0;
        double z0r = 1.0, z0i = 0.0;   // Z of order 0: the head records' alone
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
            const int tk = lanes_tk(f, head);
            if (top == 0 && !(f & (F_S0 | F_S))) {   // a head record: order 0, the cell of the train kernel
                LaneLine k;
                lanes_line<NSP>(r, pool, p0, p1, p2, p3, tk, k);
                int slot = r.slot;
                for (int e = 0; e < rep; ++e, ++slot) {
                    if (rem >= 0) {
                        LaneDeck<1> h;
                        h.Ar[0] = s.Pr[0]; h.Ai[0] = s.Pi[0]; h.Br[0] = s.Qr[0]; h.Bi[0] = s.Qi[0]; h.Zr[0] = z0r; h.Zi[0] = z0i;
                        double pend[4] = {0.0, 0.0, 0.0, 0.0};
                        lanes_cell_body<1, 0, 0, 0>(h, nullptr, 1, tk, (f & F_T0) != 0, lanes_ek(f), k, pend);
                        s.Pr[0] = h.Ar[0]; s.Pi[0] = h.Ai[0]; s.Qr[0] = h.Br[0]; s.Qi[0] = h.Bi[0]; z0r = h.Zr[0]; z0i = h.Zi[0];
                    }
                    if (f & F_ADC) lanes_odd_probe(s.Pr[0], s.Pi[0], sig_base, signal_ld, slot, nvalid, voff);
                }
                continue;
            }
            if (!lanes_odd_echo(f, head)) continue;   // (not an `odd` list: skipped, see the header)
            LaneLine k;
            lanes_line<NSP>(r, pool, p0, p1, p2, p3, 2, k);
            int slot = r.slot;
            for (int e = 0; e < rep; ++e, ++slot) {
                // the cells work between the record's two shifts: top + 1 orders are populated there, rem - 1 shifts are left
                lanes_odd_record<C>(s, top + 1 < rem - 1 ? top + 1 : rem - 1, k);
                top += 2;
                rem -= 2;
                if (f & F_ADC) lanes_odd_probe(s.Pr[0], s.Pi[0], sig_base, signal_ld, slot, nvalid, voff);
            }
        }
    }
}

}  // namespace epgx

// epgx_launch_grow.h -- launchers of the growing long-state-matrix kernels (epgx_cgrow.hip); included by epgx_api.hip and the
// units that define them only, so that work on these kernels does not rebuild every translation unit.  Not part of the public ABI.
#pragma once
#include <cstdio>
#include <vector>

#include "epgx_lanes_bodies.h"
#include "epgx_launch.h"
#include "epgx_planner.h"

// The growing launch at K = 64 (FAM_ROWS_GROW) has two variants: the rows layout (rows_grow_kernel, epgx_grow.hip: four voxels
// per wave) and one voxel per lane (rows_grow_lanes_kernel, epgx_grow_lanes.hip) for lists that lanes_plan accepts and launches
// big enough to fill the chip with waves of 64 voxels.  choose_kernel does not know of the second: it names the family, the
// launcher picks the variant from the list, the knob EPGX_LANES and the number of voxels.  EPGX_LANES_BODY (default 1) is the
// kernel's business alone: 0 runs every record of the variant through its generic body (epgx_lanes_bodies.h).
// The variant has two kernels (epgx_grow_lanes_kernels.hip.h): the one with the generic body as its fallback, and -- `train` -- the
// one without it, on a larger register deck, for lists in which every record behind the first shift has a specialised body
// (LanesPlan::train).  EPGX_LANES_TRAIN=0 and EPGX_LANES_BODY=0 both keep a launch on the first.
// A train that repeats S(+1) . X . S(+1) from an unshifted state (LanesPlan::odd) has a third: rows_grow_lanes_kernel_odd
// (epgx_grow_lanes_odd.hip) computes the orders whose parity reaches an echo and nothing else, half the cells, all in registers.
// lanes_odd_selected (EPGX_LANES_ODD) routes to it, with a trace line of its own.
hipError_t epgx_launch_rows_grow_lanes_nsp0(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L, int body, bool train);
hipError_t epgx_launch_rows_grow_lanes_nsp1(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L, int body, bool train);
hipError_t epgx_launch_rows_grow_lanes_nsp2(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L, int body, bool train);
hipError_t epgx_launch_rows_grow_lanes_nsp4(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L, int body, bool train);
hipError_t epgx_launch_rows_grow_lanes_odd_nsp0(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L);
hipError_t epgx_launch_rows_grow_lanes_odd_nsp1(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L);
hipError_t epgx_launch_rows_grow_lanes_odd_nsp2(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L);
hipError_t epgx_launch_rows_grow_lanes_odd_nsp4(hipStream_t stream, const epgx::RunArgs &a, int rem0, int L);
int epgx_lanes_odd_cells();   // the compact capacity of rows_grow_lanes_kernel_odd: cells of a lane, 12 VGPRs each
int epgx_lanes_deck(bool train);   // orders of a lane that live in VGPRs (EPGX_LANES_DECK / EPGX_LANES_TRAIN_DECK); the rest, up to L, in LDS
inline size_t epgx_lanes_lds_bytes(int L, int deck) { return L > deck ? (size_t)48 * 64 * (size_t)(L - deck) : 0; }
// `grow`: the host copy of the list `a.recs` holds; n1, n2, cap: the ranges of the rows variant
inline hipError_t epgx_launch_rows_grow(hipStream_t stream, const epgx::RunArgs &a, int n_spaces, const std::vector<epgx::Rec> &grow, int n1, int n2,
                                        const int cap[3], const epgx::Knobs &kn) {
    const epgx::LanesPlan lp = epgx::lanes_plan(grow, a.in != nullptr, a.out != nullptr, kn);
    const bool lanes = epgx::lanes_selected(lp, a.nvox, kn);
    const bool train = epgx::lanes_train_selected(lp, kn);
    const bool odd = epgx::lanes_odd_selected(lp, a.nvox, kn);
    if (odd) {
        if (epgx::tracing())
            fprintf(stderr, "[epgx] run: variant lanes-odd (one voxel per lane, odd orders only): L = %d, kernel rows_grow_lanes_kernel_odd (%d cells of 2 orders), state in %d VGPRs, 0 bytes of LDS per wave, %d shifts before the last probe\n",
                    lp.L, epgx_lanes_odd_cells(), 12 * epgx_lanes_odd_cells(), lp.rem0);
        switch (n_spaces) {
        case 0: return epgx_launch_rows_grow_lanes_odd_nsp0(stream, a, lp.rem0, lp.L);
        case 1: return epgx_launch_rows_grow_lanes_odd_nsp1(stream, a, lp.rem0, lp.L);
        case 2: return epgx_launch_rows_grow_lanes_odd_nsp2(stream, a, lp.rem0, lp.L);
        default: return epgx_launch_rows_grow_lanes_odd_nsp4(stream, a, lp.rem0, lp.L);
        }
    }
    if (epgx::tracing()) {
        if (lanes)
            fprintf(stderr, "[epgx] run: variant lanes (one voxel per lane): L = %d, kernel %s (deck %d), %zu bytes of LDS per wave, %d shifts before the last probe, body %s\n",
                    lp.L, train ? "train" : "any list", epgx_lanes_deck(train), epgx_lanes_lds_bytes(lp.L, epgx_lanes_deck(train)), lp.rem0,
                    epgx::lanes_body_names(grow, kn.lanes_body != 0).c_str());
        else
            fprintf(stderr, "[epgx] run: variant rows (four voxels per wave): %s\n",
                    lp.eligible ? "fewer voxels than the one-voxel-per-lane variant is taken for" : lp.why);
    }
    if (lanes) {
        switch (n_spaces) {
        case 0: return epgx_launch_rows_grow_lanes_nsp0(stream, a, lp.rem0, lp.L, kn.lanes_body, train);
        case 1: return epgx_launch_rows_grow_lanes_nsp1(stream, a, lp.rem0, lp.L, kn.lanes_body, train);
        case 2: return epgx_launch_rows_grow_lanes_nsp2(stream, a, lp.rem0, lp.L, kn.lanes_body, train);
        default: return epgx_launch_rows_grow_lanes_nsp4(stream, a, lp.rem0, lp.L, kn.lanes_body, train);
        }
    }
    switch (n_spaces) {
    case 0: return epgx_launch_rows_grow_nsp0(stream, a, n1, n2, cap);
    case 1: return epgx_launch_rows_grow_nsp1(stream, a, n1, n2, cap);
    case 2: return epgx_launch_rows_grow_nsp2(stream, a, n1, n2, cap);
    default: return epgx_launch_rows_grow_nsp4(stream, a, n1, n2, cap);
    }
}

// K = 128 / 256 / 512 / 1024 FROM EQUILIBRIUM while the state matrix grows: the contiguous layout walked in phases of 1, 2, 4, 8, 16
// orders per lane (epgx_cgrow.hip, one translation unit per capacity): records [0, g[0]) while at most 64 orders can hold
// anything, [g[0], g[1]) at most 128, [g[1], g[2]) at most 256, [g[2], g[3]) at most 512, the rest at the capacity
#define EPGX_DECLARE_CGROW(m) hipError_t epgx_launch_run_contig_grow_m##m(hipStream_t stream, const epgx::RunArgs &a, int n_spaces, int g1, int g2, int g3, int g4);
EPGX_DECLARE_CGROW(2) EPGX_DECLARE_CGROW(4) EPGX_DECLARE_CGROW(8) EPGX_DECLARE_CGROW(16)
#undef EPGX_DECLARE_CGROW
inline hipError_t epgx_launch_run_contig_grow(hipStream_t stream, const epgx::RunArgs &a, int K, int n_spaces, const int (&g)[4]) {
    switch (K) {
    case 128: return epgx_launch_run_contig_grow_m2(stream, a, n_spaces, g[0], g[1], g[2], g[3]);
    case 256: return epgx_launch_run_contig_grow_m4(stream, a, n_spaces, g[0], g[1], g[2], g[3]);
    case 512: return epgx_launch_run_contig_grow_m8(stream, a, n_spaces, g[0], g[1], g[2], g[3]);
    default: return epgx_launch_run_contig_grow_m16(stream, a, n_spaces, g[0], g[1], g[2], g[3]);
    }
}

// K = 2048, state-resident from equilibrium, four wavefronts per voxel with 8 orders per lane each (epgx_split.hip).
//  * state_in == null: every record on the four wavefronts, from equilibrium;
//  * state_in / dens_state: the second leg -- the records [first, n_rec) from the state [nvox][3][512] that
//    run_kernel<8, .., false> left behind record first - 1 (the populated orders reach 512 at record `first`); the third
//    and fourth part of the orders join at records join2 / join3 (they reach 1024 / 1536 there); first_slot: the probe row of the
//    first ADC from `first` on
hipError_t epgx_launch_run_split2048(hipStream_t stream, const epgx::RunArgs &a, int n_spaces, const epgx::d2 *state_in, const double *dens_state,
                                     int first, int join2, int join3, int first_slot);

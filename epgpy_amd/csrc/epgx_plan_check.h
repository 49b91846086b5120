// epgx_plan_check.h -- plan analysis: everything epgx_plan_create decides on host data alone.
//
//   analyse_plan  checks every field of an epgx_plan_desc / epgx_plan_ext, derives the grid geometry, scans the coefficient
//                 pool for the zero patterns that select the short fma chains, collects the rounding residues to clear
//                 (snaps), carries patterns through the fuse recipes and lays out the tables of logarithmic partials.
//
// No HIP here: the result is a value, and epgx_api.hip turns it into a plan on the device (upload, snap_kernel, the table
// generators).  This unit compiles with a plain host compiler (tests/host/plan_check.cpp).
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "epgx_planner.h"

namespace epgx {

// what a plan derives from grid_shape / space_strides (and, for exchange, from its EPGX_OP_X operators)
struct PlanGeometry {
    int32_t ndim = 0;
    int64_t shape[EPGX_MAX_DIMS] = {};                     // 1 beyond ndim
    int64_t strides[EPGX_MAX_SPACES][EPGX_MAX_DIMS] = {};
    int64_t space_extent[EPGX_MAX_SPACES] = {};            // largest table index each space can produce
    int64_t nvox_total = 0;
    uint32_t dense_spaces = 0;  // bit s: space s has the grid's own C-order strides
    int64_t x_span = 0;         // EPGX_OP_X in the plan: voxels per block of whole compartment groups (N * ib), else 0
    int32_t x_ncomp = 0;        // ... and its N
    int64_t entries(int space) const { return (space < 0 ? 0 : space_extent[space]) + 1; }   // table entries (-1: one for all voxels)
    int64_t stride(int space, int dim) const { return space < 0 ? 0 : strides[space][dim]; }
    // a table over `space` has one entry for all coordinates of axis `dim`, and the axis has more than one
    bool fixed_along(int space, int dim) const { return shape[dim] > 1 && stride(space, dim) == 0; }
    // shape[] and the strides of `space` as the table generators take them
    void fill(int64_t *shape_out, int64_t *str_out, int space) const {
        for (int dd = 0; dd < ndim; ++dd) {
            shape_out[dd] = shape[dd];
            str_out[dd] = stride(space, dd);
        }
    }
};

// exchange with derivative states: dxrun_kernel<N, K / 64, V> holds the state and V derivative states of the N compartments of
// a group in registers -- N (K / 64) (1 + V) <= 8 state matrices of 64 orders, N = 2 .. 4.  There is no split path for
// derivatives, so what does not fit is refused (plan analysis at K = 64, epgx_run at the capacity it is asked for)
inline bool xrun_deriv_fits(int ncomp, int K, int n_vars) {
    return ncomp >= 2 && ncomp <= 4 && n_vars >= 1 && K >= 64 && K % 64 == 0 && ncomp * (K / 64) * (1 + n_vars) <= 8;
}

// rounding residues to clear in the device copy of a table (snap_kernel): bit c of mask = column c of every entry
struct Snap { int64_t off, entries; int nc; uint32_t mask; };
// one table of logarithmic partials to generate (logtab_kernel): PlanHost::logtabs[j] is written from log_jobs[j]
struct LogJob { int64_t e_off, de_off, entries; };

struct PlanAnalysis {
    PlanHost host;
    PlanGeometry geo;
    std::vector<Snap> snaps;       // in the launch order of snap_kernel
    std::vector<LogJob> log_jobs;
};

// EPGX_OK, or the code of the first failing check with the message left for epgx_last_error() (fail)
int analyse_plan(const epgx_plan_desc *d, const epgx_plan_ext *ext, const Knobs &kn, PlanAnalysis *out);

// EPGX_TRACE: "[epgx] plan_create <what> +<ms since the object was made>" on stderr
struct Lap {
    const bool on = tracing();
    const std::chrono::steady_clock::time_point tic = std::chrono::steady_clock::now();
    void operator()(const char *what) const {
        if (on)
            fprintf(stderr, "[epgx] plan_create %-12s +%.3f ms\n", what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tic).count());
    }
};

}  // namespace epgx

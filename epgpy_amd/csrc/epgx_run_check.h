// epgx_run_check.h -- run analysis: everything epgx_run, epgx_kernel_for and the tiled entry points decide before they need
// the device or the record lists.
//
//   analyse_run    is this request legal, and which route does it take: nothing to do, the records of the range (build_range /
//                  choose_kernel then name the kernel), or -- for a range that holds EPGX_OP_X -- xrun_kernel, dxrun_kernel or
//                  the split path, with the kernel's template arguments and its name;
//   signal_room    the one "an ADC needs room in the signal buffer" check, in the wording of each route;
//   analyse_tiled  the checks of epgx_run_tiled(_deriv) and epgx_tiled(_deriv)_info and the tile shape M, H;
//   slab_voxels    the 8 GiB rule of the two-leg launch at 2048 orders and of the tiled runs.
//
// No HIP here, and handles appear as facts: epgx_api.hip compares the pointers (NULL, another context), fills a RunRequest and
// launches what a RunDecision names.  No allocation either -- epgx_run is called once per timestep in stream mode.  This unit
// compiles with a plain host compiler (tests/host/run_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

#include "epgx_plan_check.h"

namespace epgx {

inline bool supported_K(int K) { return K == 64 || K == 128 || K == 256 || K == 512 || K == 1024; }

struct StateFacts {
    bool present = false;
    int32_t K = 0;
    int64_t nvox = 0;
    bool foreign = false;   // belongs to another context than the call's
};

struct RunRequest {
    int32_t op_begin = 0, op_end = 0;
    int64_t vox0 = 0, nvox = 0;
    int32_t K = 0;          // the K asked for (`in` / `out` override it)
    StateFacts in, out;
    bool has_signal = false;
    int64_t signal_ld = 0, signal_col0 = 0;
    bool naming = false;    // epgx_kernel_for: the decision only -- no signal buffer is looked at
};

enum RunRoute {
    ROUTE_NONE,      // no voxels or no operators
    ROUTE_RECORDS,   // packed records on the kernel choose_kernel names
    ROUTE_XRUN,      // xrun_kernel<NC, M, HAS_IN>: compartment groups in registers
    ROUTE_DXRUN,     // dxrun_kernel<NC, M, V>: ... with derivative states
    ROUTE_XSPLIT     // the records between two EPGX_OP_X on the per-timestep kernels, exchange_kernel in between
};
struct RunDecision {
    int K = 0;               // the effective capacity
    bool packed16 = false;   // K = 16 / 32
    bool wide = false;       // K = 2048, state-resident from equilibrium
    RunRoute route = ROUTE_NONE;
    int NC = 0, M = 0, V = 0;   // the exchange routes: compartments, K / 64, derivative states
    bool has_adc = false;       // ... and whether the scan of the range met an ADC
    char name[128] = "";        // "none", the exchange routes' kernel; empty for ROUTE_RECORDS (Choice::name has it)
};

// EPGX_OK, or the code of the first failing check with the message left for epgx_last_error() (fail)
int analyse_run(const PlanHost &ph, const PlanGeometry &geo, const RunRequest &rq, const Knobs &kn, RunDecision *out);

// a range with an ADC needs `nvox` columns from signal_col0 on.  `exchange`: the one message of the exchange routes (analyse_run
// calls it), else the two of the records route (epgx_api.hip calls it once RangeLists::has_adc is known).  EPGX_OK when naming.
int signal_room(const RunRequest &rq, bool exchange);

// ------------------------------------------------------------------------------ tiled runs
constexpr int TILED_DERIV_V = 2;   // derivative states one launch of tiled_deriv_kernel<8, 32, NSP, V> carries (_lib.py TILED_DERIV_V)

struct TiledRequest {   // what epgx_run_tiled(_deriv) adds to (plan, Kbuf)
    int64_t vox0 = 0, nvox = 0, slab_voxels = 0;
    StateFacts in;
};
struct TiledShape {
    int M = 8, H = 32;   // orders per lane and halo of the tile kernel
    int top0 = 0;        // highest order that holds anything at the start
};
// `rq` given: a run (top0 follows from `in`); NULL: an info call, with `top0` checked against Kbuf.  `tiled_m`: EPGX_TILED_M
// (16: 16 orders per lane, halo 64 -- measurements; the derivative kernel exists at 8 orders per lane only).
int analyse_tiled(const char *who, bool deriv, const PlanHost &ph, const PlanGeometry &geo, int32_t Kbuf, int tiled_m, const TiledRequest *rq,
                  int32_t top0, TiledShape *out);

// voxels per slab of a launch that needs `per_voxel_bytes` of scratch per voxel: a multiple of four, at most 8 GiB of scratch and at
// least four voxels; `knob` = EPGX_SLAB_VOXELS (rounded up to four), `requested` = the slab_voxels argument of the tiled entry
// points (taken as it is); 0: no limit from that side
inline int64_t slab_voxels(int64_t nvox, int64_t per_voxel_bytes, int knob, int64_t requested) {
    int64_t slab = std::min<int64_t>((nvox + 3) & ~(int64_t)3, std::max<int64_t>(4, (((int64_t)8 << 30) / per_voxel_bytes) & ~(int64_t)3));
    if (knob > 0) slab = std::min<int64_t>(slab, (knob + 3) & ~3);
    if (requested > 0) slab = std::min<int64_t>(slab, requested);
    return slab;
}

}  // namespace epgx

// epgx_planner.h -- launch planning: everything that decides what a launch does, on host data alone.
//
//   build_range    packs operators [begin, end) of a plan into fused records for capacity K and derives the folded lists
//                  (runs, growing phases, derivative runs) the kernels walk;
//   choose_kernel  THE place where a launch gets its kernel;
//   tiled_schedule cuts a whole plan into the blocks and shift steps of epgx_run_tiled.
//
// No HIP here: nothing allocates, uploads or launches.  epgx_api.hip owns the device side (it uploads a RangeLists and caches
// it, and launches what a Choice names); this unit compiles with a plain host compiler (tests/host/planner_check.cpp).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/epgx.h"
#include "epgx_error.h"
#include "epgx_records.h"

namespace epgx {

// Measurement knobs of the selection: every one defaults to the kernel the library would take anyway; tools/ab_kernels.sh flips
// them for A/B runs.  epgx_api.hip reads them from the environment ONCE per process (knobs()) and hands them in.
struct Knobs {
    bool rows, rows_deriv, rows_deriv2, drun, runs, grow, contig, split, prefetch;
    int grow_min;
    bool fold;
    double grow_share;
    bool lead_forward;
    int slab_voxels; // EPGX_SLAB_VOXELS (tests): voxels per slab of the two-leg launch at 2048 orders (0: as many as 8 GiB of scratch hold)
    bool split_grow; // EPGX_SPLIT_GROW (default 1): K = 2048 in two legs where it pays (one wavefront per voxel up to 512 populated orders)
    bool xrun;      // EPGX_XRUN (default 1): ranges with exchange (EPGX_OP_X) on xrun_kernel where it covers them; 0: always the split path
    bool reach;     // EPGX_REACH (default 1): a range of rows_grow_kernel runs at the orders that can still reach a probe (grow_reach); 0: at 16 / 32 / 64
    int cgrow;      // EPGX_CGROW: 0 off, 1 (default): growing launches at K = 256 .. 1024, at K = 128 when 60 % of the records run below 64 orders; 2: at K = 128 whenever the other capacities would
    int lanes;      // EPGX_LANES: the one-voxel-per-lane variant of a FAM_ROWS_GROW launch (lanes_plan) -- 0 never, 1 from LANES_MIN_VOXELS voxels on, 2 whenever the list is eligible (tests)
    int lanes_body = 1;   // EPGX_LANES_BODY: the record bodies of that variant -- 1 (default) specialised and blocked where one exists, 0 the generic per-cell body everywhere.  The kernel's alone: no part of lanes_plan / lanes_selected
    int lanes_train = 1;  // EPGX_LANES_TRAIN: 1 (default) a train (LanesPlan::train) runs the kernel without a generic body on its larger deck, 0 every list runs the kernel with it.  lanes_plan reports `train` whatever this says; lanes_train_selected is the choice
    int lanes_odd = 1;    // EPGX_LANES_ODD: the kernel of that variant that computes only the orders whose parity reaches an echo (LanesPlan::odd, rows_grow_lanes_kernel_odd) -- 0 never, 1 (default) for launches of LANES_MIN_VOXELS voxels and more, 2 whenever the list allows it (tests).  Only ever for a launch that lanes_selected already gives to the one-voxel-per-lane variant (EPGX_LANES) and lanes_train_selected to its train kernel: the knob never takes a launch from the rows variant.  lanes_plan reports `odd` whatever this says; lanes_odd_selected is the choice
};
// EPGX_TRACE is read per call (tests switch it on and off)
inline bool tracing() { return getenv("EPGX_TRACE") != nullptr; }

// derivative plans: logarithmic partials (wT, wL per entry, logtab_kernel) of the real relaxation tables that carry a real
// partial over the same index space -- what drun_kernel's folded records read.  Behind the pool's padding.
struct LogTab {
    int64_t off = -1;     // doubles from the pool's base
    int space = -1;
    uint32_t any = 0;     // 1: some wT != 0, 2: some wL != 0
};

// the host-only part of a plan: what planning reads (epgx_plan holds one)
struct PlanHost {
    std::vector<epgx_op> ops;  // host copy of the primitive stream (validation, packing)
    std::vector<uint8_t> zero_pattern;  // per op: 1 / 3 = T table with the TX / TY pattern (plan_create), 2 = E table with Im e0 == 0
    std::vector<std::vector<int32_t>> gather_tables;  // per op: host copy of an EPGX_OP_GS table (validation)
    std::vector<epgx_dop> dops;  // first-order partials per op (n_vars > 0)
    std::vector<uint16_t> dpattern; // per op: bits 2v, 2v + 1 = zero pattern of variable v's partial table (1: phi = 0 / real E, 2: real matrix);
                                    // bit 8 + v: the partial is a generated one (14 per entry: with the partial of the constant term)
    int32_t n_vars = 0;
    bool second = false;      // EPGX_DERIV_SECOND: a one-pair second-order pass (n_vars 3: S_a, S_b, H_ab; 2: S_a, H_aa); epgx_dop::reserved
                              // then carries the operator's EPGX_HESS_CROSS_* bits (-> DRec.pad0)
    int32_t n_spaces = 0;
    int64_t n_pool = 0;       // doubles in the device pool: n_coef + the device-generated part; behind it 32 doubles of
                              // padding that start with the identity relaxation {1, 0, 1, 0} (folded records)
    int64_t n_log = 0;        // doubles of log tables behind n_pool + 32
    bool fold = true;         // fold precession-free relaxations into neighbouring rotations at run time (pack_records)
    std::vector<LogTab> logtabs;
    std::vector<int32_t> log_of;   // [op * EPGX_MAX_VARS + v] -> index into logtabs, or -1
    // EPGX_OP_T0 operators whose table the host had fused (E_a . T . E_b, epgx_fuse) and whose partial w.r.t. variable v comes
    // from the relaxations alone (epgx_fuse_partial chain without a rotation partial): the log tables of E_a and E_b
    // ([(op * EPGX_MAX_VARS + v) * 2 + {0: a, 1: b}], -1: that side has no partial), or empty.  t0_logd[op * MAX_VARS + v]
    // says whether the variable can take the logarithmic route at all.
    std::vector<int32_t> t0_log;
    std::vector<uint8_t> t0_logd;
};

// one operator range [begin, end) packed into fused records for capacity K: the lists as the kernels walk them (without the
// padding records the upload appends) and what the launch needs to know about them
struct RangeLists {
    int begin = 0, end = 0, K = 0;
    std::vector<Rec> recs;
    std::vector<DRec> drecs;  // derivative plans only
    int n_rec = 0;
    std::vector<Rec> runs;    // the same records with runs of identical ones folded (rows_kernel<.., RUNS>), or empty
    int n_runs = 0;
    std::vector<Rec> grow;    // K = 64: the run-folded records cut where the populated orders outgrow 16 and 32 (rows_grow_kernel), or empty
    int n_grow = 0, grow1 = 0, grow2 = 0;   // records [0, grow1) run at 16 orders per voxel, [grow1, grow2) at 32, the rest at 64 ...
    int grow_cap[3] = {16, 32, 64};         // ... or at fewer, where fewer can still reach a probe (grow_reach)
    std::vector<Rec> druns;   // derivative plans, K = 64: the records with a header in front of every run of same-shape
    std::vector<DRec> ddruns; // fused-echo records (drun_kernel), and their DRecs (a header's is all zero); or empty
    std::vector<DRecB> bdruns; // ... and, when the runs are of records folded at run time (DRUN_FOLD), E_b's logarithmic partials
    int n_druns = 0;
    int drun_code = 0;        // the run shape the headers of druns announce (drun_kernel is instantiated per shape)
    // K = 128 .. 1024 from equilibrium (run_contig_grow_kernel): records [0, cgrow[0]) run while at most 64 orders can hold anything,
    // [cgrow[0], cgrow[1]) at most 128, [cgrow[1], cgrow[2]) at most 256, [cgrow[2], cgrow[3]) at most 512; cgrow_share = the share
    // of the records below the capacity
    int cgrow[6] = {0, 0, 0, 0, 0, 0};   // (cgrow[3]: K = 2048, where the second leg starts; cgrow[4], cgrow[5]: at most 1024, 1536 -- where parts 2 and 3 of run_split_kernel join)
    double cgrow_share = 0.0;
    int cgrow_adc3 = 0;       // probe records in front of record cgrow[3] (K = 2048: the first row the second leg writes)
    int dgrow1 = 0, dgrow2 = 0;   // fused echoes from equilibrium: entries [0, dgrow1) of druns run with one order per lane, [dgrow1, dgrow2) with two
    int drun_inside = 0, drun_headers = 0, drun_ident = 0;   // records inside runs, runs, runs that repeat one record (EPGX_TRACE)
    bool use_lds = false, has_adc = false, has_pd = false;
    bool has_gs = false;     // some record is a gather shift (three staged arrays per wavefront instead of two)
    bool big_shift = false;  // some record shifts by |n| >= 2 (use_lds is also set by gather shifts)
    bool seq_slots = false;  // the ADC slots of the range are first_slot, first_slot + 1, ...
    int first_slot = 0;
    int pf_count = 0;        // 1 + index of the last record that refers to a per-voxel table for the first time
};

// which table of logarithmic partials (PlanHost::logtabs) the relaxation stage of a record has for every variable
struct ELog {
    int32_t tab[EPGX_MAX_VARS];   // -1: the stage has no partial w.r.t. this variable
    bool blocked;                 // some partial of the stage has no log table: the record cannot fold
    int32_t t_op;                 // primitive index of the record's rotation stage, or -1
};

void pack_records(const PlanHost &ph, int begin, int end, int K, const Knobs &kn, std::vector<Rec> &out, std::vector<DRec> &dout,
                  bool &use_lds, bool &has_adc, std::vector<ELog> &elog);
void grow_split(const std::vector<Rec> &runs, std::vector<Rec> &out, int &n1, int &n2, double work[3]);
void grow_reach(const std::vector<Rec> &list, int n1, int n2, int cap[3]);

// The one-voxel-per-lane variant of a FAM_ROWS_GROW launch (rows_grow_lanes_kernel, epgx_grow_lanes_kernels.hip.h): whether the
// cut list `grow` can run there, and what the launch needs.  A pure function of the list and the knob.
//   eligible  the launch starts from equilibrium and writes no state; every record is made of rotation / relaxation / S(+1)
//             leading or trailing / F0 probe stages (members of pair and folded runs included); no truncation, no S(-1) or
//             shift by |n| >= 2, no gather shift, no diffusion, no spoiler (folded ones included), no reset, no density stage,
//             no general matrix, no Z0 probe; the list has a probe; L <= LANES_MAX_ORDERS
//   L         the largest number of live orders between two shifts: 1 + min(top, rem), top = the shifts so far (grow_split's
//             highest populated order), rem = the shifts left up to the last probe -- grow_reach's rule shift by shift
//             instead of record by record, without the rounding to 16 / 32 / 64.  An n-echo train (two shifts each): n + 1
//   rem0      the shifts of the whole list up to its last probe (what the kernel starts `rem` from)
//   why       "" or the first reason the list was refused for
//   train     eligible, and every record is a head record or has a specialised body (lanes_body_id, epgx_lanes_bodies.h).  A head
//             record executes before any shift has taken place (top == 0) and has no leading shift: it touches order 0 alone,
//             whatever its kinds; a trailing shift (one execution then: the second would start at top == 1) only moves where its
//             cell puts the result.  Such a list can run the instantiation of the kernel that has no generic body
//   odd       a train that repeats S(+1) . X . S(+1) from an unshifted state: `train`; every record that is not a head record has
//             a leading AND a trailing S(+1) and is the folded echo about x (lanes_odd_echo, epgx_lanes_bodies.h: checked on its own,
//             whatever bodies the table holds); no head record shifts, so the
//             first such record starts at top == 0; rem0 is even.  Between two pulses F moves by two orders, Z by none, and a
//             rotation mixes one order: the orders that are odd when a pulse acts never exchange anything with the even ones, the
//             excitation enters the odd class through the first shift and a probe (F0 behind the trailing shift, F-(1) at the pulse)
//             reads it.  Such a list can run the kernel that computes the odd class alone (epgx_grow_lanes_odd_kernels.hip.h)
constexpr int LANES_MAX_ORDERS = 24;
constexpr int64_t LANES_MIN_VOXELS = 1 << 19;   // EPGX_LANES=1: the variant from this many voxels on (the crossover)
struct LanesPlan {
    bool eligible = false;
    int L = 0, rem0 = 0;
    const char *why = "";
    bool train = false;
    bool odd = false;
};
LanesPlan lanes_plan(const std::vector<Rec> &grow, bool has_in, bool has_out, const Knobs &kn);
// the launcher's choice: the knob, the list and the size of the launch
inline bool lanes_selected(const LanesPlan &lp, int64_t nvox, const Knobs &kn) {
    return lp.eligible && (kn.lanes >= 2 || (kn.lanes == 1 && nvox >= LANES_MIN_VOXELS));
}

// which kernel of the variant: the one without a generic body for a train, unless a knob asks for the other (EPGX_LANES_BODY=0
// means the generic body for every record, and only the other kernel has it)
inline bool lanes_train_selected(const LanesPlan &lp, const Knobs &kn) { return lp.eligible && lp.train && kn.lanes_train != 0 && kn.lanes_body != 0; }

// which train runs the odd-class kernel.  1 gates on the size by itself: forced-lanes runs on small grids (EPGX_LANES=2) stay
// on the train kernel unless EPGX_LANES_ODD=2 asks
inline bool lanes_odd_selected(const LanesPlan &lp, int64_t nvox, const Knobs &kn) {
    return lanes_selected(lp, nvox, kn) && lanes_train_selected(lp, kn) && lp.odd &&
           (kn.lanes_odd >= 2 || (kn.lanes_odd == 1 && nvox >= LANES_MIN_VOXELS));
}

// pack_records, then in this order: run folding, the phases of rows_grow_kernel, the phases of run_contig_grow_kernel, the runs of
// derivative plans
RangeLists build_range(const PlanHost &ph, int begin, int end, int K, const Knobs &kn);

// ------------------------------------------------------------------------------ tiled runs: state matrices of any length
// (epgx_tiled.hip).  The plan's records are packed as for any capacity, with every truncation explicit (no capacity drops
// orders here), then
//   * a shift by 2 .. H orders becomes |n| records of S(+-1) (the same moves, the truncation and the probe on the last);
//   * a shift by more than H becomes a step of its own (tiled_shift_kernel): the stages in front of it stay a record, the
//     probe behind it becomes one;
// and the list is cut into blocks whose shifts add up to at most H.  A derivative plan (n_vars > 0) carries a DRec per record,
// parallel to `recs` (epgx_run_tiled_deriv): the stages keep theirs, the unit shifts and probes made here have no partials.  `top` = the highest order that can hold anything, as in
// build_range plus truncations and resets; a launch covers the tiles up to the top after its block, and at least the tiles the
// launch before the previous one wrote into the same buffer (so no tile of the output buffer keeps a stale value).
struct TiledStep {
    int rec0 = 0, rec1 = 0;    // block: records [rec0, rec1); a shift step has none
    int shift = 0;             // shift step: n, |n| > H
    int kmax = INT32_MAX;      // shift step: truncation above kmax
    int tiles = 0;             // tiles the launch covers
    int top = 0;               // highest order that can hold anything after the step
};
struct TiledSchedule {
    std::vector<Rec> recs;
    std::vector<DRec> drecs;   // derivative plans: parallel to recs (present = 0 where a record has no partials); else empty
    std::vector<TiledStep> steps;
    int peak = 0, n_shift = 0;
    int64_t tile_launches = 0;
    bool has_adc = false;
};
Rec with_leaf(Rec r);
int tiled_schedule(const PlanHost &ph, int Kbuf, int top0, int M, int H, const Knobs &kn, TiledSchedule &ts);

// ------------------------------------------------------------------------------ kernel selection
enum Family {
    FAM_RUN,           // run_kernel<M, NSP, HAS_IN>: one wavefront per voxel, K / 64 orders per lane (any operator; state in / out)
    FAM_RUN_CONTIG,    // run_contig_kernel: K = 128 .. 1024 without a state output, K / 64 consecutive orders per lane
    FAM_RUN_CONTIG_GROW, // run_contig_grow_kernel<M, NSP>: the same from equilibrium in phases of 1, 2, 4 .. orders per lane while the state matrix grows
    FAM_RUN_SPLIT,     // run_split_kernel<4, ..>: K = 2048 from equilibrium, four wavefronts per voxel (behind a run_kernel<8, ..> leg where that pays)
    FAM_ROWS,          // rows_kernel<NSP, R, RUNS>: four voxels per wavefront, R = K / 16 orders per lane, state-resident
    FAM_ROWS_GROW,     // rows_grow_kernel<NSP>: the same walked in phases of R = 1, 2, 4 while the state matrix grows (K = 64)
    FAM_DERIV,         // deriv_kernel<M, NSP, V>: one wavefront per voxel, 1 + V states
    FAM_PACKED_DERIV,  // packed_deriv_kernel<NSP, V, KP>: 16 / 32 orders, four / two voxels per wavefront, 1 + V states
    FAM_ROWS_DERIV,    // rows_deriv_kernel<NSP, 4, V>: the rows layout with one or two derivative states
    FAM_DRUN,          // drun_kernel<NSP, V, SHAPE, V0>: rotating order slots, runs of fused / folded records, 1 + V states
    FAM_PACKED_DFOLD,  // packed_dfold_kernel: 16 / 32 orders, repetitions folded at run time, 1 + V states
    FAM_HESS           // hess_kernel<M, NSP, DIAG>: one-pair second-order pass, one wavefront per voxel, S, S_a, (S_b,) H
};
struct Choice {
    Family family = FAM_RUN;
    bool runs = false;      // rows kernels: the run-length folded record list
    bool split_grow = false; // K = 2048: two legs -- run_kernel<8, ..> up to 512 populated orders, then run_split_kernel from its state
    bool split3 = false;    // drun_kernel: three derivative states of folded runs in two launches (V0 = 2, then V = 2)
    // what the decision derived on its way and the launch needs again
    bool packed16 = false;  // K = 16 / 32
    bool wide = false;      // K = 2048, state-resident
    bool has_nd = false;    // the range holds diffusion or gather shifts
    bool contig = false;    // deriv_kernel at K >= 128: K / 64 consecutive orders per lane
    int lds_mode = 0;       // 0, or the arrays of K complex a wavefront stages in LDS (RunTail::use_lds): 2 or 3
    char name[128] = "";
    const char *why = "";
};

// THE place where a launch gets its kernel: operators [op_begin, op_end) of a plan at capacity K, with / without a state input
// and output.  Everything the decision depends on is an argument or a field of the plan / its lists -- no state of the
// context, no launch size -- so epgx_kernel_for can answer without launching (tests pin the kernel of every BASELINE config).
// Returns EPGX_OK or an error code with the message left for epgx_last_error() (fail).
int choose_kernel(const PlanHost &ph, const RangeLists &lists, int op_begin, int op_end, int K, bool has_in, bool has_out, const Knobs &kn,
                  Choice *c);

}  // namespace epgx

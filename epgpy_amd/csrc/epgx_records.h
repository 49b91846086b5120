// epgx_records.h -- what the host's launch planning (epgx_planner.cpp) and the kernels have to agree on: the fused record, its
// flags and leaf numbers, the derivative records and the shape codes of their runs.  Plain C++17, no HIP header: the planner
// compiles with a host compiler alone.  The kernel headers (epgx_kernels.hip.h, epgx_deriv_kernels.hip.h) include this file.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace epgx {

// ---------------------------------------------------------------- fused record (32 bytes)
enum : uint32_t {
    F_T = 1u << 0,       // symmetric 3x3 with real m00 (8 coefficients)
    F_MAT = 1u << 1,     // general symmetric 3x3 (9 coefficients, padded to 10)
    F_E = 1u << 2,       // diagonal (4 coefficients)
    F_S = 1u << 3,       // shift by `shift`
    F_TRUNC = 1u << 4,   // zero orders above `kmax` after the shift
    F_ADC = 1u << 5,     // record F0 ...
    F_ADC_Z = 1u << 6,   // ... or Z0
    F_SPOIL = 1u << 7,
    F_RESET = 1u << 8,
    F_PD = 1u << 9,      // density <- coefficient (uses the E slot's table reference)
    F_PD_RESET = 1u << 10,
    F_FOLD_SPOIL = 1u << 11,  // with F_FOLD: a spoiler stood right in front of the rotation -- it is part of the fold (the F columns
                         // of E_b count as zero: T only sees Z), so a spoiled repetition runs a straight-line body
    F_TX = 1u << 12,     // with F_T: every entry has Im m01 = Re m02 = Re m20 = 0 exactly (phi = 0)
    F_ER = 1u << 13,     // with F_E: every entry has Im e0 = 0 exactly (no precession, g = 0)
    F_D = 1u << 14,      // per-order real diagonal (diffusion): table entry [3][K] doubles (F, mirrored F, Z)
    F_GS = 1u << 15,     // host-planned gather shift (n-D integer shift): int32 table [3][K]
    F_MAT0 = 1u << 16,   // with F_MAT: constant term (o0, conj o0, o2) * density on the k = 0 order
    F_T0 = 1u << 17,     // with F_T: the same constant term, stored after the 8 coefficients of T
                         // (with F_TX: Re o0 = 0 exactly as well)
    F_S0 = 1u << 18,     // shift by +1 (no truncation) BEFORE the T stage
    F_TY = 1u << 19,     // with F_T: every entry has Im m01 = Im m02 = Im m20 (= Im o0) = 0 exactly (phi = +-90: a real matrix);
                         // rows_kernel runs shorter chains, the other kernels the plain ones (same bits: the products are zero)
    F_FOLD = 1u << 20,   // with F_T | F_T0: the rotation's table holds a plain T (8 coefficients); the record's effective
                         // operator is  E_a . T . E_b  with two precession-free relaxations folded in AT RUN TIME, per voxel
                         // (fold_T below): rows scaled by E_a, columns by E_b, recoveries -> constant term.  e_off / e_ix
                         // name E_a's table (the record has no E stage of its own), the `shift` word holds the BYTE OFFSET
                         // of E_b's table (a shift stage of such a record is always +1), bits 21..23 E_b's geometry:
    F_FOLD_BSPACE = 3u << 21,   //   index space of E_b's table
    F_FOLD_BVOX = 1u << 23,     //   E_b's table has one entry per index (else one entry for all voxels)
                         // A relaxation that is missing on one side is the identity entry {1, 0, 1, 0} kept behind the pool.
    // bits 24..31: number of the straight-line leaf for this record (leaf_id), 255 = generic
};
// table geometry word (entry bytes | index space << 24) of a folded record's E_b
__host__ __device__ inline uint32_t fold_b_ix(uint32_t flags) {
    return (flags & F_FOLD_BVOX) ? (32u | (((flags & F_FOLD_BSPACE) >> 21) << 24)) : 0u;
}
constexpr int32_t GS_ZERO = -1;          // gather source: nothing (zero)
constexpr int32_t GS_CONJ = 1 << 30;     // gather source: conjugate of the partner array (A <-> B)

struct Rec {
    uint32_t flags;
    int32_t shift;
    int32_t kmax;
    int32_t slot;
    uint32_t t_off;  // byte offset of the T/MAT table in the pool
    uint32_t e_off;  // byte offset of the E (or PD) table
    uint32_t t_ix;   // bits 0..23: bytes per table entry (0 = same entry for every voxel), bits 24..25: index space
    uint32_t e_ix;
};
static_assert(sizeof(Rec) == 32, "Rec must be one s_load_dwordx8");

// ---------------------------------------------------------------- straight-line leaves (dispatch_record, epgx_kernels.hip.h)
// TK: 0 none, 1 T, 2 TX, 3 T + constant term, 4 TX + constant term;  EK: 0 none, 1 E, 2 ER
constexpr uint32_t LEAF_NONE = 255u;
constexpr uint32_t LEAF_PAIR = 254u;   // header of a run of record PAIRS (rows_kernel<.., RUNS> only: rows_pair_run)
constexpr uint32_t LEAF_SINGLE = 253u; // header of a run of folded records of one shape (rows_kernel<.., RUNS> only: rows_single_run)
__host__ __device__ constexpr uint32_t leaf_id(int TK, int EK, bool HS, bool HA, bool HS0) {
    return (uint32_t)(TK + 5 * (EK + 3 * ((HS ? 1 : 0) + 2 * ((HA ? 1 : 0) + 2 * (HS0 ? 1 : 0)))));
}
// which (TK, EK, HS, HA, HS0) combinations have a leaf
__host__ __device__ constexpr bool leaf_exists(int TK, int EK, bool HS, bool HA, bool HS0) {
    if (HS0) return TK >= 1 && EK == 0;                  // leading shift: rotation (+ constant), no E
    if (TK >= 3) return EK == 0;                         // constant term: no E
    if (TK == 0 && EK == 0) return HS || HA;             // S / ADC only
    return true;
}
// leaf of a packed record (flags without the id), or LEAF_NONE.  The host stores record_leaf<false>: a
// record that truncates after its shift is a generic record for run_kernel; rows_kernel, whose leaves
// handle the truncation, recomputes the number with WITH_TRUNC = true for the records marked LEAF_NONE.
template <bool WITH_TRUNC>
__host__ __device__ inline uint32_t record_leaf(uint32_t f, int shift) {
    const uint32_t slow = F_MAT | (WITH_TRUNC ? 0u : (uint32_t)F_TRUNC) | F_ADC_Z | F_SPOIL | F_RESET | F_PD | F_PD_RESET | F_D |
                          F_GS | F_MAT0;
    if ((f & slow) || ((f & F_S) && !(f & F_FOLD) && shift != 1)) return LEAF_NONE;   // (folded records: the shift word is E_b's table)
    const int TK = !(f & F_T) ? 0 : ((f & F_T0) ? ((f & F_TX) ? 4 : 3) : ((f & F_TX) ? 2 : 1));
    const int EK = !(f & F_E) ? 0 : ((f & F_ER) ? 2 : 1);
    const bool HS = f & F_S, HA = f & F_ADC, HS0 = f & F_S0;
    if ((f & F_T0) && !(f & F_T)) return LEAF_NONE;
    if (!leaf_exists(TK, EK, HS, HA, HS0)) return LEAF_NONE;
    return leaf_id(TK, EK, HS, HA, HS0);
}

// ---------------------------------------------------------------- derivative records (epgx_deriv_kernels.hip.h)
constexpr int MAX_VARS = 3;

struct DRec {                 // 64 bytes = two s_load_dwordx8
    uint32_t t_off[MAX_VARS]; // byte offset of d(T stage)/dv, 10 doubles per entry
    uint32_t t_ix[MAX_VARS];
    uint32_t present;         // bit v: T partial for variable v; bit 4 + v: E partial; bit 16 + v: the T partial is a REAL matrix;
                              // bit 8 + v: the T partial has the phi = 0 zero pattern (Im m00 = Im m01 =
                              // Re m02 = Re m20 = 0 for every entry); bit 12 + v: the E partial is real
    uint32_t pad0;            // second-order plans (hess_kernel): HESS_* bits, which cross terms enter the H row at the T / E stage
    uint32_t e_off[MAX_VARS]; // byte offset of d(E stage)/dv, 4 doubles per entry
    uint32_t e_ix[MAX_VARS];
    uint32_t pad1[2];
};
static_assert(sizeof(DRec) == 64, "DRec must be two s_load_dwordx8");

// DRec.pad0 of a one-pair second-order plan (EPGX_DERIV_SECOND; epgx_hess_kernels.hip.h): cross term a = (dOp/da) S_b (the doubled
// term (dOp/da) S_a of a diagonal pair), cross term b = (dOp/db) S_a.  The second-order term is `present` of the H slot.
enum : uint32_t { HESS_T_XA = 1u << 0, HESS_T_XB = 1u << 1, HESS_E_XA = 1u << 4, HESS_E_XB = 1u << 5 };

// records folded at run time in derivative plans (drun_kernel, DRUN_FOLD): E_a . T . E_b as ONE stage.  DRec then holds, per
// variable, the rotation's partial (t_off / t_ix, folded like the rotation) and E_a's table of logarithmic partials (e_off /
// e_ix: two doubles per entry, logtab_kernel); this parallel record holds E_b's.  One s_load_dwordx8.
struct DRecB {
    uint32_t off[MAX_VARS];   // byte offset of E_b's (wT, wL) table for variable v; tables that do not exist point at zeros
    uint32_t ix[MAX_VARS];
    uint32_t logs;            // bit v: E_a's wT != 0 somewhere; 4 + v: E_a's wL; 8 + v: E_b's wT; 12 + v: E_b's wL
    uint32_t pad;
};
static_assert(sizeof(DRecB) == 32, "DRecB must be one s_load_dwordx8");

// ---- runs of same-shape records in derivative plans (drun_kernel, epgx_drun_kernels.hip.h): what the host (build_range, epgx_planner.cpp) and the
// kernel have to agree on
constexpr uint32_t LEAF_DRUN = 252u;   // header of a run of same-shape records in a derivative plan (drun_kernel only)
// shape code of a run (low bits of the header's flags word)
enum : uint32_t {
    DRUN_KIND = 3u,        // bits 0..1: rotation chains -- 0 general (T), 1 phi = 0 pattern (TX), 2 real matrix (TY)
    DRUN_PK = 3u << 2,     // bits 2..3: chains of the partial accumulation -- 0 general symmetric 3x3, 1 TX pattern, 2 real
    DRUN_HS0 = 1u << 4,    // leading S(+1)
    DRUN_HS = 1u << 5,     // trailing S(+1)
    DRUN_IDENT = 1u << 6,  // every record of the run refers to the same table entries (an echo train): lines loaded once
    DRUN_FOLD = 1u << 7,   // records folded at run time: E_a . T . E_b with logarithmic relaxation partials (part of the shape code)
    DRUN_LAST = 1u << 9,   // launcher flag (not part of a header's code): the one-state kernel propagates the plan's THIRD variable
    DRUN_LOGD = 1u << 8,   // fused-echo records (table from the host's fusion) whose relaxation-only partials take the logarithmic
                           // route instead of their generated partial tables (part of the shape code)
};

// shape code of a record that can be part of a run (flags without the leaf byte), or -1.  `present`: DRec.present, n_vars: V.
// Shared by the host (build_range) and nothing else: kept next to the kernel that has to agree with it.
__host__ __device__ inline int drun_shape(uint32_t f, int shift, uint32_t present, int n_vars) {
    const uint32_t need = F_T | F_T0 | F_ADC;
    const uint32_t other = F_MAT | F_E | F_ADC_Z | F_SPOIL | F_RESET | F_PD | F_PD_RESET | F_D | F_GS | F_MAT0 | F_FOLD | F_FOLD_SPOIL;
    if ((f & need) != need || (f & other)) return -1;
    if ((f & F_S) && shift != 1) return -1;
    const int kind = (f & F_TX) ? 1 : ((f & F_TY) ? 2 : 0);
    // the accumulation runs the rotation's own pattern: every present partial must have it (the partial of a rotation about x
    // or y w.r.t. the flip angle or a relaxation time has; w.r.t. the phase it has not: the flag-tested body takes those)
    for (int v = 0; v < n_vars; ++v) {
        if (!(present & (1u << v))) continue;
        const int pat = (present & (256u << v)) ? 1 : ((present & (65536u << v)) ? 2 : 0);
        if (kind != 0 && pat != kind) return -1;
    }
    return kind | (kind << 2) | ((f & F_S0) ? 16 : 0) | ((f & F_S) ? 32 : 0);
}

#ifndef EPGX_DF3_SPLIT
#define EPGX_DF3_SPLIT 1      // three derivative states of a run folded at run time: two launches (epgx_run: the last variable, then the
#endif                        // first two); the host then folds whatever the number of rotation partials (build_range)
// the same for a record folded at run time (the host's fold pass in build_range builds them)
// `spoiled`: a spoiler folded into the record (F_FOLD_SPOIL) is allowed -- the loop at 16 / 32 orders handles it, drun_kernel not
__host__ __device__ inline int dfold_shape(uint32_t f, uint32_t present, int n_vars, bool spoiled = false) {
    const uint32_t need = F_T | F_T0 | F_FOLD | F_ADC;
    const uint32_t other = F_MAT | F_E | F_ADC_Z | F_SPOIL | F_RESET | F_PD | F_PD_RESET | F_D | F_GS | F_MAT0 | (spoiled ? 0u : (uint32_t)F_FOLD_SPOIL);
    if ((f & need) != need || (f & other)) return -1;
    const int kind = (f & F_TX) ? 1 : ((f & F_TY) ? 2 : 0);
    for (int v = 0; v < n_vars; ++v) {
        if (!(present & (1u << v))) continue;
        const int pat = (present & (256u << v)) ? 1 : ((present & (65536u << v)) ? 2 : 0);
        if (kind != 0 && pat != kind) return -1;
    }
    return kind | (kind << 2) | ((f & F_S0) ? 16 : 0) | ((f & F_S) ? 32 : 0) | (int)DRUN_FOLD;
}

}  // namespace epgx

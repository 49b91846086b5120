// epgx_lanes_bodies.h -- the record bodies of rows_grow_lanes_kernel (epgx_grow_lanes_kernels.hip.h): which chains a record
// runs there, and which of them have a body specialised on those chains.  Plain C++: the kernel dispatches on lanes_body_id,
// the launcher (epgx_launch_grow.h) names the bodies of a list in its trace line with the same function.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "epgx_records.h"

namespace epgx {

// the chains the rows code runs for a record (rows_T / rows_generic; a record without a leaf runs the plain chains) --
// tk: 0 no rotation, 1 cell_T, 2 cell_TX_sumdiff, 3 cell_TY; ek: 0 no relaxation, 1 cell_E, 2 cell_ER
constexpr int lanes_tk(uint32_t f, uint32_t head) {
    return !(f & F_T) ? 0 : ((f & F_TX) ? 2 : (((f & F_TY) && head != LEAF_NONE) ? 3 : 1));
}
constexpr int lanes_ek(uint32_t f) { return !(f & F_E) ? 0 : ((f & F_ER) ? 2 : 1); }

// The specialised bodies: X(id, leading shift, trailing shift, tk, t0, ek, cells per block, name).  A record whose shifts and
// kinds are not listed runs the generic per-cell body (id -1, "generic"), and so does every record under EPGX_LANES_BODY=0.
//   echo-x   the folded echo S T0 S (run-time fold or fused on the host): what a spin-echo train repeats
// One entry: bodies for the excitation (tk 1 / 3) and for the halves of an unfused echo (tk 2 with ek 1 / 2, ek alone) were
// written and taken out again -- each of them next to the generic body took the kernel beyond 256 VGPRs.
// A list in which every record behind the head records (no leading shift, nothing shifted yet: one cell of the generic body)
// is listed here is a TRAIN (LanesPlan::train): it runs the instantiation of the kernel that has these bodies and no generic one.
#define EPGX_LANES_BODIES(X) X(0, 1, 1, 2, true, 0, 4, "echo-x")
constexpr int LANES_N_BODIES = 1;

constexpr int lanes_body_id(uint32_t f, uint32_t head) {
    const int i = (f & F_S0) ? 1 : 0, o = (f & F_S) ? 1 : 0, tk = lanes_tk(f, head), ek = lanes_ek(f);
    const bool t0 = (f & F_T0) != 0;
#define EPGX_LANES_MATCH(id, I, O, TK, T0, EK, B, name) \
    if (i == I && o == O && tk == TK && t0 == T0 && ek == EK) return id;
    EPGX_LANES_BODIES(EPGX_LANES_MATCH)
#undef EPGX_LANES_MATCH
    return -1;
}

// the one record rows_grow_lanes_kernel_odd (epgx_grow_lanes_odd_kernels.hip.h) runs behind the head records, and the one
// LanesPlan::odd admits there: the folded echo about x -- leading and trailing shift, a rotation about x with its constant
// term, no relaxation stage.  Kernel and planner test this one predicate: a second body with both shifts added to the table
// above does not become `odd` by itself
constexpr bool lanes_odd_echo(uint32_t f, uint32_t head) {
    return (f & F_S0) != 0 && (f & F_S) != 0 && lanes_tk(f, head) == 2 && (f & F_T0) != 0 && lanes_ek(f) == 0;
}

// the bodies the records of a cut list run, in the order of their first use: "exc-y/1+echo-x/4", "generic", ...
inline std::string lanes_body_names(const std::vector<Rec> &grow, bool specialised) {
    static const char *const names[LANES_N_BODIES] = {
#define EPGX_LANES_NAME(id, I, O, TK, T0, EK, B, name) name "/" #B,
        EPGX_LANES_BODIES(EPGX_LANES_NAME)
#undef EPGX_LANES_NAME
    };
    bool seen[LANES_N_BODIES + 1] = {};
    std::string out;
    size_t members = 0;
    for (const Rec &r : grow) {   // (headers of runs are not records: as lanes_plan and the kernel walk the list)
        const uint32_t f = r.flags, head = f >> 24;
        if (!members && (head == LEAF_PAIR || head == LEAF_SINGLE)) {
            members = (size_t)(head == LEAF_PAIR ? 2 : 1) * (size_t)((uint32_t)r.kmax >> 16);
            continue;
        }
        if (members) --members;
        const int id = specialised ? lanes_body_id(f, head) : -1;
        bool &s = seen[id < 0 ? LANES_N_BODIES : id];
        if (s) continue;
        s = true;
        if (!out.empty()) out += "+";
        out += id < 0 ? "generic" : names[id];
    }
    return out;
}

}  // namespace epgx

// epgx_planner.cpp -- launch planning on host data alone (epgx_planner.h): no HIP call, no device pointer.
#include "epgx_planner.h"
#include "epgx_lanes_bodies.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>

namespace epgx {

// Pack primitives [begin, end) into fused records  [misc] -> [T] -> [E] -> [S] -> [ADC].
// "S E" is rewritten "E S" first: E multiplies every order by the same coefficients and S only
// moves values, so the two commute bit for bit (the wrap value conj(B_1) * e0 equals
// conj(B_1 * conj(e0)) exactly); nothing else is reordered.
// which table of logarithmic partials (epgx_plan::logtabs) the relaxation stage of a record has for every variable
void pack_records(const PlanHost &ph, int begin, int end, int K, const Knobs &kn, std::vector<Rec> &out, std::vector<DRec> &dout,
                  bool &use_lds, bool &has_adc, std::vector<ELog> &elog) {
    const std::vector<epgx_op> &all = ph.ops;
    const std::vector<uint8_t> &zero_pattern = ph.zero_pattern;
    const std::vector<epgx_dop> &dops = ph.dops;
    const std::vector<uint16_t> &dpattern = ph.dpattern;
    const std::vector<int32_t> &log_of = ph.log_of;
    const bool fold = ph.fold;
    const uint32_t identity_off = (uint32_t)(ph.n_pool * 8);
    std::vector<epgx_op> ops;
    for (int i = begin; i < end; ++i)
        if (all[i].opcode != EPGX_OP_NOP) {
            ops.push_back(all[i]);
            // travels with the operator through the reordering: zero pattern in the low byte, the
            // primitive's index (for its partial derivatives) above it
            ops.back().reserved = (int32_t)zero_pattern[i] | (i << 8);
        }
    const bool deriv = !dops.empty();
    for (bool swapped = true; swapped;) {
        swapped = false;
        for (size_t i = 0; i + 1 < ops.size(); ++i)
            if (ops[i].opcode == EPGX_OP_S && ops[i + 1].opcode == EPGX_OP_E) {
                std::swap(ops[i], ops[i + 1]);
                swapped = true;
            }
    }
    auto table_ix = [](const epgx_op &op) -> uint32_t {
        if (op.space < 0) return 0u;  // same entry for every voxel
        return (uint32_t)(op.ncoef * 8) | ((uint32_t)op.space << 24);  // entry bytes | index space
    };
    out.clear();
    dout.clear();
    use_lds = has_adc = false;
    Rec cur;
    DRec dcur;
    ELog lcur;
    memset(&cur, 0, sizeof(cur));
    memset(&dcur, 0, sizeof(dcur));
    auto no_logs = [&]() {
        for (int v = 0; v < EPGX_MAX_VARS; ++v) lcur.tab[v] = -1;
        lcur.blocked = false;
        lcur.t_op = -1;
    };
    no_logs();
    elog.clear();
    int stage = 0;  // 1 misc, 2 leading S(+1), 3 T/MAT, 4 E, 5 S, 6 ADC
    auto flush = [&]() {   // (the leaf numbers are assigned at the end, after the fold pass)
        if (stage) {
            out.push_back(cur);
            if (deriv) dout.push_back(dcur);
            if (deriv) elog.push_back(lcur);
        }
        memset(&cur, 0, sizeof(cur));
        memset(&dcur, 0, sizeof(dcur));
        no_logs();
        stage = 0;
    };
    auto partials = [&](const epgx_op &op, bool t_stage) {
        if (!deriv) return;
        const epgx_dop &dp = dops[(size_t)(op.reserved >> 8)];
        const uint32_t pattern = dpattern[(size_t)(op.reserved >> 8)];
        for (int v = 0; v < EPGX_MAX_VARS; ++v) {
            if (dp.coef_off[v] < 0) continue;
            const uint32_t pat = (pattern >> (2 * v)) & 3u;
            if (pat == 1) dcur.present |= (t_stage ? 256u : 4096u) << v;
            if (pat == 2 && t_stage) dcur.present |= 65536u << v;
            const bool with_const = t_stage && (pattern & (256u << v));   // generated partial of a T0 table: 14 per entry
            const uint32_t bytes = t_stage ? (with_const ? 112u : 80u) : 32u;
            const uint32_t ix = dp.space[v] < 0 ? 0u : (bytes | ((uint32_t)dp.space[v] << 24));
            if (ph.second && v < ph.n_vars - 1) {   // which cross terms of the H row this stage takes: the host's decision
                if (dp.reserved & (v == 0 ? EPGX_HESS_CROSS_A : EPGX_HESS_CROSS_B))
                    dcur.pad0 |= (v == 0 ? (t_stage ? HESS_T_XA : HESS_E_XA) : (t_stage ? HESS_T_XB : HESS_E_XB));
            }
            if (t_stage) {
                dcur.t_off[v] = (uint32_t)(dp.coef_off[v] * 8);
                dcur.t_ix[v] = ix;
                dcur.present |= 1u << v;
                if (with_const) {   // the partial of the constant term sits where a relaxation partial would: slots 10..12 of the
                    dcur.e_off[v] = dcur.t_off[v] + 80u;   // partial line; such a record has no relaxation stage (below)
                    dcur.e_ix[v] = ix;
                    dcur.present |= 16u << v;
                }
            } else {
                dcur.e_off[v] = (uint32_t)(dp.coef_off[v] * 8);
                dcur.e_ix[v] = ix;
                dcur.present |= 16u << v;
                const int32_t tab = !log_of.empty() ? log_of[(size_t)(op.reserved >> 8) * EPGX_MAX_VARS + v] : -1;
                lcur.tab[v] = tab;
                if (tab < 0) lcur.blocked = true;
            }
        }
    };
    auto is_matrix = [](const epgx_op &op) {
        return op.opcode == EPGX_OP_T || op.opcode == EPGX_OP_T0 || op.opcode == EPGX_OP_MAT || op.opcode == EPGX_OP_MAT0;
    };
    for (size_t oi = 0; oi < ops.size(); ++oi) {
        const epgx_op &op = ops[oi];
        int st;
        switch (op.opcode) {
        case EPGX_OP_T: case EPGX_OP_T0: case EPGX_OP_MAT: case EPGX_OP_MAT0: st = 3; break;
        case EPGX_OP_E: st = 4; break;
        case EPGX_OP_S:
            // "S T ..." : a shift by +1 (no truncation) directly in front of a rotation opens the
            // record of that rotation instead of being a record of its own -- every record costs
            // a dependent scalar fetch that the wave has to sit out
            // (only when the shift could not close the current record anyway, and when the rotation
            // is not followed by an E: those shapes have straight-line bodies)
            // (also behind a lone rotation when the NEXT rotation is followed by a shift of its own -- "T | S T S ..." : the
            // excitation of a train.  The shift saves no record either way, and the first repetition of the train then has the
            // shape of the others, so that the run-length folding takes all of them: EPGX_LEAD_FORWARD=0, measurements)
            st = ((stage == 0 || stage >= 5 ||
                   (stage == 3 && kn.lead_forward && oi + 2 < ops.size() && ops[oi + 2].opcode == EPGX_OP_S && ops[oi + 2].ia == 1)) &&
                  op.ia == 1 && op.ib >= K - 1 && oi + 1 < ops.size() && is_matrix(ops[oi + 1]) &&
                  !(oi + 2 < ops.size() && ops[oi + 2].opcode == EPGX_OP_E))
                     ? 2
                     : 5;
            break;
        case EPGX_OP_ADC: st = 6; break;
        default: st = 1; break;
        }
        if (st <= stage || st == 1) flush();
        if (deriv && st == 4 && (cur.flags & F_T0) && (dcur.present & 0x70u)) flush();   // (the relaxation-partial slots are taken)
        switch (op.opcode) {
        case EPGX_OP_T: case EPGX_OP_T0: case EPGX_OP_MAT: case EPGX_OP_MAT0:
            cur.flags |= (op.opcode == EPGX_OP_T)    ? F_T
                         : (op.opcode == EPGX_OP_T0) ? (F_T | F_T0)
                         : (op.opcode == EPGX_OP_MAT) ? F_MAT
                                                      : (F_MAT | F_MAT0);
            if ((op.opcode == EPGX_OP_T || op.opcode == EPGX_OP_T0) && (op.reserved & 0xff) == 1) cur.flags |= F_TX;
            if ((op.opcode == EPGX_OP_T || op.opcode == EPGX_OP_T0) && (op.reserved & 0xff) == 3) cur.flags |= F_TY;
            partials(op, true);
            lcur.t_op = op.reserved >> 8;
            cur.t_off = (uint32_t)(op.coef_off * 8);
            cur.t_ix = table_ix(op);
            break;
        case EPGX_OP_E:
            cur.flags |= F_E | ((op.reserved & 0xff) == 2 ? F_ER : 0u);
            partials(op, false);
            cur.e_off = (uint32_t)(op.coef_off * 8);
            cur.e_ix = table_ix(op);
            break;
        case EPGX_OP_S:
            if (st == 2) {
                cur.flags |= F_S0;
                break;
            }
            cur.flags |= F_S;
            cur.shift = op.ia;
            if (op.ib < K - 1) {
                cur.flags |= F_TRUNC;
                cur.kmax = op.ib;
            }
            if (std::abs(op.ia) > 1) use_lds = true;
            break;
        case EPGX_OP_ADC:
            cur.flags |= F_ADC | (op.ib ? F_ADC_Z : 0u);
            cur.slot = op.ia;
            has_adc = true;
            break;
        case EPGX_OP_D: case EPGX_OP_GS:
            cur.flags |= (op.opcode == EPGX_OP_D) ? F_D : F_GS;
            cur.t_off = (uint32_t)(op.coef_off * 8);
            cur.t_ix = table_ix(op);
            if (op.opcode == EPGX_OP_GS) use_lds = true;
            st = 7;  // nothing else may join this record
            break;
        case EPGX_OP_SPOIL: cur.flags |= F_SPOIL; break;
        case EPGX_OP_RESET: cur.flags |= F_RESET; break;
        case EPGX_OP_PD:
            cur.flags |= F_PD | (op.ia ? F_PD_RESET : 0u);
            cur.e_off = (uint32_t)(op.coef_off * 8);
            cur.e_ix = table_ix(op);
            st = 4;  // the E slot of this record is taken
            break;
        default: break;
        }
        stage = st;
    }
    flush();

    // ---- run-time fold (F_FOLD, fold_T in epgx_kernels.hip.h).  A rotation next to precession-free relaxations whose
    // tables do not share its index space -- T over a B1 axis, E over (T1, T2): the product table would be the whole grid
    // PER PULSE, so the host's E.T.E fusion (epgx_fuse) does not apply -- becomes ONE stage  E_a . T . E_b  whose
    // coefficients every wavefront computes for its voxels when it meets the record: 3 instructions per record instead of
    // 6 per order and relaxation.  E_a = the relaxation stage of the record itself; E_b = the relaxation that closes the
    // PREVIOUS record (it commutes with the integer shift and the truncation behind it: E scales every order alike, and
    // the recovery only touches Z_0, which a shift does not move).  An ADC behind E_b pins it; so does a reset or density
    // stage in front of the rotation.  A SPOILER there is folded as well (F_FOLD_SPOIL: zero F columns).  The decisions only look at neighbours inside one ADC-to-ADC
    // span, so the per-timestep launches (ranges cut at the probes) and the state-resident launch of the whole
    // sequence fold alike -- the same chains in the same order in every kernel (same bits; the one exception is the sum /
    // difference form of rotations about x in the 64-order state-resident kernels: last bits, include/epgx.h epgx_run).
    // (The decision is per PLAN, never per launch capacity: the same plan must run the same chains at every K.  A host
    // that runs a plan with 16 orders per voxel sets EPGX_PLAN_NO_FOLD: with one order per lane a relaxation stage is 6
    // instructions per record, less than the fold's extra loads cost -- the 1000-TR MRF train with max_nstate = 10 takes
    // 28.2 ms unfolded and 35.6 ms folded at K = 16; K = 32: 43.8 / 33.2 ms.)
    if (fold && !deriv) {
        const uint32_t misc = F_SPOIL | F_RESET | F_PD | F_PD_RESET;
        for (size_t j = 0; j < out.size(); ++j) {
            Rec &c = out[j];
            if (!(c.flags & F_T) || (c.flags & (F_MAT | F_T0 | F_FOLD | F_D | F_GS | F_PD))) continue;
            if ((c.flags & F_S) && c.shift != 1) continue;             // the shift word is about to carry E_b's table
            if ((c.flags & F_E) && !(c.flags & F_ER)) continue;        // precession behind the rotation: not a real diagonal
            const bool has_a = (c.flags & F_E) != 0;
            // a spoiler right in front of the rotation (and no reset / density stage with it) joins the fold: F <- 0 means
            // that T only sees Z, i.e. the F columns of E_b count as zero; E_b itself commutes with the spoiler
            const bool spoil = (c.flags & F_SPOIL) && !(c.flags & (misc & ~(uint32_t)F_SPOIL));
            Rec *p = j > 0 ? &out[j - 1] : nullptr;
            const bool has_b = p && (p->flags & F_E) && (p->flags & F_ER) && !(c.flags & (misc & ~(uint32_t)F_SPOIL)) &&
                               !(p->flags & (F_ADC | F_ADC_Z | F_PD | F_PD_RESET | F_D | F_GS | F_FOLD));
            if (!has_a && !has_b && !spoil) continue;
            const uint32_t a_off = has_a ? c.e_off : identity_off, a_ix = has_a ? c.e_ix : 0u;
            c.flags = (c.flags & ~(uint32_t)(F_E | F_ER)) | F_FOLD | F_T0;
            if (spoil) c.flags = (c.flags & ~(uint32_t)F_SPOIL) | F_FOLD_SPOIL;
            c.e_off = a_off;
            c.e_ix = a_ix;
            c.shift = (int32_t)(has_b ? p->e_off : identity_off);
            if (has_b) {
                if (p->e_ix & 0xffffffu) c.flags |= F_FOLD_BVOX | (((p->e_ix >> 24) & 3u) << 21);
                p->flags &= ~(uint32_t)(F_E | F_ER);
                p->e_off = p->e_ix = 0;
                // what is left of the previous record: nothing, or a lone S(+1) that can lead this record
                const uint32_t rest = p->flags & 0xffffffu;
                const bool lone_shift = (rest & ~(uint32_t)F_TRUNC) == F_S && p->shift == 1 && !(c.flags & F_S0) &&
                                        (!(rest & F_TRUNC) || !(c.flags & F_S));   // (one kmax per record: the trailing shift's)
                if (lone_shift) {
                    c.flags |= F_S0 | (rest & F_TRUNC);
                    if (rest & F_TRUNC) c.kmax = p->kmax;
                    p->flags = 0;
                }
            }
        }
        out.erase(std::remove_if(out.begin(), out.end(), [](const Rec &r) { return (r.flags & 0xffffffu) == 0; }), out.end());
    }
    for (Rec &r : out)   // K < 64 always runs rows_kernel, whose leaves truncate themselves (see record_leaf)
        r.flags = (r.flags & 0xffffffu) | ((K < 64 ? record_leaf<true>(r.flags, r.shift) : record_leaf<false>(r.flags, r.shift)) << 24);
}

// The run-folded record list of a launch that starts from EQUILIBRIUM (one populated order), cut where the populated orders
// outgrow 16 and 32 (rows_grow_kernel: the reference grows its state matrix the same way, functions.py:135 / shift.py:86).
// `top` = the highest order that can hold anything: every S(+-1) of a record adds one (resets and truncations are ignored:
// `top` only ever over-estimates, which is safe).  Repeat-count records and header runs are cut at the boundaries.
// work[p] = the record executions of range p.
void grow_split(const std::vector<Rec> &runs, std::vector<Rec> &out, int &n1, int &n2, double work[3]) {
    auto shifts_of = [](const Rec &r) { return ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0); };
    static const int cap[3] = {15, 31, 1 << 30};
    int top = 0, phase = 0;
    n1 = n2 = -1;
    work[0] = work[1] = work[2] = 0.0;
    auto next_phase = [&]() {
        if (phase == 0) n1 = (int)out.size();
        else n2 = (int)out.size();
        ++phase;
    };
    for (size_t i = 0; i < runs.size();) {
        const Rec &r = runs[i];
        const uint32_t head = r.flags >> 24;
        const int count = (int)((uint32_t)r.kmax >> 16);
        if (head == LEAF_PAIR || head == LEAF_SINGLE) {
            const int per = head == LEAF_PAIR ? 2 : 1;   // records per repetition
            int d = 0;
            for (int j = 0; j < per; ++j) d += shifts_of(runs[i + 1 + (size_t)j]);
            int done = 0;
            while (done < count) {
                int m = d > 0 ? (cap[phase] - top) / d : count - done;
                m = std::min(m, count - done);
                if (m <= 0) {
                    next_phase();
                    continue;
                }
                Rec h = r;
                h.kmax = m << 16;
                out.push_back(h);
                for (int j = 0; j < per * m; ++j) out.push_back(runs[i + 1 + (size_t)(per * done + j)]);
                work[phase] += (double)per * m;
                top += m * d;
                done += m;
            }
            i += 1 + (size_t)per * (size_t)count;
            continue;
        }
        const int d = shifts_of(r), rep = std::max(count, 1);
        int done = 0;
        while (done < rep) {
            int m = d > 0 ? (cap[phase] - top) / d : rep - done;
            m = std::min(m, rep - done);
            if (m <= 0) {
                next_phase();
                continue;
            }
            Rec c = r;
            c.kmax = (r.kmax & 0xffff) | (m << 16);
            if (r.flags & F_ADC) c.slot = r.slot + done;   // (a repeat count implies consecutive ADC rows)
            out.push_back(c);
            work[phase] += m;
            top += m * d;
            done += m;
        }
        ++i;
    }
    if (n1 < 0) n1 = (int)out.size();
    if (n2 < 0) n2 = (int)out.size();
    n1 = std::min(n1, n2);
}

// The orders per voxel the three ranges [0, n1), [n1, n2), [n2, end) of a cut list NEED (rows_grow_kernel writes no state: its
// only outputs are the order-0 probes).  A coefficient of order k reaches order 0 through k shifts and through nothing else, so
// at a record execution with `rem` shifts left up to the last probe of the list (its own included: a record shifts before it
// probes) the orders above `rem` are dead, and the orders above `top` (grow_split) are empty: the execution needs
// 1 + min(top, rem) orders, a range the maximum over its executions.  Like `top`, `rem` only ever over-estimates (resets,
// spoilers and truncations are ignored).  Records behind the last probe need nothing; a list without a probe keeps 16 / 32 / 64.
// cap[p] = the smallest of 16 / 32 / 64 that holds the need of range p, never more than the range has today.
void grow_reach(const std::vector<Rec> &list, int n1, int n2, int cap[3]) {
    auto shifts_of = [](const Rec &r) { return ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0); };
    struct Exec { int range, d, rep, top0; bool adc; };   // a record of the list: `rep` executions of `d` shifts each from top0 on
    std::vector<Exec> ex;
    int top = 0;
    for (size_t i = 0, members = 0; i < list.size(); ++i) {
        const Rec &r = list[i];
        const uint32_t head = r.flags >> 24;
        const int count = (int)((uint32_t)r.kmax >> 16);
        if (!members && (head == LEAF_PAIR || head == LEAF_SINGLE)) {   // (a header's low flag bits are a shape code, not flags)
            members = (size_t)(head == LEAF_PAIR ? 2 : 1) * (size_t)count;
            continue;
        }
        const int rep = members ? 1 : std::max(count, 1);
        if (members) --members;
        ex.push_back({(int)i < n1 ? 0 : ((int)i < n2 ? 1 : 2), shifts_of(r), rep, top, (r.flags & F_ADC) != 0});
        top += rep * ex.back().d;
    }
    static const int today[3] = {16, 32, 64};
    int need[3] = {0, 0, 0};
    bool probed = false;
    long rem = 0;   // shifts behind the record at hand up to the last probe
    for (size_t q = ex.size(); q-- > 0;) {
        const Exec &x = ex[q];
        if (!probed && !x.adc) continue;
        probed = true;
        for (int e = x.rep - 1; e >= 0; --e) {
            rem += x.d;
            const long t = (long)x.top0 + (long)x.d * (e + 1);
            need[x.range] = (int)std::max<long>(need[x.range], 1 + std::min(t, rem));
        }
    }
    for (int p = 0; p < 3; ++p) cap[p] = !probed ? today[p] : std::min(today[p], need[p] <= 16 ? 16 : (need[p] <= 32 ? 32 : 64));
}

// see epgx_planner.h.  `top` and `rem` are counted exactly as the kernel counts them (every S(+1) of a record, leading or
// trailing; resets and truncations cannot occur), so L is the largest window the kernel will ever open.
LanesPlan lanes_plan(const std::vector<Rec> &grow, bool has_in, bool has_out, const Knobs &kn) {
    LanesPlan lp;
    auto refuse = [&](const char *why) {
        lp.eligible = false;
        lp.why = why;
        return lp;
    };
    if (kn.lanes <= 0) return refuse("EPGX_LANES=0");
    if (has_in || has_out) return refuse("a state input or output");
    if (grow.empty()) return refuse("no growing record list");
    struct Exec { int d, rep; bool adc, body, lead, odd_echo; };
    std::vector<Exec> ex;
    size_t members = 0;
    for (const Rec &r : grow) {
        const uint32_t f = r.flags, head = f >> 24;
        const int count = (int)((uint32_t)r.kmax >> 16);
        if (!members && (head == LEAF_PAIR || head == LEAF_SINGLE)) {   // (a header's low flag bits are a shape code, not flags)
            members = (size_t)(head == LEAF_PAIR ? 2 : 1) * (size_t)count;
            continue;
        }
        const int rep = members ? 1 : std::max(count, 1);
        if (members) --members;
        if (f & F_TRUNC) return refuse("a truncation below the capacity");
        if (f & (F_SPOIL | F_FOLD_SPOIL)) return refuse("a spoiler");
        if (f & F_RESET) return refuse("a reset");
        if (f & (F_PD | F_PD_RESET)) return refuse("a density stage");
        if (f & F_GS) return refuse("an n-D shift");
        if (f & F_D) return refuse("diffusion");
        if (f & (F_MAT | F_MAT0)) return refuse("a general matrix");
        if (f & F_ADC_Z) return refuse("a Z0 probe");
        if ((f & F_S) && !(f & F_FOLD) && r.shift != 1) return refuse(r.shift == -1 ? "S(-1)" : "a shift by more than one order");
        if ((f & F_T0) && !(f & F_T)) return refuse("a constant term without a rotation");
        ex.push_back({((f & F_S0) ? 1 : 0) + ((f & F_S) ? 1 : 0), rep, (f & F_ADC) != 0, lanes_body_id(f, head) >= 0, (f & F_S0) != 0, lanes_odd_echo(f, head)});
    }
    // the shifts up to the last probe (a record shifts before it probes), then shift by shift: between two shifts the state
    // holds 1 + min(top, rem) live orders
    size_t last = ex.size();
    for (size_t q = 0; q < ex.size(); ++q)
        if (ex[q].adc) last = q;
    if (last == ex.size()) return refuse("no probe");
    long rem = 0;
    for (size_t q = 0; q <= last; ++q) rem += (long)ex[q].d * ex[q].rep;
    lp.rem0 = (int)std::min<long>(rem, 1 << 30);
    long top = 0, need = 1;
    for (size_t q = 0; q <= last; ++q)
        for (long s = (long)ex[q].d * ex[q].rep; s > 0; --s) {
            ++top;
            --rem;
            need = std::max(need, 1 + std::min(top, rem));
        }
    lp.L = (int)std::min<long>(need, 1 << 30);
    if (need > LANES_MAX_ORDERS) return refuse("more than 24 live orders");
    lp.eligible = true;
    // a train: head records, then bodies only.  A head record executes while nothing has shifted yet and has no leading shift
    // (its window is order 0 alone; a trailing shift is where its one cell puts the result), once if it shifts
    lp.train = true;
    top = 0;
    for (const Exec &x : ex) {
        const bool head_rec = top == 0 && !x.lead && (x.d == 0 || x.rep == 1);
        if (!head_rec && !x.body) lp.train = false;
        top += (long)x.d * x.rep;
    }
    // the odd class alone: every record behind the head records has both shifts and is the folded echo the kernel runs
    // (lanes_odd_echo: the kernel skips anything else), starts at an even `top` (the head records have not shifted) and leaves
    // an even `rem`
    lp.odd = lp.train && lp.rem0 % 2 == 0;
    top = 0;
    for (const Exec &x : ex) {
        const bool head_rec = top == 0 && !x.lead && (x.d == 0 || x.rep == 1);
        if (head_rec ? x.d != 0 : !(x.lead && x.d == 2 && x.odd_echo)) lp.odd = false;
        top += (long)x.d * x.rep;
    }
    return lp;
}

// what a launch needs to know about the packed records of a range
static void range_facts(RangeLists &pr) {
    const std::vector<Rec> &recs = pr.recs;
    pr.n_rec = (int)recs.size();
    for (const Rec &r : recs) pr.big_shift = pr.big_shift || ((r.flags & F_S) && !(r.flags & F_FOLD) && std::abs(r.shift) > 1);
    for (const Rec &r : recs) pr.has_gs = pr.has_gs || (r.flags & F_GS);
    pr.seq_slots = true;
    int expect = -1;
    for (const Rec &r : recs) pr.has_pd = pr.has_pd || (r.flags & F_PD);
    for (const Rec &r : recs)
        if (r.flags & F_ADC) {
            if (expect < 0) pr.first_slot = r.slot;
            else if (r.slot != expect) pr.seq_slots = false;
            expect = r.slot + 1;
        }
    {
        std::vector<std::pair<uint32_t, uint32_t>> seen;
        auto fresh = [&](uint32_t off, uint32_t ix) {
            if ((ix & 0xffffffu) == 0) return false;   // same entry for every voxel: hot in the caches
            for (auto &q : seen)
                if (q.first == off && q.second == ix) return false;
            if (seen.size() < 4096) seen.emplace_back(off, ix);
            return true;
        };
        for (int i = 0; i < pr.n_rec; ++i) {
            const Rec &r = recs[(size_t)i];
            bool any = false;
            if (r.flags & (F_T | F_MAT | F_D | F_GS)) any |= fresh(r.t_off, r.t_ix);
            if (r.flags & (F_E | F_PD)) any |= fresh(r.e_off, r.e_ix);
            if (any) pr.pf_count = i + 1;
        }
    }
}

// Folded copy of the records for rows_kernel<.., RUNS>:
//  * a run of identical records (an MSE train: same shape, same table entries, consecutive ADC rows) becomes one
//    record with a repeat count in the upper half of the kmax word (rows_run);
//  * a run of >= 4 record PAIRS [T, E, S(+1)?, ADC] [E, S(+1)] of constant shapes but arbitrary tables (the repetitions of an
//    SSFP / MRF train that cannot be fused) gets a header record in front (leaf byte LEAF_PAIR, shape code, number
//    of pairs): rows_pair_run.
// Kept when it saves a quarter of the records or pair runs cover half of them.
static void fold_runs(RangeLists &pr, int K) {
    const std::vector<Rec> &recs = pr.recs;
    const std::vector<DRec> &drecs = pr.drecs;
    std::vector<Rec> &runs = pr.runs;
    if (K <= 64 && drecs.empty() && pr.n_rec) {
        auto leaf_of = [&](const Rec &r) {   // with the truncation handled inside the leaf (K = 64 records carry LEAF_NONE for it)
            const uint32_t l = r.flags >> 24;
            return (l == LEAF_NONE && (r.flags & F_TRUNC)) ? record_leaf<true>(r.flags & 0xffffffu, r.shift) : l;
        };
        auto pair_code = [&](const Rec &a, const Rec &b) -> int {   // -1: not a pair this kernel loops over
            int code = -1;
            for (int c = 0; c < 16 && code < 0; ++c)
                if (leaf_of(a) == leaf_id((c & 1) ? 2 : 1, (c & 2) ? 2 : 1, (c & 8) != 0, true, false) &&
                    leaf_of(b) == leaf_id(0, (c & 4) ? 2 : 1, true, false, false))
                    code = c;
            return code;
        };
        // (same stages AND same table geometry -- entry size and index space: the kernel hoists the per-lane entry offsets)
        auto same_shape = [](const Rec &x, const Rec &y) {
            return x.flags == y.flags && x.shift == y.shift && x.kmax == y.kmax && x.t_ix == y.t_ix && x.e_ix == y.e_ix;
        };
        // run of folded records of one shape (rows_single_run): stages and table geometry equal, table offsets free
        auto single_code = [&](const Rec &a) -> int {
            if (!(a.flags & F_FOLD)) return -1;
            for (int c = 0; c < 16; ++c)
                if (leaf_of(a) == leaf_id((c & 1) ? 4 : 3, 0, (c & 4) != 0, (c & 8) != 0, (c & 2) != 0)) return c;
            return -1;
        };
        auto same_fold_shape = [](const Rec &x, const Rec &y) {
            return x.flags == y.flags && (x.kmax & 0xffff) == (y.kmax & 0xffff) && x.t_ix == y.t_ix && x.e_ix == y.e_ix;
        };
        auto identical = [](const Rec &x, const Rec &y) {
            return x.flags == y.flags && x.shift == y.shift && x.kmax == y.kmax && x.t_off == y.t_off && x.e_off == y.e_off &&
                   x.t_ix == y.t_ix && x.e_ix == y.e_ix;
        };
        size_t in_pairs = 0;
        bool back_is_plain = false;   // runs.back() is an ordinary record (not part of a pair run): a repeat may fold into it
        for (int i = 0; i < pr.n_rec;) {
            const int scode = single_code(recs[(size_t)i]);
            if (scode >= 0 && !(i + 1 < pr.n_rec && identical(recs[(size_t)i], recs[(size_t)i + 1]))) {
                int n = 1;   // (a train of IDENTICAL records is folded into a repeat count instead, below)
                while (i + n < pr.n_rec && n < 0x7fff && same_fold_shape(recs[(size_t)i], recs[(size_t)i + n]) &&
                       !(i + n + 1 < pr.n_rec && identical(recs[(size_t)i + n], recs[(size_t)i + n + 1])))
                    ++n;
                if (n >= 4) {
                    Rec head;
                    memset(&head, 0, sizeof(head));
                    head.flags = (LEAF_SINGLE << 24) | (uint32_t)scode;
                    head.kmax = n << 16;
                    runs.push_back(head);
                    for (int j = 0; j < n; ++j) {
                        runs.push_back(recs[(size_t)i + j]);
                        runs.back().kmax = (runs.back().kmax & 0xffff) | (1 << 16);
                    }
                    in_pairs += (size_t)n;
                    i += n;
                    back_is_plain = false;
                    continue;
                }
            }
            int code = i + 1 < pr.n_rec ? pair_code(recs[(size_t)i], recs[(size_t)i + 1]) : -1;
            int npairs = 0;
            if (code >= 0) {
                npairs = 1;
                while (i + 2 * npairs + 1 < pr.n_rec && npairs < 0x7fff && same_shape(recs[(size_t)i], recs[(size_t)i + 2 * npairs]) &&
                       same_shape(recs[(size_t)i + 1], recs[(size_t)i + 2 * npairs + 1]))
                    ++npairs;
            }
            if (npairs >= 4) {
                Rec head;
                memset(&head, 0, sizeof(head));
                head.flags = (LEAF_PAIR << 24) | (uint32_t)code;
                head.kmax = npairs << 16;
                runs.push_back(head);
                for (int j = 0; j < 2 * npairs; ++j) {
                    runs.push_back(recs[(size_t)i + j]);
                    runs.back().kmax = (runs.back().kmax & 0xffff) | (1 << 16);
                }
                in_pairs += 2 * (size_t)npairs;
                i += 2 * npairs;
                back_is_plain = false;
                continue;
            }
            const Rec &r = recs[(size_t)i];
            bool same = false;
            if (back_is_plain && (r.flags >> 24) != LEAF_NONE) {
                const Rec &q = runs.back();
                const int rep = (int)((uint32_t)q.kmax >> 16);
                same = q.flags == r.flags && q.shift == r.shift && (q.kmax & 0xffff) == r.kmax && q.t_off == r.t_off &&
                       q.e_off == r.e_off && q.t_ix == r.t_ix && q.e_ix == r.e_ix && rep < 0x7fff &&
                       (!(r.flags & F_ADC) || r.slot == q.slot + rep);
            }
            if (same) runs.back().kmax += 1 << 16;
            else {
                runs.push_back(r);
                runs.back().kmax = (r.kmax & 0xffff) | (1 << 16);
                back_is_plain = true;
            }
            ++i;
        }
        if (runs.size() * 4 > (size_t)pr.n_rec * 3 && in_pairs * 2 < (size_t)pr.n_rec) runs.clear();
    }
    pr.n_runs = (int)runs.size();
}

// K = 64: the same list cut into phases of 16 / 32 / 64 orders per voxel for launches from equilibrium (rows_grow_kernel); kept
// when at least a tenth of the record executions run below 64 orders (a 20-echo train: 15 of 20; a 1000-TR train: 30 of 1000)
static void grow_phases(RangeLists &pr, int K, const Knobs &kn) {
    const std::vector<Rec> &runs = pr.runs;
    std::vector<Rec> &grow = pr.grow;
    if (K == 64 && !runs.empty()) {
        double work[3];
        grow_split(runs, grow, pr.grow1, pr.grow2, work);
        if (kn.grow_min >= 2) pr.grow1 = 0;   // (EPGX_GROW_MIN=2, measurements: first phase at 2 orders per lane)
        if (kn.reach) grow_reach(grow, pr.grow1, pr.grow2, pr.grow_cap);   // (EPGX_REACH=0, measurements: 16 / 32 / 64)
        // the share of record executions that run below 64 orders: the first two ranges, and the last where it runs short
        const double all = work[0] + work[1] + work[2];
        const double early = all > 0 ? (work[0] + work[1] + (pr.grow_cap[2] < 64 ? work[2] : 0.0)) / all : 0.0;
        if (early < kn.grow_share) grow.clear();   // (EPGX_GROW_SHARE, measurements)
        if (tracing())
            for (size_t i = 0; i < grow.size(); ++i)
                fprintf(stderr, "[epgx] grow list %zu: leaf %u flags %06x x %u (orders <= %d)%s\n", i, grow[i].flags >> 24, grow[i].flags & 0xffffffu,
                        (uint32_t)grow[i].kmax >> 16, grow[i].kmax & 0xffff, (int)i == pr.grow1 || (int)i == pr.grow2 ? "   <- next phase" : "");
    }
    pr.n_grow = (int)grow.size();
}

// K = 128 .. 2048: where the populated orders of a launch from equilibrium outgrow 64, 128 .. 1536 (run_contig_grow_kernel; the
// two legs at 2048 orders).  `top` = the highest order that can hold anything, as in grow_split: every shift of a record adds one
static void cgrow_phases(RangeLists &pr, int K) {
    const std::vector<Rec> &recs = pr.recs;
    const std::vector<DRec> &drecs = pr.drecs;
    if (K >= 128 && drecs.empty() && pr.n_rec && !pr.use_lds) {
        int top = 0, phase = 0;
        double below = 0;
        static const int cap[6] = {63, 127, 255, 511, 1023, 1535};
        for (int &g : pr.cgrow) g = pr.n_rec;
        for (int i = 0; i < pr.n_rec; ++i) {
            const Rec &r = recs[(size_t)i];
            top += ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0);
            while (phase < 6 && top > cap[phase]) pr.cgrow[phase++] = i;
            if (phase < 5 && 64 << phase < K) below += 1;
        }
        for (int i = 0; i < pr.cgrow[3] && i < pr.n_rec; ++i) pr.cgrow_adc3 += (recs[(size_t)i].flags & F_ADC) ? 1 : 0;
        for (int q = 0; q < 6; ++q)
            if (cap[q] + 1 >= K) pr.cgrow[q] = pr.n_rec;     // (no phase at or above the capacity)
        for (int q = 1; q < 6; ++q) pr.cgrow[q] = std::max(pr.cgrow[q], pr.cgrow[q - 1]);
        pr.cgrow_share = below / pr.n_rec;
    }
}

// Derivative plans at 64 orders: runs of >= 4 records of one shape get a header (leaf byte LEAF_DRUN, shape code, count) and
// run on rotating order slots (drun_kernel, epgx_drun_kernels.hip.h); kept when the runs cover at least half of the
// records.  Two families of shapes:
//   * fused echoes  [S(+1)?  E.T.E + generated partials  S(+1)?  ADC]  (the host fused the tables: epgx_fuse_partial);
//   * repetitions FOLDED AT RUN TIME (DRUN_FOLD)  [S(+1)?  E_a . T . E_b  S(+1)?  ADC]  -- a rotation over one index space
//     between real relaxations over another (MRF / SSFP trains over a (T1, T2, B1) grid).  The fold happens HERE, for this
//     array only (every other kernel keeps walking the unfolded records of recs): E_a = the relaxation stage of the
//     rotation's own record, E_b = the record in front of it when that is nothing but a real relaxation and a shift by
//     one.  The rotation's partial is folded like the rotation (a . dT . b per coefficient); a relaxation's partial
//     enters through its table of logarithmic partials (PlanHost::logtabs) -- every relaxation partial of both stages
//     needs one, else the record stays unfolded.  Records the runs leave over are emitted UNFOLDED (their originals).
static void deriv_runs(const PlanHost &ph, RangeLists &pr, int K, const Knobs &kn, const std::vector<ELog> &elog) {
    const PlanHost *pl = &ph;
    const std::vector<Rec> &recs = pr.recs;
    const std::vector<DRec> &drecs = pr.drecs;
    std::vector<Rec> &druns = pr.druns;
    std::vector<DRec> &ddruns = pr.ddruns;
    std::vector<DRecB> &bdruns = pr.bdruns;
    if ((K == 64 || K == 32 || K == 16) && !drecs.empty() && pr.n_rec) {   // (16 / 32 orders: folded repetitions only, packed_dfold_kernel)
        const int nv = pl->n_vars;
        struct Item { Rec r; DRec d; DRecB b; int lo, hi; bool folded, logd, moved; };
        std::vector<Item> fl;
        fl.reserve((size_t)pr.n_rec);
        const uint32_t identity_off = (uint32_t)(pl->n_pool * 8), zeros_off = (uint32_t)((pl->n_pool + 8) * 8);
        // (plan_create fills log_of for derivative plans that may fold: EPGX_FOLD, EPGX_PLAN_NO_FOLD)
        const bool dfold = !pl->log_of.empty() && elog.size() == recs.size();
        for (int j = 0; j < pr.n_rec; ++j) {
            Item it;
            memset(&it, 0, sizeof(it));
            it.r = recs[(size_t)j];
            it.d = drecs[(size_t)j];
            it.lo = it.hi = j;
            const Rec &c = recs[(size_t)j];
            const uint32_t cf = c.flags & 0xffffffu;
            // (a spoiler in front of the rotation joins the fold at 16 / 32 orders -- where spoiled trains live: F_FOLD_SPOIL, the F
            // columns of E_b count as zero for the STATE; packed_dfold_kernel knows what that means for the derivative states)
            const uint32_t no_spoil = K == 64 ? (uint32_t)F_SPOIL : 0u;
            bool can = dfold && (cf & F_T) && (cf & F_ADC) &&
                       !(cf & (F_MAT | F_MAT0 | F_T0 | F_FOLD | F_D | F_GS | F_PD | F_PD_RESET | no_spoil | F_RESET | F_ADC_Z)) &&
                       !((cf & F_S) && c.shift != 1) && !((cf & F_E) && !(cf & F_ER));
            const bool has_a = (cf & F_E) != 0;
            if (can && has_a && elog[(size_t)j].blocked) can = false;
            // (three derivative states at 64 orders: the kernel carries one partial line of the rotation, epgx_drun_kernels.hip.h)
            if (can && K == 64 && nv == 3 && !EPGX_DF3_SPLIT && __builtin_popcount(drecs[(size_t)j].present & 7u) > 1) can = false;
            bool has_b = false;
            if (can && j > 0 && !fl.empty() && !fl.back().folded && fl.back().lo == j - 1) {
                const Rec &q = recs[(size_t)j - 1];
                const uint32_t rest = q.flags & 0xffffffu;
                has_b = (rest & F_E) && (rest & F_ER) && !(rest & ~(uint32_t)(F_E | F_ER | F_S | F_TRUNC)) &&
                        (!(rest & F_S) || q.shift == 1) && !elog[(size_t)j - 1].blocked &&
                        !((cf & F_S0) && (rest & F_S)) && (!(rest & F_TRUNC) || !(cf & F_S));
            }
            if (!can || (!has_a && !has_b)) {
                // a fused echo (EPGX_OP_T0 from the host's fusion) whose partials w.r.t. some variables come from its relaxations
                // alone: those variables take the logarithmic route (weights of E_a / E_b instead of a generated partial table)
                const int t_op = dfold && K == 64 && (cf & F_T0) ? elog[(size_t)j].t_op : -1;
                if (t_op >= 0 && !pl->t0_logd.empty()) {
                    DRec nd = it.d;
                    DRecB nb;
                    memset(&nb, 0, sizeof(nb));
                    bool any = false, ok = true;
                    for (int v = 0; v < EPGX_MAX_VARS; ++v) nb.off[v] = zeros_off;
                    for (int v = 0; v < nv && ok; ++v) {
                        if (!pl->t0_logd[(size_t)t_op * EPGX_MAX_VARS + v] || !(nd.present & (1u << v))) continue;
                        const int32_t ta = pl->t0_log[((size_t)t_op * EPGX_MAX_VARS + v) * 2], tb = pl->t0_log[((size_t)t_op * EPGX_MAX_VARS + v) * 2 + 1];
                        if ((ta >= 0 && pl->logtabs[(size_t)ta].off < 0) || (tb >= 0 && pl->logtabs[(size_t)tb].off < 0)) continue;   // not of the logarithmic form
                        nd.present &= ~(((1u | 16u | 256u | 65536u) << v));
                        nd.t_off[v] = nd.t_ix[v] = 0;
                        nd.e_off[v] = zeros_off;
                        nd.e_ix[v] = 0;
                        if (ta >= 0) {
                            const auto &lt = pl->logtabs[(size_t)ta];
                            nd.e_off[v] = (uint32_t)(lt.off * 8);
                            nd.e_ix[v] = lt.space < 0 ? 0u : (16u | ((uint32_t)lt.space << 24));
                            nb.logs |= ((lt.any & 1u) ? (1u << v) : 0u) | ((lt.any & 2u) ? (16u << v) : 0u);
                        }
                        if (tb >= 0) {
                            const auto &lt = pl->logtabs[(size_t)tb];
                            nb.off[v] = (uint32_t)(lt.off * 8);
                            nb.ix[v] = lt.space < 0 ? 0u : (16u | ((uint32_t)lt.space << 24));
                            nb.logs |= ((lt.any & 1u) ? (256u << v) : 0u) | ((lt.any & 2u) ? (4096u << v) : 0u);
                        }
                        any = true;
                    }
                    // (three derivative states: one partial line of the rotation at most)
                    if (any && !(nv == 3 && __builtin_popcount(nd.present & 7u) > 1)) {
                        it.d = nd;
                        it.b = nb;
                        it.logd = true;
                    }
                }
                fl.push_back(it);
                continue;
            }
            Rec f = c;
            f.flags = (cf & ~(uint32_t)(F_E | F_ER | F_SPOIL)) | F_FOLD | F_T0 | ((cf & F_SPOIL) ? (uint32_t)F_FOLD_SPOIL : 0u) | (LEAF_NONE << 24);
            f.e_off = has_a ? c.e_off : identity_off;
            f.e_ix = has_a ? c.e_ix : 0u;
            f.shift = (int32_t)identity_off;
            DRec fd;
            memset(&fd, 0, sizeof(fd));
            DRecB fb;
            memset(&fb, 0, sizeof(fb));
            const DRec &dc = drecs[(size_t)j];
            for (int v = 0; v < EPGX_MAX_VARS; ++v) {
                fd.e_off[v] = fb.off[v] = zeros_off;
                if (v < nv && (dc.present & (1u << v))) {   // the rotation's partial: folded like the rotation, constant term included
                    fd.t_off[v] = dc.t_off[v];
                    fd.t_ix[v] = dc.t_ix[v];
                    fd.present |= (dc.present & ((1u << v) | (256u << v) | (65536u << v))) | (16u << v);
                }
                const int32_t ta = has_a ? elog[(size_t)j].tab[v] : -1;
                if (ta >= 0) {
                    const auto &lt = pl->logtabs[(size_t)ta];
                    fd.e_off[v] = (uint32_t)(lt.off * 8);
                    fd.e_ix[v] = lt.space < 0 ? 0u : (16u | ((uint32_t)lt.space << 24));
                    fb.logs |= ((lt.any & 1u) ? (1u << v) : 0u) | ((lt.any & 2u) ? (16u << v) : 0u);
                }
            }
            if (has_b) {
                const Rec &q = recs[(size_t)j - 1];
                const uint32_t rest = q.flags & 0xffffffu;
                f.shift = (int32_t)q.e_off;
                if (q.e_ix & 0xffffffu) f.flags |= F_FOLD_BVOX | (((q.e_ix >> 24) & 3u) << 21);
                if (rest & F_S) {
                    f.flags |= F_S0 | (rest & F_TRUNC);
                    if (rest & F_TRUNC) f.kmax = q.kmax;
                }
                for (int v = 0; v < nv; ++v) {
                    const int32_t tb = elog[(size_t)j - 1].tab[v];
                    if (tb < 0) continue;
                    const auto &lt = pl->logtabs[(size_t)tb];
                    fb.off[v] = (uint32_t)(lt.off * 8);
                    fb.ix[v] = lt.space < 0 ? 0u : (16u | ((uint32_t)lt.space << 24));
                    fb.logs |= ((lt.any & 1u) ? (256u << v) : 0u) | ((lt.any & 2u) ? (4096u << v) : 0u);
                }
                fl.pop_back();
                it.lo = j - 1;
            }
            it.r = f;
            it.d = fd;
            it.b = fb;
            it.folded = true;
            fl.push_back(it);
        }
        auto shape_of = [&](const Item &x) {
            if (x.folded) return dfold_shape(x.r.flags & 0xffffffu, x.d.present, nv, K != 64);
            if (K != 64) return -1;
            const int code = drun_shape(x.r.flags & 0xffffffu, x.r.shift, x.d.present, nv);
            return (code >= 0 && x.logd) ? (code | (int)DRUN_LOGD) : code;
        };
        // A trailing S(+1) that closes the record in front of a train (the excitation pulse: [T S] [T0 S ADC] [S0 T0 S ADC] ...) is
        // the LEADING shift of the train's first record just as well -- same stages in the same order.  Moved, the first echo
        // has the shape of the others and joins their run (20 echoes: 20 records in the run instead of 16 + 4 flag-tested ones).
        if (K == 64)
            for (size_t j = 1; j + 1 < fl.size(); ++j) {
                Item &q = fl[j - 1], &c = fl[j];
                const Item &n = fl[j + 1];
                const uint32_t qf = q.r.flags & 0xffffffu, cf = c.r.flags & 0xffffffu, nf2 = n.r.flags & 0xffffffu;
                if (q.folded || c.folded != n.folded || q.lo != q.hi || c.lo != c.hi) continue;
                if (!(qf & F_S) || q.r.shift != 1 || (qf & (F_TRUNC | F_ADC | F_ADC_Z | F_FOLD))) continue;    // (nothing behind that shift)
                if ((cf & F_S0) || !(nf2 & F_S0) || (cf | F_S0) != nf2 || c.logd != n.logd || shape_of(n) < 0) continue;
                q.r.flags = ((qf & ~(uint32_t)F_S)) | (LEAF_NONE << 24);
                q.r.shift = 0;
                c.r.flags = (cf | F_S0) | (LEAF_NONE << 24);
                q.moved = c.moved = true;             // (emitted from the item itself from now on: see below)
            }
        const int nf = (int)fl.size();
        auto same_shape = [&](int x, int y) {
            const Item &X = fl[(size_t)x], &Y = fl[(size_t)y];
            const Rec &a = X.r, &b = Y.r;
            const DRec &da = X.d, &db = Y.d;
            if (X.folded != Y.folded || X.logd != Y.logd) return false;
            if (((a.flags ^ b.flags) & 0xffffffu) || a.kmax != b.kmax || a.t_ix != b.t_ix || a.e_ix != b.e_ix || da.present != db.present)
                return false;                                       // (the leaf byte of a record inside a run is never read)
            if (!X.folded && a.shift != b.shift) return false;      // (a folded record keeps E_b's table offset there)
            if ((X.folded || X.logd) && X.b.logs != Y.b.logs) return false;
            for (int v = 0; v < nv; ++v) {
                if (da.t_ix[v] != db.t_ix[v] || da.e_ix[v] != db.e_ix[v]) return false;
                if ((X.folded || X.logd) && X.b.ix[v] != Y.b.ix[v]) return false;
            }
            return true;
        };
        auto same_tables = [&](int x, int y) {
            const Item &X = fl[(size_t)x], &Y = fl[(size_t)y];
            const Rec &a = X.r, &b = Y.r;
            const DRec &da = X.d, &db = Y.d;
            if (a.t_off != b.t_off || a.e_off != b.e_off) return false;
            for (int v = 0; v < nv; ++v)
                if (da.t_off[v] != db.t_off[v] || da.e_off[v] != db.e_off[v] || X.b.off[v] != Y.b.off[v]) return false;
            return true;
        };
        // maximal runs of >= 4 same-shape records; the kernel handles ONE shape per launch: the one that covers most records
        struct Found { int first, n, code; };
        std::vector<Found> found;
        std::map<int, size_t> covered;
        for (int i = 0; i < nf;) {
            const int code = shape_of(fl[(size_t)i]);
            int n = 1;
            if (code >= 0)
                while (i + n < nf && n < 0x7fff && same_shape(i, i + n)) ++n;
            if (code >= 0 && n >= 4 && K != 64) {
                // 16 / 32 orders: a train that repeats ONE record (an echo train: same tables in every record) stays with the
                // straight-line leaves of packed_deriv_kernel, which beat the folded loop there (20-echo MSE, 1024 x 1024, three
                // variables: 6.4 / 2.9 ms at 32 / 16 orders against 6.9 / 3.2 folded); new tables per repetition (MRF) fold
                bool ident = true;
                for (int j = 1; j < n && ident; ++j) ident = same_tables(i, i + j);
                if (ident) {
                    i += n;
                    continue;
                }
            }
            if (code >= 0 && n >= 4) {
                // the loops of drun_kernel are unrolled four times (the slot bases come round after four records) and finish a
                // run of any length (up to three more records, then the registers are put back in order); the loop at
                // 16 / 32 orders takes a record at a time anyway
                const int take = n;
                found.push_back({i, take, code});
                covered[code] += (size_t)take * (size_t)(fl[(size_t)i].folded ? 2 : 1);   // (weights: original records covered)
            }
            i += n;
        }
        size_t in_runs = 0;
        for (const auto &c : covered)
            if (c.second > in_runs) {
                in_runs = c.second;
                pr.drun_code = c.first;
            }
        DRec dzero;
        memset(&dzero, 0, sizeof(dzero));
        DRecB bzero;
        memset(&bzero, 0, sizeof(bzero));
        size_t next = 0;
        for (int i = 0; i < nf;) {
            while (next < found.size() && (found[next].first < i || found[next].code != pr.drun_code)) ++next;
            if (next < found.size() && found[next].first == i) {
                const int n = found[next].n;
                bool ident = !fl[(size_t)i].folded;
                for (int j = 1; j < n && ident; ++j) ident = same_tables(i, i + j);
                Rec head;
                memset(&head, 0, sizeof(head));
                head.flags = (LEAF_DRUN << 24) | (uint32_t)pr.drun_code | (ident ? (uint32_t)DRUN_IDENT : 0u);
                head.kmax = n << 16;
                pr.drun_inside += n;
                pr.drun_headers += 1;
                pr.drun_ident += ident ? 1 : 0;
                druns.push_back(head);
                ddruns.push_back(dzero);
                bdruns.push_back(bzero);
                for (int j = 0; j < n; ++j) {
                    druns.push_back(fl[(size_t)i + j].r);
                    ddruns.push_back(fl[(size_t)i + j].d);
                    bdruns.push_back(fl[(size_t)i + j].b);
                }
                i += n;
                continue;
            }
            if (fl[(size_t)i].moved) {           // a record whose shift moved (above): the item's own record, unfolded
                druns.push_back(fl[(size_t)i].r);
                ddruns.push_back(drecs[(size_t)fl[(size_t)i].lo]);
                bdruns.push_back(bzero);
                ++i;
                continue;
            }
            for (int j = fl[(size_t)i].lo; j <= fl[(size_t)i].hi; ++j) {   // outside the runs: the records as they were packed
                druns.push_back(recs[(size_t)j]);
                ddruns.push_back(drecs[(size_t)j]);
                bdruns.push_back(bzero);
            }
            ++i;
        }
        if (in_runs * 2 < (size_t)pr.n_rec) {
            druns.clear();
            ddruns.clear();
            bdruns.clear();
        }
        // Fused echoes with logarithmic partials at 64 orders, from equilibrium: the run list cut where the populated orders
        // outgrow 16 and 32 (cf. grow_split) -- drun_kernel walks the first ranges with one and two orders per lane.  Cutting a
        // run ends its owed E_a update there and starts the next part afresh: the same sums in another association (rounding).
        if (K == 64 && !druns.empty() && (pr.drun_code & (int)DRUN_LOGD) && !(pr.drun_code & (int)DRUN_FOLD)) {
            auto shifts_of = [](const Rec &r) { return ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0); };
            static const int cap[3] = {15, 31, 1 << 30};
            std::vector<Rec> r2;
            std::vector<DRec> d2v;
            std::vector<DRecB> b2;
            int top = 0, phase = 0, n1 = -1, n2 = -1;
            double work[3] = {0, 0, 0};
            auto next_phase = [&]() {
                if (phase == 0) n1 = (int)r2.size();
                else n2 = (int)r2.size();
                ++phase;
            };
            for (size_t i = 0; i < druns.size();) {
                const Rec &r = druns[i];
                if ((r.flags >> 24) == LEAF_DRUN) {
                    const int count = (int)((uint32_t)r.kmax >> 16);
                    const int d = shifts_of(druns[i + 1]);
                    int done = 0;
                    while (done < count) {
                        int m = d > 0 ? (cap[phase] - top) / d : count - done;
                        m = std::min(m, count - done);
                        if (m <= 0) {
                            next_phase();
                            continue;
                        }
                        Rec h = r;
                        h.kmax = m << 16;
                        r2.push_back(h);
                        d2v.push_back(ddruns[i]);
                        b2.push_back(bdruns[i]);
                        for (int j = 0; j < m; ++j) {
                            r2.push_back(druns[i + 1 + (size_t)(done + j)]);
                            d2v.push_back(ddruns[i + 1 + (size_t)(done + j)]);
                            b2.push_back(bdruns[i + 1 + (size_t)(done + j)]);
                        }
                        work[phase] += m;
                        top += m * d;
                        done += m;
                    }
                    i += 1 + (size_t)count;
                    continue;
                }
                const int d = shifts_of(r);
                while (top + d > cap[phase]) next_phase();
                r2.push_back(r);
                d2v.push_back(ddruns[i]);
                b2.push_back(bdruns[i]);
                work[phase] += 1;
                top += d;
                ++i;
            }
            if (n1 < 0) n1 = (int)r2.size();
            if (n2 < 0) n2 = (int)r2.size();
            const double all = work[0] + work[1] + work[2];
            if (all > 0 && (work[0] + work[1]) / all >= 0.1) {
                druns.swap(r2);
                ddruns.swap(d2v);
                bdruns.swap(b2);
                pr.dgrow1 = std::min(n1, n2);
                pr.dgrow2 = n2;
                if (kn.grow_min >= 2) pr.dgrow1 = 0;
            }
        }
    }
    pr.n_druns = (int)druns.size();
}

RangeLists build_range(const PlanHost &ph, int begin, int end, int K, const Knobs &kn) {
    RangeLists pr;
    pr.begin = begin;
    pr.end = end;
    pr.K = K;
    std::vector<ELog> elog;
    pack_records(ph, begin, end, K, kn, pr.recs, pr.drecs, pr.use_lds, pr.has_adc, elog);
    range_facts(pr);
    fold_runs(pr, K);
    grow_phases(pr, K, kn);
    cgrow_phases(pr, K);
    if (!ph.second) deriv_runs(ph, pr, K, kn, elog);   // (second-order passes walk the plain record list: hess_kernel)
    return pr;
}

Rec with_leaf(Rec r) {
    r.flags &= 0xffffffu;
    r.flags |= record_leaf<false>(r.flags, r.shift) << 24;
    return r;
}

int tiled_schedule(const PlanHost &ph, int Kbuf, int top0, int M, int H, const Knobs &kn, TiledSchedule &ts) {
    std::vector<Rec> packed;
    std::vector<DRec> drecs;
    std::vector<ELog> elog;
    bool use_lds = false;
    const int n_ops = (int)ph.ops.size();
    pack_records(ph, 0, n_ops, 1 << 30, kn, packed, drecs, use_lds, ts.has_adc, elog);
    const int W = 64 * M - 2 * H;
    struct Item { Rec r; int big; DRec d; };    // big: 0, or the shift of a step of its own; d: the record's partials (derivative plans)
    std::vector<Item> items;
    const uint32_t probe = F_ADC | F_ADC_Z;
    const bool deriv = !drecs.empty();
    DRec none;                          // a record made here (unit shift, probe) has no partials
    memset(&none, 0, sizeof(none));
    for (size_t ri = 0; ri < packed.size(); ++ri) {
        const Rec &r = packed[ri];
        const DRec &d = deriv ? drecs[ri] : none;
        const int n = ((r.flags & F_S) && !(r.flags & F_FOLD)) ? r.shift : 1;
        if (!(r.flags & F_S) || std::abs(n) <= 1) {
            items.push_back({r, 0, d});
            continue;
        }
        Rec head = r;
        head.flags &= ~(F_TRUNC | probe);
        if (std::abs(n) > H) {
            head.flags &= ~F_S;
            head.shift = 0;
            if (head.flags & 0xffffffu) items.push_back({with_leaf(head), 0, d});
            Rec step;
            memset(&step, 0, sizeof(step));
            step.flags = r.flags & F_TRUNC;
            step.kmax = r.kmax;
            items.push_back({step, n, none});
        } else {
            head.shift = n > 0 ? 1 : -1;
            items.push_back({with_leaf(head), 0, d});
            for (int j = 1; j < std::abs(n); ++j) {
                Rec one;
                memset(&one, 0, sizeof(one));
                one.flags = F_S | (j + 1 == std::abs(n) ? (r.flags & F_TRUNC) : 0u);
                one.shift = n > 0 ? 1 : -1;
                one.kmax = r.kmax;
                items.push_back({with_leaf(one), 0, none});
            }
            if (!(r.flags & probe)) continue;
            Rec &last = items.back().r;
            last.flags |= r.flags & probe;
            last.slot = r.slot;
            last = with_leaf(last);
            continue;
        }
        if (r.flags & probe) {
            Rec adc;
            memset(&adc, 0, sizeof(adc));
            adc.flags = r.flags & probe;
            adc.slot = r.slot;
            items.push_back({with_leaf(adc), 0, none});
        }
    }
    ts.recs.clear();
    ts.drecs.clear();
    ts.steps.clear();
    ts.peak = top0;
    ts.n_shift = 0;
    ts.tile_launches = 0;
    int top = top0, units = 0;
    int cov[2] = {top0 / W + 1, 0};   // tiles the latest step wrote into buffer 0 / 1 (the start state is in buffer 0)
    TiledStep cur;
    auto close = [&](TiledStep st) {
        const int buf = (int)(ts.steps.size() + 1) & 1;      // the buffer this step writes
        st.top = top;
        st.tiles = std::max(top / W + 1, cov[buf]);
        cov[buf] = st.tiles;
        ts.tile_launches += st.tiles;
        ts.steps.push_back(st);
    };
    for (const Item &it : items) {
        const Rec &r = it.r;
        if (it.big) {
            if (cur.rec1 > cur.rec0) close(cur);
            TiledStep st;
            st.shift = it.big;
            top += std::abs(it.big);
            if (r.flags & F_TRUNC) {
                st.kmax = r.kmax;
                top = std::min(top, r.kmax);
            }
            ts.peak = std::max(ts.peak, top);
            close(st);
            ++ts.n_shift;
            cur = TiledStep();
            cur.rec0 = cur.rec1 = (int)ts.recs.size();
            units = 0;
            continue;
        }
        const int u = ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0);
        if (units + u > H && cur.rec1 > cur.rec0) {
            close(cur);
            cur = TiledStep();
            cur.rec0 = cur.rec1 = (int)ts.recs.size();
            units = 0;
        }
        units += u;
        if (r.flags & (F_RESET | F_PD_RESET)) top = 0;
        if (r.flags & F_S0) top += 1;
        if (r.flags & F_S) top += 1;
        if (r.flags & F_TRUNC) top = std::min(top, r.kmax);
        ts.peak = std::max(ts.peak, top);
        ts.recs.push_back(r);
        if (deriv) ts.drecs.push_back(it.d);
        cur.rec1 = (int)ts.recs.size();
    }
    if (cur.rec1 > cur.rec0) close(cur);
    if (ts.peak >= Kbuf)
        return fail(EPGX_ERR_INVALID, "epgx_run_tiled: the plan populates orders up to %d, Kbuf=%d", ts.peak, Kbuf);
    return EPGX_OK;
}

int choose_kernel(const PlanHost &ph, const RangeLists &lists, int op_begin, int op_end, int K, bool has_in, bool has_out, const Knobs &kn,
                  Choice *c) {
    const PlanHost *pl = &ph;
    const RangeLists *pr = &lists;
    const bool packed16 = K == 16 || K == 32, wide = K == 2048 && !has_in && !has_out;
    bool has_general = false, has_nd = false;   // general 3x3 matrices; diffusion / gather shifts
    for (int i = op_begin; i < op_end; ++i) {
        const int oc = pl->ops[i].opcode;
        has_general = has_general || oc == EPGX_OP_MAT || oc == EPGX_OP_MAT0;
        has_nd = has_nd || oc == EPGX_OP_D || oc == EPGX_OP_GS;
    }
    c->packed16 = packed16;
    c->wide = wide;
    c->has_nd = has_nd;
    c->lds_mode = pr->use_lds ? ((pr->has_gs && K < 1024) ? 3 : 2) : 0;      // (gather shifts at 1024 orders stage Z behind F: gather_shift)
    // (the rows kernels and packed_deriv_kernel address the pool through a buffer resource of 2 GiB)
    const bool pool_in_reach = (pl->n_pool + 64 + pl->n_log) * (int64_t)sizeof(double) <= 0x7fffffff;
    if (packed16 && !pool_in_reach)
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 need a coefficient pool below 2 GiB (use K = 64)");
    if (wide && (pr->use_lds || pl->n_vars > 0))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 2048 handles rotations, relaxation, shifts by +-1 and probes only (no derivative states)");
    if (packed16 && pr->big_shift) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 handle shifts by +-1 (and, at K = 16, gather shifts) only");
    if (packed16 && pl->n_vars > 0 && has_in) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 derivative plans start from equilibrium");
    if (packed16 && pl->n_vars > 0 && pr->use_lds) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 derivative plans handle shifts by +-1 only");
    const int nsp = pl->n_spaces <= 2 ? pl->n_spaces : 4, V = pl->n_vars;
    const bool plain_ops = !has_general && !has_nd && !pr->use_lds;   // rotations, relaxation, shifts by +-1, probes, SPOILER / RESET / PD
    if (V > 0 && pl->second) {
        // one-pair second-order pass: S, S_a, (S_b,) H_ab in registers -- the capacities at which a launch carries three derivative states
        if (has_in || has_out) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: second-order plans run state-resident from equilibrium (in = out = NULL)");
        if (K != 64 && K != 128 && K != 256 && K != 512)
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: second-order plans support K = 64, 128, 256, 512, got %d", K);
        const bool diag = V == 2;
        c->family = FAM_HESS;
        c->why = diag ? "second-order pass for a diagonal pair: S, S_a, H_aa, one wavefront per voxel"
                      : "second-order pass for one variable pair: S, S_a, S_b, H_ab, one wavefront per voxel";
        // (hess_kernel<8, 1, false> alone needs scratch (32 bytes per lane): such plans run the two-space instantiation, whose second
        // space no record refers to)
        snprintf(c->name, sizeof(c->name), "hess_kernel<%d, %d, %s>", K / 64, (K == 512 && !diag && nsp == 1) ? 2 : nsp, diag ? "true" : "false");
        return EPGX_OK;
    }
    if (V > 0) {
        if (has_out) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: derivative plans run state-resident (out = NULL)");
        if (K > 1024) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: derivative plans support K <= 1024, got %d", K);
        if (K == 1024 && V > 1)
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: at K = 1024 a launch carries ONE derivative state (plan has %d variables: one plan per variable)", V);
        // deriv_kernel at K >= 128: consecutive orders per lane unless the range shifts by |n| >= 2, gathers or diffuses (EPGX_CONTIG=0: never)
        // (not with three derivative states at 256 / 512 orders: 282 VGPRs / 585 spill instructions there against 249 / 9 lane-strided,
        // measured 111 against 75 ms and 313 against 174 ms)
        c->contig = kn.contig && K >= 128 && !pr->use_lds && !has_nd && !(V == 3 && (K == 256 || K == 512));
        const bool resident64 = K == 64 && !has_in && plain_ops && pool_in_reach;
        if (packed16 && kn.drun && !pr->druns.empty() && !pr->bdruns.empty() && !has_in && !pr->use_lds && pool_in_reach) {
            c->family = FAM_PACKED_DFOLD;
            c->why = "16 / 32 orders, mostly runs of repetitions folded at run time";
            snprintf(c->name, sizeof(c->name), "packed_dfold_kernel<%d, %d>", V, K);
        } else if (kn.drun && !pr->druns.empty() && resident64) {
            c->family = FAM_DRUN;
            c->split3 = V == 3 && (pr->drun_code & (int)DRUN_FOLD) && EPGX_DF3_SPLIT;
            c->why = (pr->drun_code & (int)DRUN_FOLD)   ? "64 orders, mostly runs of repetitions folded at run time: rotating order slots"
                     : (pr->drun_code & (int)DRUN_LOGD) ? "64 orders, mostly runs of fused echoes with logarithmic relaxation partials: rotating order slots"
                                                        : "64 orders, mostly runs of fused echoes: rotating order slots";
            // (runs with logarithmic partials exist for four index spaces only; the others for one and four: epgx_launch_drun)
            const int knsp = ((pr->drun_code & 384) || pl->n_spaces > 1) ? 4 : 1;
            if (c->split3) snprintf(c->name, sizeof(c->name), "drun_kernel<%d, 1, %d, 2> + drun_kernel<%d, 2, %d, 0>", knsp, pr->drun_code, knsp, pr->drun_code);
            else snprintf(c->name, sizeof(c->name), "drun_kernel<%d, %d, %d, 0>", knsp, V, pr->drun_code);
        } else if (kn.rows_deriv && (V == 1 || (V == 2 && kn.rows_deriv2)) && resident64) {
            c->family = FAM_ROWS_DERIV;
            c->why = "64 orders from equilibrium, one or two derivative states: four voxels per wavefront";
            snprintf(c->name, sizeof(c->name), "rows_deriv_kernel<%d, 4, %d>", nsp, V);
        } else if (packed16) {
            c->family = FAM_PACKED_DERIV;
            c->why = "16 / 32 orders with derivative states";
            snprintf(c->name, sizeof(c->name), "packed_deriv_kernel<%d, %d, %d>", nsp, V, K);
        } else {
            c->family = FAM_DERIV;
            c->why = "derivative states, one wavefront per voxel";
            snprintf(c->name, sizeof(c->name), "deriv_kernel<%d, %d, %d%s>", K / 64, nsp, V, c->contig ? ", true" : "");
        }
        return EPGX_OK;
    }
    // K = 256 .. 1024 (EPGX_CGROW=2: from 128) from equilibrium with a good share of the records while the state matrix is short: phases of 1, 2, 4 .. orders per lane
    // (at K = 128 the four-voxels-per-wavefront kernel with 8 orders per lane is the alternative: the phases win while the train mostly
    // runs below 64 orders -- 40 echoes 1.08 against 1.17 ms, 63 echoes 1.82 against 1.78; EPGX_CGROW=2: always)
    const bool cgrow = kn.contig && kn.cgrow && K >= 128 && K <= 1024 && !has_in && !has_out && !pr->use_lds && !has_nd &&
                       pr->cgrow_share >= ((K == 128 && kn.cgrow < 2) ? std::max(kn.grow_share, 0.6) : kn.grow_share);
    if (cgrow) {
        c->family = FAM_RUN_CONTIG_GROW;
        c->why = "from equilibrium, a good share of the records while the state matrix is short: K / 64 consecutive orders per lane reached in phases of 1, 2, 4 ..";
        snprintf(c->name, sizeof(c->name), "run_contig_grow_kernel<%d, %d>", K / 64, nsp);
        return EPGX_OK;
    }
    // four voxels per wavefront, K / 16 orders per lane: always at 16 / 32 orders; at 64 / 128 state-resident launches of plain operators
    const bool rows = packed16 || (kn.rows && (K == 64 || K == 128) && !has_in && !has_out && plain_ops && pool_in_reach);
    if (rows) {
        c->runs = kn.runs && !pr->runs.empty() && K <= 64;
        if (c->runs && K == 64 && kn.grow && !pr->grow.empty()) {
            c->family = FAM_ROWS_GROW;
            c->why = "64 orders from equilibrium, a good share of the records while the state matrix is short: phases of 1 / 2 / 4 orders per lane";
            snprintf(c->name, sizeof(c->name), "rows_grow_kernel<%d>", nsp);
        } else {
            c->family = FAM_ROWS;
            c->why = "state-resident, four voxels per wavefront";
            snprintf(c->name, sizeof(c->name), "rows_kernel<%d, %d, %s>", nsp, K / 16, (c->runs && K <= 64) ? "true" : "false");
        }
        return EPGX_OK;
    }
    // one wavefront per voxel (four at K = 2048).  Launches without a state output at
    // K >= 128 are free to choose the order layout: a lane then holds K / 64 consecutive orders and a shift by one costs 8 DPP
    // moves instead of 16 K / 64 moves and selects (epgx_split.hip; the same bits).  Not with shifts by |n| >= 2, gather shifts or diffusion.
    const bool free_layout = !has_out && !pr->use_lds && !has_nd;
    if (K == 2048) {
        c->family = FAM_RUN_SPLIT;
        c->split_grow = kn.split_grow && pr->cgrow_share >= kn.grow_share && pr->cgrow[3] > 0;
        c->why = c->split_grow ? "2048 orders from equilibrium: one wavefront per voxel while at most 512 orders hold anything, then up to four (the state crosses HBM once)"
                               : "2048 orders from equilibrium: four wavefronts per voxel";
        if (c->split_grow) snprintf(c->name, sizeof(c->name), "run_kernel<8, %d, false> + run_split_kernel<4, %d, true>", nsp, nsp);
        else snprintf(c->name, sizeof(c->name), "run_split_kernel<4, %d, false>", nsp);
    } else if (kn.contig && K >= 128 && K <= 1024 && free_layout) {
        c->family = FAM_RUN_CONTIG;
        c->why = "no state output: K / 64 consecutive orders per lane";
        snprintf(c->name, sizeof(c->name), "run_contig_kernel<%d, %d, %s>", K / 64, nsp, has_in ? "true" : "false");
    } else {
        c->family = FAM_RUN;
        c->why = "one wavefront per voxel, state through HBM or operators the other kernels do not take";
        snprintf(c->name, sizeof(c->name), "run_kernel<%d, %d, %s>", K / 64, nsp, has_in ? "true" : "false");
    }
    return EPGX_OK;
}

}  // namespace epgx

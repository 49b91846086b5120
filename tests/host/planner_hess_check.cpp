// planner_hess_check.cpp -- the launch planner's part in one-pair second-order passes (EPGX_DERIV_SECOND), on a machine without a
// GPU: pack_records carries the operators' cross-term bits into DRec.pad0 per stage, choose_kernel names hess_kernel<M, NSP, DIAG>
// for the capacities 64 .. 512 and refuses the others.  Same conventions as planner_check.cpp: one line per check, non-zero exit at
// the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_planner.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) exit(1);
}
#define CHECK(cond) check((cond), #cond)

static const int NOTRUNC = 1 << 20;

struct Seq {
    PlanHost ph;
    int n_adc = 0;
    void push(int opcode, int ia, int ib, int64_t off, int ncoef, int space) {
        epgx_op op;
        memset(&op, 0, sizeof(op));
        op.opcode = opcode; op.space = space; op.ia = ia; op.ib = ib; op.coef_off = off; op.ncoef = ncoef;
        ph.ops.push_back(op);
        ph.zero_pattern.push_back(0);
        ph.gather_tables.emplace_back();
        epgx_dop d;
        memset(&d, 0, sizeof(d));
        for (int v = 0; v < EPGX_MAX_VARS; ++v) { d.space[v] = -1; d.coef_off[v] = -1; }
        ph.dops.push_back(d);
        ph.dpattern.push_back(0);
    }
    // partial tables of the operator just pushed: off[v] < 0 = none; `cross`: EPGX_HESS_CROSS_* bits
    void partials(int64_t o0, int64_t o1, int64_t o2, int cross) {
        epgx_dop &d = ph.dops.back();
        d.coef_off[0] = o0; d.coef_off[1] = o1; d.coef_off[2] = o2;
        d.reserved = cross;
    }
    int n() const { return (int)ph.ops.size(); }
};

static Knobs defaults() {
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1};
    return k;
}

// T | (S E T S E ADC) x n for the pair (a, b): a = the relaxation's variable, b = the rotation's; second-order tables on both
static Seq train(int n, int n_vars, int n_spaces) {
    Seq s;
    s.ph.n_spaces = n_spaces;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = false;
    s.ph.second = true;
    s.ph.n_vars = n_vars;
    const bool diag = n_vars == 2;
    s.push(EPGX_OP_T, 0, 0, 0, 8, -1);
    for (int i = 0; i < n; ++i) {
        for (int half = 0; half < 2; ++half) {
            s.push(EPGX_OP_S, 1, NOTRUNC, 0, 0, -1);
            s.push(EPGX_OP_E, 0, 0, 64, 4, n_spaces ? 0 : -1);
            // the relaxation: dE/da (slot 0), its second-order table in the H slot; cross term a from the first pulse on (S_b alive)
            if (diag) s.partials(100, 200, -1, i > 0 || half > 0 ? EPGX_HESS_CROSS_A : 0);
            else s.partials(100, -1, 200, i > 0 || half > 0 ? EPGX_HESS_CROSS_A : 0);
            if (half == 0) {
                s.push(EPGX_OP_T, 0, 0, 16, 8, -1);
                if (diag) s.partials(300, 400, -1, EPGX_HESS_CROSS_A);        // the same variable: the doubled cross term
                else s.partials(-1, 300, -1, EPGX_HESS_CROSS_B);              // dT/db (slot 1) acting on S_a, no second-order table
            }
        }
        s.push(EPGX_OP_ADC, s.n_adc, 0, 0, 0, -1);
        s.n_adc += 1 + n_vars;
    }
    return s;
}

int main() {
    const Knobs kn = defaults();
    for (int n_vars = 2; n_vars <= 3; ++n_vars) {
        const bool diag = n_vars == 2;
        Seq s = train(3, n_vars, 1);
        RangeLists rl = build_range(s.ph, 0, s.n(), 64, kn);
        CHECK(rl.druns.empty() && rl.n_druns == 0);          // second-order passes walk the plain record list
        CHECK(rl.recs.size() == rl.drecs.size());
        int t_xa = 0, t_xb = 0, e_xa = 0, e_xb = 0, e_none = 0;
        for (size_t j = 0; j < rl.recs.size(); ++j) {
            const Rec &r = rl.recs[j];
            const DRec &d = rl.drecs[j];
            if (r.flags & F_T) {
                t_xa += (d.pad0 & HESS_T_XA) ? 1 : 0;
                t_xb += (d.pad0 & HESS_T_XB) ? 1 : 0;
            } else CHECK(!(d.pad0 & (HESS_T_XA | HESS_T_XB)));
            if (r.flags & F_E) {
                e_xa += (d.pad0 & HESS_E_XA) ? 1 : 0;
                e_xb += (d.pad0 & HESS_E_XB) ? 1 : 0;
                e_none += (d.pad0 & (HESS_E_XA | HESS_E_XB)) ? 0 : 1;
                CHECK((d.present & (16u << (n_vars - 1))) != 0);   // the relaxation's second-order table sits in the H slot
            } else CHECK(!(d.pad0 & (HESS_E_XA | HESS_E_XB)));
        }
        CHECK(e_xa == 5 && e_none == 1 && e_xb == 0);          // six relaxations, the first before any pulse declared b
        CHECK(diag ? (t_xa == 3 && t_xb == 0) : (t_xa == 0 && t_xb == 3));
        for (int K : {64, 128, 256, 512}) {
            for (int nsp = 0; nsp <= 3; ++nsp) {
                Seq q = train(3, n_vars, nsp);
                RangeLists lists = build_range(q.ph, 0, q.n(), K, kn);
                Choice c;
                CHECK(choose_kernel(q.ph, lists, 0, q.n(), K, false, false, kn, &c) == EPGX_OK);
                char want[64];
                int knsp = nsp <= 2 ? nsp : 4;
                if (K == 512 && !diag && knsp == 1) knsp = 2;       // the one instantiation that would need scratch
                snprintf(want, sizeof(want), "hess_kernel<%d, %d, %s>", K / 64, knsp, diag ? "true" : "false");
                check(c.family == FAM_HESS && std::string(c.name) == want, want);
            }
        }
        Choice c;
        RangeLists big = build_range(s.ph, 0, s.n(), 1024, kn);
        CHECK(choose_kernel(s.ph, big, 0, s.n(), 1024, false, false, kn, &c) == EPGX_ERR_UNSUPPORTED);
        RangeLists small = build_range(s.ph, 0, s.n(), 32, kn);
        CHECK(choose_kernel(s.ph, small, 0, s.n(), 32, false, false, kn, &c) == EPGX_ERR_UNSUPPORTED);
        CHECK(choose_kernel(s.ph, rl, 0, s.n(), 64, true, false, kn, &c) == EPGX_ERR_UNSUPPORTED);     // from a state input
        CHECK(choose_kernel(s.ph, rl, 0, s.n(), 64, false, true, kn, &c) == EPGX_ERR_UNSUPPORTED);     // with a state output
        // the same plan without the flag is a first-order plan: no cross bits reach the records, the usual kernels are named
        s.ph.second = false;
        RangeLists first = build_range(s.ph, 0, s.n(), 128, kn);
        for (const DRec &d : first.drecs) CHECK(d.pad0 == 0);
        CHECK(choose_kernel(s.ph, first, 0, s.n(), 128, false, false, kn, &c) == EPGX_OK);
        CHECK(c.family != FAM_HESS && std::string(c.name).find("hess_kernel") == std::string::npos);
    }
    printf("planner_hess_check: all checks passed\n");
    return 0;
}

// lanes_check.cpp -- lanes_plan (epgpy_amd/csrc/epgx_planner.cpp): which cut record lists the one-voxel-per-lane variant of the
// growing launch takes, and the live count L it is launched with, on a machine without a GPU.
//
// Plans are built as in planner_check.cpp (made-up pool offsets: planning never reads a coefficient) and run through the C++
// that ships; L is checked against the rule restated in its simplest form: between two shifts a launch holds
// 1 + min(shifts so far, shifts left before the last probe) live orders.  One line per check; exits non-zero at the first failure.
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
    void push(int opcode, int ia, int ib, int64_t off, int ncoef, int space, int zero) {
        epgx_op op;
        memset(&op, 0, sizeof(op));
        op.opcode = opcode;
        op.space = space;
        op.ia = ia;
        op.ib = ib;
        op.coef_off = off;
        op.ncoef = ncoef;
        ph.ops.push_back(op);
        ph.zero_pattern.push_back((uint8_t)zero);
        ph.gather_tables.emplace_back();
    }
    void T(int64_t off) { push(EPGX_OP_T, 0, 0, off, 8, 0, 0); }
    void E(int64_t off, bool real) { push(EPGX_OP_E, 0, 0, off, 4, 0, real ? 2 : 0); }
    void S(int n, int kmax = NOTRUNC) { push(EPGX_OP_S, n, kmax, 0, 0, -1, 0); }
    void ADC(bool z0 = false) { push(EPGX_OP_ADC, n_adc++, z0 ? 1 : 0, 0, 0, -1, 0); }
    void SPOIL() { push(EPGX_OP_SPOIL, 0, 0, 0, 0, -1, 0); }
    void RESET() { push(EPGX_OP_RESET, 0, 0, 0, 0, -1, 0); }
    int n() const { return (int)ph.ops.size(); }
};

static Seq new_seq(bool fold) {
    Seq s;
    s.ph.n_spaces = 1;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = fold;
    return s;
}

static Knobs knobs(int lanes) {   // the values knobs() takes with an empty environment, and EPGX_LANES
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, lanes};
    return k;
}

// T | (E S T E S ADC?) x n: `probe(i)` says whether echo i (0 ..) is probed; shift: the sign of the echoes from `back` on
template <class P>
static Seq echo_train(int n, bool fold, bool real, P probe, int back = 1 << 30, int kmax = NOTRUNC) {
    Seq s = new_seq(fold);
    s.T(0);
    for (int i = 0; i < n; ++i) {
        s.E(64, real);
        s.S(i >= back ? -1 : 1, kmax);
        s.T(16);
        s.E(64, real);
        s.S(i >= back ? -1 : 1, kmax);
        if (probe(i)) s.ADC();
    }
    return s;
}
static bool every(int) { return true; }

// the rule, on the shifts of the operator stream itself
static int live_count(const Seq &s) {
    int last = -1;
    for (int i = 0; i < s.n(); ++i)
        if (s.ph.ops[(size_t)i].opcode == EPGX_OP_ADC) last = i;
    int total = 0;
    for (int i = 0; i <= last; ++i) total += s.ph.ops[(size_t)i].opcode == EPGX_OP_S ? 1 : 0;
    int top = 0, need = 1;
    for (int i = 0; i <= last; ++i)
        if (s.ph.ops[(size_t)i].opcode == EPGX_OP_S) {
            ++top;
            const int live = 1 + (top < total - top ? top : total - top);
            need = live > need ? live : need;
        }
    return need;
}

static LanesPlan plan_of(const Seq &s, int lanes = 1, bool has_in = false, bool has_out = false) {
    const Knobs kn = knobs(lanes);
    RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
    return lanes_plan(l.grow, has_in, has_out, kn);
}

static void expect(const LanesPlan &lp, bool eligible, const char *why, const char *what) {
    printf("   %-44s -> %s%s\n", what, lp.eligible ? "lanes, L = " : "rows: ", lp.eligible ? std::to_string(lp.L).c_str() : lp.why);
    check(lp.eligible == eligible && std::string(lp.why) == why, what);
}

int main() {
    printf("== L for 1 .. 31 echoes\n");
    for (int n = 1; n <= 31; ++n) {
        for (int fold = 0; fold < 2; ++fold) {
            Seq s = echo_train(n, fold != 0, true, every);
            const Knobs kn = knobs(1);
            RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
            if (l.grow.empty()) continue;   // (short trains keep rows_kernel: no growing list, nothing to select)
            const LanesPlan lp = lanes_plan(l.grow, false, false, kn);
            printf("   %2d echoes%s: L = %d, %d shifts before the last probe, %s\n", n, fold ? " (folded)" : "", lp.L, lp.rem0,
                   lp.eligible ? "lanes" : lp.why);
            CHECK(lp.L == n + 1 && lp.L == live_count(s));
            CHECK(lp.rem0 == 2 * n);
            CHECK(lp.eligible == (n + 1 <= LANES_MAX_ORDERS));
            if (!lp.eligible) CHECK(std::string(lp.why) == "more than 24 live orders");
        }
    }
    {
        Seq s = echo_train(20, true, true, every);
        CHECK(plan_of(s).L == 21);   // the benchmark's train
        Seq t = echo_train(23, true, true, every);
        CHECK(plan_of(t).L == 24 && plan_of(t).eligible);   // the largest supported
    }

    printf("== probed / unprobed mixes\n");
    {
        // 9 probed echoes and 3 unprobed ones behind them: the window only counts the shifts up to the last probe
        Seq s = echo_train(12, true, true, [](int i) { return i < 9; });
        const LanesPlan lp = plan_of(s);
        printf("   9 probed + 3 unprobed echoes: L = %d, %d shifts before the last probe, %s\n", lp.L, lp.rem0, lp.eligible ? "lanes" : lp.why);
        CHECK(lp.eligible && lp.L == 10 && lp.rem0 == 18 && lp.L == live_count(s));
        // probes on every other echo (the last echo is probed: 20 echoes, probes behind echoes 2, 4 .. 20)
        // (this operator stream does not fold into a growing list -- its unprobed echoes pack into two records each -- so the cut
        // list is written down: T, then ten times an unprobed and a probed fused echo, one execution per record)
        std::vector<Rec> list;
        auto rec = [&](uint32_t flags, int rep, int slot) {
            Rec r;
            memset(&r, 0, sizeof(r));
            r.flags = flags | (LEAF_NONE << 24);
            r.shift = (flags & F_S) ? 1 : 0;
            r.kmax = rep << 16;
            r.slot = slot;
            list.push_back(r);
        };
        rec(F_T, 1, 0);
        for (int i = 0; i < 10; ++i) {
            rec(F_S0 | F_T | F_T0 | F_S, 1, 0);
            rec(F_S0 | F_T | F_T0 | F_S | F_ADC, 1, i);
        }
        const LanesPlan lo = lanes_plan(list, false, false, knobs(1));
        CHECK(lo.eligible && lo.L == 21 && lo.rem0 == 40);
        list.back().flags &= ~(uint32_t)F_ADC;   // the last echo unprobed as well: the 18 echoes up to the probe before it count
        const LanesPlan lm = lanes_plan(list, false, false, knobs(1));
        CHECK(lm.eligible && lm.L == 19 && lm.rem0 == 36);
        // a single probe behind 12 echoes: one record with a repeat count, one with the probe
        list.clear();
        rec(F_T, 1, 0);
        rec(F_S0 | F_T | F_T0 | F_S, 11, 0);
        rec(F_S0 | F_T | F_T0 | F_S | F_ADC, 1, 0);
        const LanesPlan lq = lanes_plan(list, false, false, knobs(1));
        CHECK(lq.eligible && lq.L == 13 && lq.rem0 == 24);
        // unfolded relaxations with precession: pairs of records
        Seq u = echo_train(20, false, false, every);
        const LanesPlan lu = plan_of(u);
        CHECK(lu.eligible && lu.L == 21 && lu.rem0 == 40);
    }

    printf("== accept and refuse\n");
    {
        Seq s = echo_train(20, true, true, every);
        expect(plan_of(s, 1), true, "", "20 echoes");
        expect(plan_of(s, 2), true, "", "20 echoes, EPGX_LANES=2");
        expect(plan_of(s, 0), false, "EPGX_LANES=0", "20 echoes, EPGX_LANES=0");
        expect(plan_of(s, 1, true, false), false, "a state input or output", "20 echoes from a state");
        expect(plan_of(s, 1, false, true), false, "a state input or output", "20 echoes with a state output");
        expect(lanes_plan(std::vector<Rec>(), false, false, knobs(1)), false, "no growing record list", "no list");
        Seq back = echo_train(20, true, true, every, 10);
        expect(plan_of(back), false, "S(-1)", "echoes 11 .. 20 shift back");
        {   // (a plan with max_nstate = 10 runs at 16 orders and has no growing list: the flag is set on the 20-echo list by hand)
            const Knobs kn = knobs(1);
            RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
            l.grow.back().flags |= F_TRUNC;
            l.grow.back().kmax = (l.grow.back().kmax & ~0xffff) | 10;
            expect(lanes_plan(l.grow, false, false, kn), false, "a truncation below the capacity", "a truncation at order 10");
        }
        Seq spoiled = echo_train(9, true, true, every);
        spoiled.SPOIL();
        spoiled.T(0);
        for (int i = 0; i < 11; ++i) {
            spoiled.E(64, true); spoiled.S(1); spoiled.T(16); spoiled.E(64, true); spoiled.S(1); spoiled.ADC();
        }
        expect(plan_of(spoiled), false, "a spoiler", "a spoiler between two trains");
        Seq reset = echo_train(9, true, true, every);
        reset.RESET();
        reset.T(0);
        for (int i = 0; i < 11; ++i) {
            reset.E(64, true); reset.S(1); reset.T(16); reset.E(64, true); reset.S(1); reset.ADC();
        }
        expect(plan_of(reset), false, "a reset", "a reset between two trains");
        Seq z0 = echo_train(20, true, true, every);
        z0.ADC(true);
        expect(plan_of(z0), false, "a Z0 probe", "a Z0 probe behind the train");
        Seq none = echo_train(20, true, true, [](int) { return false; });
        {
            const Knobs kn = knobs(1);
            RangeLists l = build_range(none.ph, 0, none.n(), 64, kn);
            if (!l.grow.empty()) expect(lanes_plan(l.grow, false, false, kn), false, "no probe", "a train without a probe");
        }
        Seq big = echo_train(31, true, true, every);
        expect(plan_of(big), false, "more than 24 live orders", "31 echoes (L = 32)");
    }

    printf("== the launcher's choice\n");
    {
        const LanesPlan lp = plan_of(echo_train(20, true, true, every));
        CHECK(!lanes_selected(lp, 72, knobs(1)));
        CHECK(!lanes_selected(lp, 256 * 256, knobs(1)));      // mse_256 stays on the rows layout
        CHECK(lanes_selected(lp, 1024 * 1024, knobs(1)));
        CHECK(lanes_selected(lp, LANES_MIN_VOXELS, knobs(1)) && !lanes_selected(lp, LANES_MIN_VOXELS - 1, knobs(1)));
        CHECK(lanes_selected(lp, 72, knobs(2)));
        CHECK(!lanes_selected(lp, 1024 * 1024, knobs(0)));
        LanesPlan no;
        CHECK(!lanes_selected(no, 1024 * 1024, knobs(2)));
    }
    printf("lanes_check: all checks passed\n");
    return 0;
}

// lanes_odd_check.cpp -- LanesPlan::odd and lanes_odd_selected (epgpy_amd/csrc/epgx_planner.{h,cpp}): which trains of the
// one-voxel-per-lane variant may run the kernel that computes the orders of one parity alone (rows_grow_lanes_kernel_odd), on a
// machine without a GPU.  The rule: the list is a train; every record that is not a head record has a leading and a trailing
// S(+1); no head record shifts; the shifts up to the last probe are an even number.
//
// Lists come from the planner that ships (operator streams as in lanes_train_check.cpp, made-up pool offsets) and, where a shape
// has to be exact, are written down record by record.  One line per check; exits non-zero at the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_lanes_bodies.h"
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
        op.reserved = zero;   // (a rotation's zero pattern travels in the operator: 1 about x, 3 about y)
        ph.ops.push_back(op);
        ph.zero_pattern.push_back((uint8_t)zero);
        ph.gather_tables.emplace_back();
    }
    void T(int64_t off, int pattern = 0) { push(EPGX_OP_T, 0, 0, off, 8, 0, pattern); }
    void E(int64_t off, bool real) {
        push(EPGX_OP_E, 0, 0, off, 4, 0, 0);
        ph.zero_pattern.back() = real ? 2 : 0;
    }
    void S(int n) { push(EPGX_OP_S, n, NOTRUNC, 0, 0, -1, 0); }
    void ADC() { push(EPGX_OP_ADC, n_adc++, 0, 0, 0, -1, 0); }
    void T0(int64_t off, int pattern) { push(EPGX_OP_T0, 0, 0, off, 12, 0, pattern); }
    // S E T S E of an echo about x, E . T . E fused on the host into one T0 (plan.py), with or without its probe
    void echo(bool adc = true) {
        S(1);
        T0(16, 1);
        S(1);
        if (adc) ADC();
    }
    int n() const { return (int)ph.ops.size(); }
};

static Seq new_seq() {
    Seq s;
    s.ph.n_spaces = 1;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = true;
    return s;
}

// the values knobs() takes with an empty environment, then EPGX_LANES, EPGX_LANES_BODY, EPGX_LANES_TRAIN, EPGX_LANES_ODD
static Knobs knobs(int lanes = 1, int body = 1, int train = 1, int odd = 1) {
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, lanes, body, train, odd};
    return k;
}

// excitation | n echoes about x, a probe behind every echo or behind every `every`-th
static Seq mse(int n, int every = 1) {
    Seq s = new_seq();
    s.T(0);
    for (int i = 0; i < n; ++i) s.echo((i + 1) % every == 0 || i == n - 1);
    return s;
}

static LanesPlan plan_of(const Seq &s, const char *what, const Knobs &kn = knobs()) {
    RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
    check(!l.grow.empty(), "the stream has a growing list");
    const LanesPlan lp = lanes_plan(l.grow, false, false, kn);
    printf("   %s: %zu records -> %s, L %d, rem0 %d, train %d, odd %d\n", what, l.grow.size(), lp.eligible ? "eligible" : lp.why, lp.L, lp.rem0,
           (int)lp.train, (int)lp.odd);
    return lp;
}

// a list written down: one execution group per record
struct List {
    std::vector<Rec> recs;
    void rec(uint32_t flags, int rep = 1, int slot = 0) {
        Rec r;
        memset(&r, 0, sizeof(r));
        r.flags = flags | (LEAF_NONE << 24);
        r.shift = (flags & F_S) ? 1 : 0;
        r.kmax = rep << 16;
        r.slot = slot;
        recs.push_back(r);
    }
    LanesPlan plan(const Knobs &kn = knobs()) const { return lanes_plan(recs, false, false, kn); }
};
static const uint32_t ECHO = F_S0 | F_T | F_TX | F_T0 | F_S;   // the folded echo

int main() {
    printf("== plain trains from the planner: 1 .. 23 echoes\n");
    int planned = 0, planned_other = 0;
    for (int n = 1; n <= 23; ++n) {
        // written down: the excitation, n echoes; probes behind every echo, or behind every other one and the last
        List l, m;
        l.rec(F_T);
        l.rec(ECHO | F_ADC, n);
        m.rec(F_T);
        for (int i = 0; i < n; ++i) m.rec((i % 2 == 1 || i == n - 1) ? (ECHO | F_ADC) : ECHO, 1, i / 2);
        CHECK(l.plan().eligible && l.plan().train && l.plan().odd && l.plan().L == n + 1 && l.plan().rem0 == 2 * n);
        CHECK(m.plan().eligible && m.plan().train && m.plan().odd && m.plan().L == n + 1 && m.plan().rem0 == 2 * n);
        // from the planner, where the train is long enough to become a growing launch at 64 orders
        if (build_range(mse(n).ph, 0, mse(n).n(), 64, knobs()).grow.empty()) continue;
        ++planned;
        const LanesPlan lp = plan_of(mse(n), "probe behind every echo");
        CHECK(lp.eligible && lp.train && lp.odd && lp.L == n + 1 && lp.rem0 == 2 * n);
        // (lists whose records alternate rarely become a growing launch: the written-down lists above carry that pattern)
        if (build_range(mse(n, 2).ph, 0, mse(n, 2).n(), 64, knobs()).grow.empty()) continue;
        ++planned_other;
        const LanesPlan lq = plan_of(mse(n, 2), "probe behind every other echo and the last");
        CHECK(lq.eligible && lq.train && lq.odd && lq.rem0 == 2 * n);
    }
    printf("   from the planner: %d trains probed behind every echo, %d probed behind every other\n", planned, planned_other);
    CHECK(planned >= 16);
    {
        Seq s = new_seq();   // records of several kinds before the first shift, none of them shifts
        s.T(0);
        s.E(80, false);
        s.T(32, 3);
        for (int i = 0; i < 20; ++i) s.echo();
        const LanesPlan lp = plan_of(s, "three operators before the first shift");
        CHECK(lp.eligible && lp.train && lp.odd && lp.L == 21 && lp.rem0 == 40);
    }

    printf("== lists written down\n");
    {
        List l;   // the headline's list as the kernel walks it; with a probe on the excitation as well
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 20);
        CHECK(l.plan().odd && l.plan().L == 21 && l.plan().rem0 == 40);
        List m;
        m.rec(F_T | F_ADC);
        m.rec(ECHO | F_ADC, 20, 1);
        CHECK(m.plan().train && m.plan().odd);
        List h;   // head records of every kind, repeated or not, as long as none shifts
        h.rec(F_T);
        h.rec(F_E | F_ER, 3);
        h.rec(F_T | F_TY);
        h.rec(F_T | F_E | F_ADC);
        h.rec(ECHO | F_ADC, 12, 1);
        CHECK(h.plan().train && h.plan().odd);
        List t;   // an unprobed tail: rem0 counts the shifts up to the last probe
        t.rec(F_T);
        t.rec(ECHO | F_ADC, 9);
        t.rec(ECHO, 10);
        CHECK(t.plan().train && t.plan().odd && t.plan().rem0 == 18 && t.plan().L == 10);
        List z;   // no head record at all
        z.rec(ECHO | F_ADC, 8);
        CHECK(z.plan().train && z.plan().odd);
    }
    {
        List l;   // a head record with a trailing shift: a train, with even windows on the way up -- and an odd rem0
        l.rec(F_T | F_S);
        l.rec(ECHO | F_ADC, 8);
        CHECK(l.plan().train && !l.plan().odd && l.plan().rem0 == 17);
        List m;   // the lone S(+1) behind the excitation
        m.rec(F_T);
        m.rec(F_S);
        m.rec(ECHO | F_ADC, 8);
        CHECK(m.plan().train && !m.plan().odd);
        // (a shifting head record and an odd rem0 come together: every later record of a train adds two shifts, and a record
        // shifts before it probes.  lanes_plan states both conditions; the kernel needs both)
        List e;
        e.rec(F_T | F_S | F_ADC);
        e.rec(ECHO, 8);
        CHECK(e.plan().eligible && e.plan().rem0 == 1 && !e.plan().odd);
    }
    {
        List l;   // no train: no odd class
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 5);
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 5, 5);
        CHECK(l.plan().eligible && !l.plan().train && !l.plan().odd);
        List h;   // the halves of an unfused echo
        h.rec(F_T);
        for (int i = 0; i < 8; ++i) {
            h.rec(F_E | F_ER | F_S);
            h.rec(F_T | F_TX | F_E | F_ER | F_S | F_ADC, 1, i);
        }
        CHECK(h.plan().eligible && !h.plan().train && !h.plan().odd);
        List r;   // refused by the variant
        r.rec(F_T);
        r.rec(ECHO | F_ADC, 31);
        CHECK(!r.plan().eligible && !r.plan().odd);
        List z;
        z.rec(F_T);
        z.rec(ECHO | F_ADC, 8);
        const LanesPlan from_state = lanes_plan(z.recs, true, false, knobs());
        CHECK(z.plan().odd);
        CHECK(!from_state.eligible && !from_state.odd);
    }
    {
        // MRF: an inversion, then per repetition a rotation of its own, relaxation, probe, relaxation, ONE shift: no parity
        Seq s = new_seq();
        s.T(0, 3);
        s.E(80, true);
        for (int i = 0; i < 40; ++i) {
            s.T(128 + 8 * i, 3);
            s.E(64, true);
            s.ADC();
            s.E(96, true);
            s.S(1);
        }
        const LanesPlan lp = plan_of(s, "MRF list");
        CHECK(lp.eligible && !lp.train && !lp.odd);
    }

    printf("== the knob and the size of the launch\n");
    {
        List l;
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 20);
        List m;   // a train that is not odd
        m.rec(F_T);
        m.rec(F_S);
        m.rec(ECHO | F_ADC, 20);
        const int64_t big = LANES_MIN_VOXELS, small = LANES_MIN_VOXELS - 1, tiny = 72;
        for (int odd = 0; odd <= 2; ++odd)
            for (int lanes = 0; lanes <= 2; ++lanes)
                for (int body = 0; body <= 1; ++body)
                    for (int train = 0; train <= 1; ++train) {
                        const Knobs kn = knobs(lanes, body, train, odd);
                        const LanesPlan lp = l.plan(kn);
                        // `odd` describes the list: the knobs do not change it (EPGX_LANES=0 refuses the list as a whole)
                        CHECK(lp.odd == (lanes != 0) && lp.train == (lanes != 0));
                        CHECK(!m.plan(kn).odd);
                        for (int64_t nvox : {tiny, small, big}) {
                            const bool lanes_on = lanes >= 2 || (lanes == 1 && nvox >= LANES_MIN_VOXELS);
                            const bool want = lanes_on && body && train && (odd >= 2 || (odd == 1 && nvox >= LANES_MIN_VOXELS));
                            CHECK(lanes_odd_selected(lp, nvox, kn) == want);
                            CHECK(!lanes_odd_selected(m.plan(kn), nvox, kn));
                            // the other choices do not see the knob
                            CHECK(lanes_selected(lp, nvox, kn) == lanes_selected(l.plan(knobs(lanes, body, train, 1)), nvox, knobs(lanes, body, train, 1)));
                            CHECK(lanes_train_selected(lp, kn) == (lanes != 0 && body && train));
                        }
                    }
        // the default, spelled out: forced lanes on a small grid stay on the train kernel, the benchmark's grid moves
        CHECK(!lanes_odd_selected(l.plan(knobs(2)), tiny, knobs(2)) && lanes_train_selected(l.plan(knobs(2)), knobs(2)));
        CHECK(lanes_odd_selected(l.plan(knobs(2, 1, 1, 2)), tiny, knobs(2, 1, 1, 2)));
        CHECK(lanes_odd_selected(l.plan(), 1024 * 1024, knobs()) && !lanes_odd_selected(l.plan(), 256 * 256, knobs()));
        Knobs d = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, 1};
        CHECK(d.lanes_odd == 1);   // the default of the field
    }
    printf("lanes_odd_check: all checks passed\n");
    return 0;
}

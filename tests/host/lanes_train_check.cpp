// lanes_train_check.cpp -- LanesPlan::train and lanes_train_selected (epgpy_amd/csrc/epgx_planner.{h,cpp}): which cut record lists
// of the one-voxel-per-lane variant may run its kernel WITHOUT a generic record body (rows_grow_lanes_kernel<NSP, true>), on a
// machine without a GPU.  The rule: the list is eligible, and every record either has a specialised body (lanes_body_id,
// epgx_lanes_bodies.h) or is a head record -- one that executes before any shift has taken place and has no leading shift
// (once, if it has a trailing one).
//
// Lists come from the planner that ships (operator streams as in lanes_check.cpp, made-up pool offsets) and, where a shape has
// to be exact, are written down record by record.  One line per check; exits non-zero at the first failure.
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
    // S E T S E ADC of an echo about x: as the operators stand, or with E . T . E fused on the host into one T0 (plan.py)
    void echo(bool fused, bool real = true) {
        S(1);
        if (fused) {
            T0(16, 1);
            S(1);
        } else {
            E(64, real); T(16, 1); S(1); E(64, real);
        }
        ADC();
    }
    int n() const { return (int)ph.ops.size(); }
};

static Seq new_seq(bool fold) {
    Seq s;
    s.ph.n_spaces = 1;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = fold;
    return s;
}

// the values knobs() takes with an empty environment, then EPGX_LANES, EPGX_LANES_BODY, EPGX_LANES_TRAIN
static Knobs knobs(int lanes = 1, int body = 1, int train = 1) {
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, lanes, body, train};
    return k;
}

// excitation | n echoes about x with relaxations on either side of the refocusing pulse: what bench.py's mse_* run
static Seq mse(int n, bool fused, bool real = true) {
    Seq s = new_seq(true);
    s.T(0);
    for (int i = 0; i < n; ++i) s.echo(fused, real);
    return s;
}

static void show(const std::vector<Rec> &list) {
    size_t shown = 0;
    for (const Rec &r : list) {
        if (++shown > 8) {
            printf("      ... %zu more\n", list.size() - 8);
            break;
        }
        const uint32_t f = r.flags, head = f >> 24;
        printf("      flags %08x  leaf %3u  count %d  body %d\n", f & 0xffffffu, head, (int)((uint32_t)r.kmax >> 16), lanes_body_id(f, head));
    }
}

static LanesPlan plan_of(const Seq &s, const char *what, const Knobs &kn = knobs()) {
    RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
    printf("   %s: %zu records in the cut list\n", what, l.grow.size());
    show(l.grow);
    check(!l.grow.empty(), "the stream has a growing list");
    const LanesPlan lp = lanes_plan(l.grow, false, false, kn);
    printf("      -> %s, train %d\n", lp.eligible ? "eligible" : lp.why, (int)lp.train);
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
static const uint32_t ECHO = F_S0 | F_T | F_TX | F_T0 | F_S;   // the folded echo: the one specialised body (echo-x)

int main() {
    static_assert(lanes_body_id(ECHO | (LEAF_NONE << 24), LEAF_NONE) == 0, "the folded echo has body 0");
    static_assert(lanes_body_id(F_T | (LEAF_NONE << 24), LEAF_NONE) < 0, "an excitation has none");

    printf("== trains from the planner\n");
    for (int n : {12, 20, 23}) {
        const LanesPlan lp = plan_of(mse(n, true), "fused train");
        CHECK(lp.eligible && lp.L == n + 1 && lp.train);
    }
    {
        const LanesPlan lp = plan_of(mse(20, false), "unfused train");
        CHECK(lp.eligible && lp.L == 21 && !lp.train);
        const LanesPlan lq = plan_of(mse(20, false, false), "unfused train with precession");
        CHECK(lq.eligible && !lq.train);
    }
    {
        // MRF: an inversion, then per repetition a rotation of its own, relaxation, probe, relaxation, one shift
        Seq s = new_seq(true);
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
        CHECK(lp.eligible && !lp.train);
    }
    {
        // an extra rotation between echoes 5 and 6: it executes after ten shifts and has no body
        Seq s = new_seq(true);
        s.T(0);
        for (int i = 0; i < 5; ++i) s.echo(true);
        s.T(32);
        for (int i = 0; i < 15; ++i) s.echo(true);
        const LanesPlan lp = plan_of(s, "train with an unlisted record after the first shift");
        CHECK(lp.eligible && !lp.train);
    }
    {
        // several records before the first shift: a general rotation, a relaxation with precession, a rotation about y
        Seq s = new_seq(true);
        s.T(0);
        s.E(80, false);
        s.T(32, 3);
        for (int i = 0; i < 20; ++i) s.echo(true);
        const LanesPlan lp = plan_of(s, "three records of several kinds before the first shift");
        CHECK(lp.eligible && lp.L == 21 && lp.train);
    }

    printf("== lists written down\n");
    {
        List l;   // the headline's list as the kernel walks it
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 20);
        CHECK(l.plan().eligible && l.plan().train && l.plan().L == 21);
    }
    {
        List l;   // head records of every kind the variant accepts, some repeated
        l.rec(F_T);
        l.rec(F_E);
        l.rec(F_E | F_ER, 3);
        l.rec(F_T | F_TY);
        l.rec(F_T | F_TX | F_T0);
        l.rec(F_T | F_E | F_ADC);
        l.rec(ECHO | F_ADC, 12);
        CHECK(l.plan().eligible && l.plan().train);
    }
    {
        List l;   // no head record at all
        l.rec(ECHO | F_ADC, 8);
        CHECK(l.plan().eligible && l.plan().train);
    }
    {
        List l;   // a record without a shift is a head record only while nothing has shifted
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 5);
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 5);
        CHECK(l.plan().eligible && !l.plan().train);
    }
    {
        List l;   // a trailing shift on a record that executes once before any shift: still order 0 alone, still a head record
        l.rec(F_T | F_S);
        l.rec(ECHO | F_ADC, 8);
        CHECK(l.plan().eligible && l.plan().train);
        List m;   // (a lone S(+1) behind the excitation: the odd-lead trains)
        m.rec(F_T);
        m.rec(F_S);
        m.rec(ECHO | F_ADC, 8);
        CHECK(m.plan().eligible && m.plan().train);
        List r;   // ... but its second execution would start at order 1, a second shifting record does, and a leading shift opens two orders
        r.rec(F_T | F_S, 2);
        r.rec(ECHO | F_ADC, 8);
        CHECK(r.plan().eligible && !r.plan().train);
        List q;
        q.rec(F_T | F_S);
        q.rec(F_S);
        q.rec(ECHO | F_ADC, 8);
        CHECK(q.plan().eligible && !q.plan().train);
        List p;
        p.rec(F_S0 | F_T);
        p.rec(ECHO | F_ADC, 8);
        CHECK(p.plan().eligible && !p.plan().train);
        // the halves of an unfused echo have no body
        List h;
        h.rec(F_T);
        for (int i = 0; i < 8; ++i) {
            h.rec(F_E | F_ER | F_S);
            h.rec(F_T | F_TX | F_E | F_ER | F_S | F_ADC, 1, i);
        }
        CHECK(h.plan().eligible && !h.plan().train);
    }
    {
        List l;   // an echo about another axis, one with a relaxation stage, one without the constant term
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 4);
        l.rec(F_S0 | F_T | F_T0 | F_S | F_ADC, 4, 4);
        CHECK(l.plan().eligible && !l.plan().train);
        List m;
        m.rec(F_T);
        m.rec(ECHO | F_E | F_ADC, 8);
        CHECK(m.plan().eligible && !m.plan().train);
        List n;
        n.rec(F_T);
        n.rec((ECHO & ~(uint32_t)F_T0) | F_ADC, 8);
        CHECK(n.plan().eligible && !n.plan().train);
    }
    {
        List l;   // a list the variant refuses is no train
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 31);
        CHECK(!l.plan().eligible && !l.plan().train);
        List m;
        m.rec(F_T);
        m.rec(ECHO, 8);
        CHECK(!m.plan().eligible && !m.plan().train && std::string(m.plan().why) == "no probe");
    }

    printf("== the knobs\n");
    {
        List l;
        l.rec(F_T);
        l.rec(ECHO | F_ADC, 20);
        List u;
        u.rec(F_T);
        u.rec(ECHO | F_E | F_ADC, 20);
        for (int lanes = 1; lanes <= 2; ++lanes) {
            // `train` describes the list, whatever EPGX_LANES_TRAIN and EPGX_LANES_BODY say; the choice of the kernel follows them
            CHECK(l.plan(knobs(lanes, 1, 1)).train && lanes_train_selected(l.plan(knobs(lanes, 1, 1)), knobs(lanes, 1, 1)));
            CHECK(l.plan(knobs(lanes, 1, 0)).train && !lanes_train_selected(l.plan(knobs(lanes, 1, 0)), knobs(lanes, 1, 0)));
            CHECK(l.plan(knobs(lanes, 0, 1)).train && !lanes_train_selected(l.plan(knobs(lanes, 0, 1)), knobs(lanes, 0, 1)));
            CHECK(!lanes_train_selected(u.plan(knobs(lanes, 1, 1)), knobs(lanes, 1, 1)));
        }
        CHECK(!l.plan(knobs(0)).eligible && !l.plan(knobs(0)).train && !lanes_train_selected(l.plan(knobs(0)), knobs(0)));
        Knobs d = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, 1};
        CHECK(d.lanes_body == 1 && d.lanes_train == 1);   // the defaults of the two fields
        // the knob takes no part in eligibility or in the choice between the variants
        CHECK(lanes_selected(l.plan(knobs(1, 1, 0)), 1024 * 1024, knobs(1, 1, 0)) && !lanes_selected(l.plan(knobs(1, 1, 0)), 72, knobs(1, 1, 0)));
        const LanesPlan from_state = lanes_plan(l.recs, true, false, knobs());
        CHECK(!from_state.eligible && !from_state.train);
    }
    printf("lanes_train_check: all checks passed\n");
    return 0;
}

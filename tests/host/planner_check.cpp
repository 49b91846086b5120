// planner_check.cpp -- the launch planner (epgpy_amd/csrc/epgx_planner.cpp) on a machine without a GPU.
//
// Builds epgx_op arrays directly, with made-up pool offsets (planning never reads a coefficient), runs the C++ that ships and
// checks its lists and decisions against rules restated here in the simplest form: record by record, execution by execution.
// One line per check; exits non-zero at the first failure.  `make` builds it, `make asan` with the address / undefined-behaviour
// sanitizers (tests/test_planner_host.py runs the plain build).
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

// ------------------------------------------------------------------ plans
static const int NOTRUNC = 1 << 20;   // S: ib >= K - 1 means no truncation

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
    void T(int64_t off, int space = 0) { push(EPGX_OP_T, 0, 0, off, 8, space, 0); }
    void T0(int64_t off, int space = 0) { push(EPGX_OP_T0, 0, 0, off, 12, space, 0); }
    void E(int64_t off, bool real, int space = 0) { push(EPGX_OP_E, 0, 0, off, 4, space, real ? 2 : 0); }
    void S(int n) { push(EPGX_OP_S, n, NOTRUNC, 0, 0, -1, 0); }
    void ADC() { push(EPGX_OP_ADC, n_adc++, 0, 0, 0, -1, 0); }
    int n() const { return (int)ph.ops.size(); }
};

static Seq new_seq(bool fold) {
    Seq s;
    s.ph.n_spaces = 1;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = fold;
    return s;
}

static Knobs defaults() {   // the values knobs() takes with an empty environment
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1};
    return k;
}

// T | (E S T E S ADC) x n with the same tables, real relaxations (they fold into the rotations), `tail` unprobed echoes behind
static Seq echo_train(int n, int tail = 0) {
    Seq s = new_seq(true);
    s.T(0);
    for (int i = 0; i < n + tail; ++i) {
        s.E(64, true);
        s.S(1);
        s.T(16);
        s.E(64, true);
        s.S(1);
        if (i < n) s.ADC();
    }
    return s;
}

// T | (S T ADC) x n: one shift per probe
static Seq shift_train(int n) {
    Seq s = new_seq(false);
    s.T(0);
    for (int i = 0; i < n; ++i) {
        s.S(1);
        s.T(16);
        s.ADC();
    }
    return s;
}

// ------------------------------------------------------------------ lists
static int count_of(const Rec &r) { return (int)((uint32_t)r.kmax >> 16); }
static uint32_t leaf_of(const Rec &r) { return r.flags >> 24; }
static int shifts_of(const Rec &r) { return ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0); }

// a folded list as the record executions it stands for: headers dropped, repeat counts unrolled, ADC slots advancing by one
static std::vector<Rec> expand(const std::vector<Rec> &list, std::vector<int> *owner = nullptr) {
    std::vector<Rec> out;
    size_t members = 0;
    for (size_t i = 0; i < list.size(); ++i) {
        const Rec &r = list[i];
        if (!members && (leaf_of(r) == LEAF_PAIR || leaf_of(r) == LEAF_SINGLE)) {
            members = (size_t)(leaf_of(r) == LEAF_PAIR ? 2 : 1) * (size_t)count_of(r);
            continue;
        }
        int rep = count_of(r) > 0 ? count_of(r) : 1;
        if (members) {
            --members;
            if (rep != 1) check(false, "a record inside a run carries a repeat count");
        }
        for (int j = 0; j < rep; ++j) {
            Rec c = r;
            if (r.flags & F_ADC) c.slot = r.slot + j;
            out.push_back(c);
            if (owner) owner->push_back((int)i);
        }
    }
    return out;
}

// the fields the folds do not rewrite
static bool same_record(const Rec &a, const Rec &b) {
    return (a.flags & 0xffffffu) == (b.flags & 0xffffffu) && a.shift == b.shift && (a.kmax & 0xffff) == (b.kmax & 0xffff) && a.slot == b.slot &&
           a.t_off == b.t_off && a.e_off == b.e_off && a.t_ix == b.t_ix && a.e_ix == b.e_ix;
}
static bool same_list(const std::vector<Rec> &a, const std::vector<Rec> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!same_record(a[i], b[i])) return false;
    return true;
}
static int headers(const std::vector<Rec> &list, uint32_t leaf, int *count = nullptr) {
    int n = 0;
    size_t members = 0;
    for (const Rec &r : list) {
        if (members) {
            --members;
            continue;
        }
        if (leaf_of(r) == LEAF_PAIR || leaf_of(r) == LEAF_SINGLE) {
            members = (size_t)(leaf_of(r) == LEAF_PAIR ? 2 : 1) * (size_t)count_of(r);
            if (leaf_of(r) == leaf) {
                ++n;
                if (count) *count = count_of(r);
            }
        }
    }
    return n;
}

static void lossless(const RangeLists &l, const char *what) {
    printf("-- lossless: %s (%zu records, %zu in runs, %zu in grow)\n", what, l.recs.size(), l.runs.size(), l.grow.size());
    CHECK(l.n_rec == (int)l.recs.size() && l.n_runs == (int)l.runs.size() && l.n_grow == (int)l.grow.size() && l.n_druns == (int)l.druns.size());
    if (!l.runs.empty()) CHECK(same_list(expand(l.runs), l.recs));
    if (!l.grow.empty()) CHECK(same_list(expand(l.grow), expand(l.runs)));
}

// ------------------------------------------------------------------ repeat count
static void test_repeat_count() {
    printf("== repeat count\n");
    {
        Seq s = echo_train(20);
        RangeLists l = build_range(s.ph, 0, s.n(), 64, defaults());
        lossless(l, "20-echo train");
        CHECK(!l.runs.empty());
        int carriers = 0, carried = 0;
        for (const Rec &r : l.runs)
            if (count_of(r) > 1) {
                ++carriers;
                carried = count_of(r);
            }
        // the excitation and the first echo have shapes of their own (no E_b, no leading shift); the other 19 echoes are one record
        CHECK(carriers == 1);
        CHECK(carried == 19);
        CHECK(headers(l.runs, LEAF_PAIR) == 0 && headers(l.runs, LEAF_SINGLE) == 0);
    }
    {
        const int n = 0x7fff + 2;     // 0x8000 identical echoes behind the first: one more than a count holds
        Seq s = echo_train(n);
        Knobs kn = defaults();
        RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
        lossless(l, "0x7fff + 2 echoes");
        int most = 0, carriers = 0;
        for (const Rec &r : l.runs) {
            most = count_of(r) > most ? count_of(r) : most;
            carriers += count_of(r) > 1 ? 1 : 0;
        }
        CHECK(most == 0x7fff);
        CHECK(carriers == 1);                      // (the one left over is an ordinary record)
        CHECK(l.runs.size() == l.recs.size() - 0x7fff + 1);
    }
}

// ------------------------------------------------------------------ run thresholds
// `pairs` x [T E S ADC][E S] with distinct tables, or `pairs` x folded [T.E S ADC] with distinct rotations; behind them ten
// identical records (they fold into one repeat count, so that the list is kept whatever the pairs do)
static Seq pair_seq(int pairs, int suffix) {
    Seq s = new_seq(false);
    for (int i = 0; i < pairs; ++i) {
        s.T(1000 + 16 * i);
        s.E(64, false);
        s.S(1);
        s.ADC();
        s.E(128, false);
        s.S(1);
    }
    for (int i = 0; i < suffix; ++i) {
        s.T(16);
        s.E(64, false);
        s.S(1);
        s.ADC();
    }
    return s;
}
static Seq single_seq(int singles, int suffix) {
    Seq s = new_seq(true);
    for (int i = 0; i < singles + suffix; ++i) {
        s.T(i < singles ? 1000 + 16 * i : 16);
        s.E(64, true);
        s.S(1);
        s.ADC();
    }
    return s;
}
static void test_run_thresholds() {
    printf("== run thresholds\n");
    for (int n = 3; n <= 4; ++n) {
        Seq s = pair_seq(n, 10);
        RangeLists l = build_range(s.ph, 0, s.n(), 64, defaults());
        lossless(l, n == 3 ? "3 pairs + 10 identical" : "4 pairs + 10 identical");
        CHECK((int)l.recs.size() == 2 * n + 10);
        CHECK(!l.runs.empty());
        int count = 0;
        CHECK(headers(l.runs, LEAF_PAIR, &count) == (n == 4 ? 1 : 0));
        if (n == 4) CHECK(count == 4);
    }
    for (int n = 3; n <= 4; ++n) {
        Seq s = single_seq(n, 10);
        RangeLists l = build_range(s.ph, 0, s.n(), 64, defaults());
        lossless(l, n == 3 ? "3 folded singles + 10 identical" : "4 folded singles + 10 identical");
        CHECK((int)l.recs.size() == n + 10);
        for (const Rec &r : l.recs) CHECK(r.flags & F_FOLD);
        CHECK(!l.runs.empty());
        int count = 0;
        CHECK(headers(l.runs, LEAF_SINGLE, &count) == (n == 4 ? 1 : 0));
        if (n == 4) CHECK(count == 4);
    }
    {   // the keep rule: dropped when the list saves under a quarter of the records and pair runs cover under half
        Seq s = pair_seq(3, 0);       // 6 records, nothing folds: 6 > 3/4 x 6, no pair run
        RangeLists l = build_range(s.ph, 0, s.n(), 64, defaults());
        CHECK(l.recs.size() == 6 && l.runs.empty() && l.n_runs == 0);
        Seq p = pair_seq(4, 0);       // 8 records + a header: saves nothing, but the pair run covers all
        l = build_range(p.ph, 0, p.n(), 64, defaults());
        lossless(l, "4 pairs alone");
        CHECK(l.recs.size() == 8 && l.runs.size() == 9);
        Seq q = pair_seq(4, 9);       // the pair run covers 8 of 17 (under half), the list has 10 <= 3/4 x 17: kept on the saving
        l = build_range(q.ph, 0, q.n(), 64, defaults());
        lossless(l, "4 pairs + 9 identical");
        CHECK(l.recs.size() == 17 && l.runs.size() == 10);
    }
}

// ------------------------------------------------------------------ rows_grow phases
// the running shift count after every record execution of a list
static std::vector<int> running_shifts(const std::vector<Rec> &execs) {
    std::vector<int> top;
    int t = 0;
    for (const Rec &r : execs) top.push_back(t += shifts_of(r));
    return top;
}

// what test_reach_rule.shifts_left implies: an execution with `rem` shifts left up to the last probe (its own included: a record
// shifts before it probes) and `top` populated orders needs 1 + min(top, rem) orders; a range the smallest of 16 / 32 / 64 that holds
// the need of its executions
static void reach_caps(const RangeLists &l, int want[3]) {
    std::vector<int> owner;
    const std::vector<Rec> ex = expand(l.grow, &owner);
    const std::vector<int> top = running_shifts(ex);
    int last = -1;
    for (size_t i = 0; i < ex.size(); ++i)
        if (ex[i].flags & F_ADC) last = (int)i;
    int need[3] = {0, 0, 0};
    for (int i = 0; i <= last; ++i) {
        const int rem = top[(size_t)last] - (i ? top[(size_t)i - 1] : 0);
        const int p = owner[(size_t)i] < l.grow1 ? 0 : (owner[(size_t)i] < l.grow2 ? 1 : 2);
        const int n = 1 + (top[(size_t)i] < rem ? top[(size_t)i] : rem);
        need[p] = n > need[p] ? n : need[p];
    }
    const int today[3] = {16, 32, 64};
    for (int p = 0; p < 3; ++p) {
        const int fit = need[p] <= 16 ? 16 : (need[p] <= 32 ? 32 : 64);
        want[p] = last < 0 ? today[p] : (fit < today[p] ? fit : today[p]);
    }
}

static void check_phase_starts(const RangeLists &l) {
    std::vector<int> owner;
    const std::vector<Rec> ex = expand(l.grow, &owner);
    const std::vector<int> top = running_shifts(ex);
    // grow1 / grow2 = the first records whose running shift count exceeds 15 / 31: everything in front stays at or below
    int first15 = (int)l.grow.size(), first31 = (int)l.grow.size();
    for (size_t i = ex.size(); i-- > 0;) {
        if (top[i] > 15) first15 = owner[i];
        if (top[i] > 31) first31 = owner[i];
    }
    CHECK(l.grow1 == first15);
    CHECK(l.grow2 == first31);
    for (size_t i = 0; i < ex.size(); ++i) {
        if (owner[i] < l.grow1) CHECK(top[i] <= 15);
        else if (owner[i] < l.grow2) CHECK(top[i] <= 31);
    }
}

static void test_grow_phases() {
    printf("== rows_grow phases\n");
    Knobs kn = defaults();
    {
        Seq s = echo_train(20);
        RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
        lossless(l, "20-echo train");
        CHECK(!l.grow.empty());
        check_phase_starts(l);
        // the record that carries 19 echoes (2 shifts each, from 2) straddles both boundaries: cut into 6 (up to 14), 8 (up to 30) and 5
        CHECK(l.grow.size() == l.runs.size() + 2);
        CHECK(l.grow1 == 3 && l.grow2 == 4);
        CHECK(count_of(l.grow[2]) == 6 && count_of(l.grow[3]) == 8 && count_of(l.grow[4]) == 5);
        CHECK(l.grow[3].slot == l.grow[2].slot + 6 && l.grow[4].slot == l.grow[3].slot + 8);
    }
    const int trains[5][2] = {{20, 0}, {20, 3}, {20, 12}, {24, 3}, {40, 3}};   // (echoes, unprobed echoes behind): the last range at 16, 32 and 64
    for (const auto &nt : trains) {
        const int tail = nt[1];
        Seq s = echo_train(nt[0], tail);
        RangeLists l = build_range(s.ph, 0, s.n(), 64, kn);
        lossless(l, "echo train with unprobed echoes behind");
        CHECK(!l.grow.empty());
        check_phase_starts(l);
        int want[3];
        reach_caps(l, want);
        printf("   %d echoes + %d: grow_cap %d %d %d, the rule gives %d %d %d\n", nt[0], tail, l.grow_cap[0], l.grow_cap[1], l.grow_cap[2], want[0], want[1], want[2]);
        CHECK(l.grow_cap[0] <= 16 && l.grow_cap[1] <= 32 && l.grow_cap[2] <= 64);
        CHECK(l.grow_cap[0] == want[0] && l.grow_cap[1] == want[1] && l.grow_cap[2] == want[2]);
        Knobs off = kn;
        off.reach = false;
        off.grow_share = 0.0;
        RangeLists m = build_range(s.ph, 0, s.n(), 64, off);
        CHECK(!m.grow.empty());
        CHECK(m.grow_cap[0] == 16 && m.grow_cap[1] == 32 && m.grow_cap[2] == 64);
    }
    {   // 20 echoes without the reach rule: 2 + 6 + 8 of the 21 executions run below 64 orders
        Seq s = echo_train(20);
        Knobs off = kn;
        off.reach = false;
        off.grow_share = 0.7;
        CHECK(!build_range(s.ph, 0, s.n(), 64, off).grow.empty());
        off.grow_share = 0.8;
        RangeLists l = build_range(s.ph, 0, s.n(), 64, off);
        CHECK(l.grow.empty() && l.n_grow == 0);
        CHECK(!l.runs.empty());
    }
}

// ------------------------------------------------------------------ cgrow
static void test_cgrow() {
    printf("== cgrow\n");
    static const int cap[6] = {63, 127, 255, 511, 1023, 1535};
    Seq s = shift_train(140);
    for (int K : {128, 256, 512, 1024, 2048}) {
        RangeLists l = build_range(s.ph, 0, s.n(), K, defaults());
        for (int q = 1; q < 6; ++q) CHECK(l.cgrow[q] >= l.cgrow[q - 1]);
        for (int q = 0; q < 6; ++q)
            if (cap[q] + 1 >= K) CHECK(l.cgrow[q] == l.n_rec);
        CHECK(l.runs.empty() && l.grow.empty());
    }
    {
        RangeLists l = build_range(s.ph, 0, s.n(), 256, defaults());
        const std::vector<int> top = running_shifts(l.recs);
        CHECK(top.back() == 140);
        int pass63 = -1, pass127 = -1, counted = 0;
        for (size_t i = 0; i < top.size(); ++i) {
            if (pass63 < 0 && top[i] > 63) pass63 = (int)i;
            if (pass127 < 0 && top[i] > 127) pass127 = (int)i;
            counted += top[i] <= 127 ? 1 : 0;      // (runs while fewer orders than the capacity's 256 can hold anything: 64 or 128)
        }
        CHECK(l.cgrow[0] == pass63);
        CHECK(l.cgrow[1] == pass127);
        CHECK(l.cgrow[2] == l.n_rec && l.cgrow[3] == l.n_rec);
        CHECK(l.cgrow_share == (double)counted / l.n_rec);
    }
    {
        Seq w = shift_train(600);
        RangeLists l = build_range(w.ph, 0, w.n(), 2048, defaults());
        const std::vector<int> top = running_shifts(l.recs);
        int pass511 = -1, adc = 0;
        for (size_t i = 0; i < top.size() && pass511 < 0; ++i) {
            if (top[i] > 511) pass511 = (int)i;
            else adc += (l.recs[i].flags & F_ADC) ? 1 : 0;
        }
        CHECK(pass511 > 0 && l.cgrow[3] == pass511);
        CHECK(l.cgrow_adc3 == adc);
        CHECK(adc > 500);
    }
}

// ------------------------------------------------------------------ derivative runs
static void test_deriv_runs() {
    printf("== derivative runs\n");
    // a probed excitation, eight fused echoes [S T0 ADC] with tables of their own and a partial each, a relaxation with a probe behind
    Seq s = new_seq(false);
    s.ph.n_vars = 1;
    s.T(0);
    s.ADC();
    for (int i = 0; i < 8; ++i) {
        s.S(1);
        s.T0(1000 + 16 * i);
        s.ADC();
    }
    s.E(64, false);
    s.ADC();
    for (int i = 0; i < s.n(); ++i) {
        epgx_dop d;
        memset(&d, 0, sizeof(d));
        for (int v = 0; v < EPGX_MAX_VARS; ++v) d.coef_off[v] = d.space[v] = -1;
        if (s.ph.ops[(size_t)i].opcode == EPGX_OP_T0) d.coef_off[0] = 5000 + 16 * i;
        s.ph.dops.push_back(d);
        s.ph.dpattern.push_back(0);
    }
    RangeLists l = build_range(s.ph, 0, s.n(), 64, defaults());
    lossless(l, "fused echoes with a partial");
    CHECK(l.drecs.size() == l.recs.size() && l.runs.empty() && l.grow.empty());
    CHECK(!l.druns.empty() && l.ddruns.size() == l.druns.size() && l.bdruns.size() == l.druns.size());
    CHECK(l.drun_headers == 1);
    // headers dropped, the list is the packed records and their DRecs again (nothing folds here: the plan has no log tables)
    std::vector<Rec> flat;
    std::vector<DRec> dflat;
    DRec zero;
    memset(&zero, 0, sizeof(zero));
    int inside = 0;
    for (size_t i = 0; i < l.druns.size(); ++i) {
        if (leaf_of(l.druns[i]) == LEAF_DRUN) {
            CHECK(memcmp(&l.ddruns[i], &zero, sizeof(zero)) == 0);
            CHECK((int)(l.druns[i].flags & 0x1ffu & ~(uint32_t)DRUN_IDENT) == l.drun_code);
            inside += count_of(l.druns[i]);
            continue;
        }
        flat.push_back(l.druns[i]);
        dflat.push_back(l.ddruns[i]);
    }
    CHECK(inside == l.drun_inside && inside >= 7);
    CHECK(same_list(flat, l.recs));
    CHECK(dflat.size() == l.drecs.size() && memcmp(dflat.data(), l.drecs.data(), dflat.size() * sizeof(DRec)) == 0);
}

// ------------------------------------------------------------------ choose_kernel
struct Row {
    const char *what;
    int K;
    bool has_in, has_out;
    int n_vars, n_spaces;
    bool runs, grow, druns;
    int drun_code;
    double cgrow_share;
    int cgrow_knob;       // Knobs::cgrow
    const char *name;     // as the GPU tests pin it (tests/signal_cases.py, tests/jacobian_cases.py, tests/test_gpu_contract.py)
    Family family;
};

static RangeLists lists_for(const Row &r) {
    RangeLists l;
    Rec rec;
    memset(&rec, 0, sizeof(rec));
    l.K = r.K;
    l.recs.assign(3, rec);
    l.n_rec = 3;
    if (r.runs) l.runs.assign(2, rec);
    if (r.grow) l.grow.assign(2, rec);
    if (r.druns) {
        l.druns.assign(2, rec);
        l.ddruns.resize(2);
        l.bdruns.resize(2);
    }
    l.n_runs = (int)l.runs.size();
    l.n_grow = (int)l.grow.size();
    l.n_druns = (int)l.druns.size();
    l.drun_code = r.drun_code;
    l.cgrow_share = r.cgrow_share;
    for (int q = 0; q < 6; ++q) l.cgrow[q] = r.cgrow_share > 0 ? 2 : 3;
    return l;
}

static void test_choose_kernel() {
    printf("== choose_kernel\n");
    Seq s = shift_train(1);
    const int n = s.n();
    const Row rows[] = {
        {"FAM_ROWS_GROW", 64, false, false, 0, 1, true, true, false, 0, 0, 1, "rows_grow_kernel<1>", FAM_ROWS_GROW},
        {"FAM_ROWS with runs", 64, false, false, 0, 2, true, false, false, 0, 0, 1, "rows_kernel<2, 4, true>", FAM_ROWS},
        {"FAM_ROWS at 16 orders", 16, false, false, 0, 2, false, false, false, 0, 0, 1, "rows_kernel<2, 1, false>", FAM_ROWS},
        {"FAM_ROWS at 128 orders", 128, false, false, 0, 1, false, false, false, 0, 0, 1, "rows_kernel<1, 8, false>", FAM_ROWS},
        {"FAM_RUN, state out", 64, false, true, 0, 1, true, true, false, 0, 0, 1, "run_kernel<1, 1, false>", FAM_RUN},
        {"FAM_RUN, state in and out", 64, true, true, 0, 1, true, true, false, 0, 0, 1, "run_kernel<1, 1, true>", FAM_RUN},
        {"FAM_RUN at 1024 orders", 1024, true, true, 0, 1, false, false, false, 0, 0.9, 1, "run_kernel<16, 1, true>", FAM_RUN},
        {"FAM_RUN_CONTIG", 128, true, false, 0, 1, false, false, false, 0, 0.9, 1, "run_contig_kernel<2, 1, true>", FAM_RUN_CONTIG},
        {"FAM_RUN_CONTIG from equilibrium", 512, false, false, 0, 4, false, false, false, 0, 0.05, 1, "run_contig_kernel<8, 4, false>", FAM_RUN_CONTIG},
        {"FAM_RUN_CONTIG_GROW", 256, false, false, 0, 1, false, false, false, 0, 0.5, 1, "run_contig_grow_kernel<4, 1>", FAM_RUN_CONTIG_GROW},
        {"K = 128, share 0.59", 128, false, false, 0, 1, false, false, false, 0, 0.59, 1, "rows_kernel<1, 8, false>", FAM_ROWS},
        {"K = 128, share 0.61", 128, false, false, 0, 1, false, false, false, 0, 0.61, 1, "run_contig_grow_kernel<2, 1>", FAM_RUN_CONTIG_GROW},
        {"K = 128, share 0.59, EPGX_CGROW=2", 128, false, false, 0, 1, false, false, false, 0, 0.59, 2, "run_contig_grow_kernel<2, 1>", FAM_RUN_CONTIG_GROW},
        {"K = 256, EPGX_CGROW=0", 256, false, false, 0, 1, false, false, false, 0, 0.5, 0, "run_contig_kernel<4, 1, false>", FAM_RUN_CONTIG},
        {"FAM_RUN_SPLIT, two legs", 2048, false, false, 0, 1, false, false, false, 0, 0.5, 1, "run_kernel<8, 1, false> + run_split_kernel<4, 1, true>", FAM_RUN_SPLIT},
        {"FAM_RUN_SPLIT, one leg", 2048, false, false, 0, 2, false, false, false, 0, 0.0, 1, "run_split_kernel<4, 2, false>", FAM_RUN_SPLIT},
        {"FAM_DERIV, consecutive orders", 128, false, false, 1, 1, false, false, false, 0, 0, 1, "deriv_kernel<2, 1, 1, true>", FAM_DERIV},
        {"FAM_DERIV from a state", 64, true, false, 2, 3, false, false, false, 0, 0, 1, "deriv_kernel<1, 4, 2>", FAM_DERIV},
        {"FAM_DERIV, three states at 256", 256, false, false, 3, 2, false, false, false, 0, 0, 1, "deriv_kernel<4, 2, 3>", FAM_DERIV},
        {"FAM_PACKED_DERIV", 16, false, false, 2, 2, false, false, false, 0, 0, 1, "packed_deriv_kernel<2, 2, 16>", FAM_PACKED_DERIV},
        {"FAM_ROWS_DERIV", 64, false, false, 1, 1, false, false, false, 0, 0, 1, "rows_deriv_kernel<1, 4, 1>", FAM_ROWS_DERIV},
        {"FAM_ROWS_DERIV, two states", 64, false, false, 2, 3, false, false, false, 0, 0, 1, "rows_deriv_kernel<4, 4, 2>", FAM_ROWS_DERIV},
        {"FAM_DRUN, logarithmic partials", 64, false, false, 2, 3, false, false, true, 309, 0, 1, "drun_kernel<4, 2, 309, 0>", FAM_DRUN},
        {"FAM_DRUN, folded", 64, false, false, 2, 3, false, false, true, 154, 0, 1, "drun_kernel<4, 2, 154, 0>", FAM_DRUN},
        {"FAM_DRUN, folded, three states", 64, false, false, 3, 3, false, false, true, 154, 0, 1, "drun_kernel<4, 1, 154, 2> + drun_kernel<4, 2, 154, 0>", FAM_DRUN},
        {"FAM_PACKED_DFOLD", 16, false, false, 2, 3, false, false, true, 154, 0, 1, "packed_dfold_kernel<2, 16>", FAM_PACKED_DFOLD},
    };
    for (const Row &r : rows) {
        s.ph.n_vars = r.n_vars;
        s.ph.n_spaces = r.n_spaces;
        Knobs kn = defaults();
        kn.cgrow = r.cgrow_knob;
        Choice c;
        const int rc = choose_kernel(s.ph, lists_for(r), 0, n, r.K, r.has_in, r.has_out, kn, &c);
        printf("   %-36s -> %s\n", r.what, rc ? g_err : c.name);
        check(rc == EPGX_OK && std::string(c.name) == r.name && c.family == r.family, r.what);
        check(c.packed16 == (r.K == 16 || r.K == 32) && c.wide == (r.K == 2048) && !c.has_nd && c.lds_mode == 0, "  ... and the facts of the launch");
    }

    printf("== choose_kernel: EPGX_ERR_UNSUPPORTED\n");
    struct Bad {
        int K;
        bool has_in, has_out;
        int n_vars;
        bool big_pool, use_lds, big_shift;
        const char *message;
    };
    const Bad bad[] = {
        {16, false, false, 0, true, false, false, "epgx_run: K = 16 / 32 need a coefficient pool below 2 GiB (use K = 64)"},
        {2048, false, false, 0, false, true, false, "epgx_run: K = 2048 handles rotations, relaxation, shifts by +-1 and probes only (no derivative states)"},
        {2048, false, false, 1, false, false, false, "epgx_run: K = 2048 handles rotations, relaxation, shifts by +-1 and probes only (no derivative states)"},
        {32, false, false, 0, false, true, true, "epgx_run: K = 16 / 32 handle shifts by +-1 (and, at K = 16, gather shifts) only"},
        {16, true, false, 1, false, false, false, "epgx_run: K = 16 / 32 derivative plans start from equilibrium"},
        {16, false, false, 1, false, true, false, "epgx_run: K = 16 / 32 derivative plans handle shifts by +-1 only"},
        {64, false, true, 1, false, false, false, "epgx_run: derivative plans run state-resident (out = NULL)"},
        {2048, true, false, 1, false, false, false, "epgx_run: derivative plans support K <= 1024, got 2048"},
        {1024, false, false, 2, false, false, false, "epgx_run: at K = 1024 a launch carries ONE derivative state (plan has 2 variables: one plan per variable)"},
    };
    for (const Bad &b : bad) {
        Seq q = shift_train(1);
        q.ph.n_vars = b.n_vars;
        if (b.big_pool) q.ph.n_pool = (int64_t)1 << 28;
        Row r = {"", b.K, b.has_in, b.has_out, b.n_vars, 1, false, false, false, 0, 0, 1, "", FAM_RUN};
        RangeLists l = lists_for(r);
        l.use_lds = b.use_lds;
        l.big_shift = b.big_shift;
        Choice c;
        g_err[0] = 0;
        const int rc = choose_kernel(q.ph, l, 0, q.n(), b.K, b.has_in, b.has_out, defaults(), &c);
        printf("   K = %d: %s\n", b.K, g_err);
        check(rc == EPGX_ERR_UNSUPPORTED && std::string(g_err) == b.message, b.message);
    }
}

// ------------------------------------------------------------------ tiled schedule
static void test_tiled() {
    printf("== tiled_schedule\n");
    Seq s = new_seq(false);
    s.T(0);
    for (int i = 0; i < 100; ++i) {
        s.S(1);
        s.T(16);
        s.ADC();
    }
    s.S(3);
    s.ADC();
    s.S(-1);
    s.S(40);
    s.ADC();
    for (int H : {32, 2}) {
        TiledSchedule ts;
        CHECK(tiled_schedule(s.ph, 4096, 0, 8, H, defaults(), ts) == EPGX_OK);
        int next = 0, shift_steps = 0, blocks = 0;
        for (const TiledStep &st : ts.steps) {
            if (st.shift) {     // a shift above H is a step of its own: no records
                ++shift_steps;
                CHECK(std::abs(st.shift) > H);
                continue;
            }
            ++blocks;
            CHECK(st.rec0 == next && st.rec1 > st.rec0);      // contiguous, every record once
            next = st.rec1;
            int units = 0;
            for (int i = st.rec0; i < st.rec1; ++i) {
                units += shifts_of(ts.recs[(size_t)i]);
                if ((ts.recs[(size_t)i].flags & F_S) && !(ts.recs[(size_t)i].flags & F_FOLD)) CHECK(std::abs(ts.recs[(size_t)i].shift) == 1);
            }
            CHECK(units <= H);
        }
        CHECK(next == (int)ts.recs.size());
        CHECK(shift_steps == ts.n_shift && shift_steps == (H == 32 ? 1 : 2));      // S(40) at both halos, S(3) at H = 2
        CHECK(blocks >= (100 + (H == 32 ? 4 : 1)) / H);
        CHECK(ts.has_adc && ts.peak == 100 + 3 + 1 + 40);
    }
    TiledSchedule ts;
    CHECK(tiled_schedule(s.ph, 128, 0, 8, 32, defaults(), ts) == EPGX_ERR_INVALID);
    CHECK(std::string(g_err) == "epgx_run_tiled: the plan populates orders up to 144, Kbuf=128");
}

int main() {
    test_repeat_count();
    test_run_thresholds();
    test_grow_phases();
    test_cgrow();
    test_deriv_runs();
    test_choose_kernel();
    test_tiled();
    printf("planner_check: all checks passed\n");
    return 0;
}

// run_check.cpp -- run analysis (epgpy_amd/csrc/epgx_run_check.cpp) on a machine without a GPU.
//
// Builds PlanHost / PlanGeometry values by hand (the smallest operator lists that reach each line), describes a call of epgx_run,
// epgx_kernel_for or a tiled entry point as a RunRequest / TiledRequest and runs the C++ that ships: every refusal with its code
// and its full message, the order of the checks, the routes with their kernel names, the tile shapes and the slab rule.  One line
// per check; exits non-zero at the first failure.  `make run_check` builds it, `make asan` with the address / undefined-behaviour
// sanitizers (tests/test_run_check_host.py runs the plain build).
//
// The message texts are those of epgx_api.hip before the analysis moved out of it.  Refusals this program cannot reach are the
// ones that compare handles (NULL context or plan, a plan of another context: tests/test_gpu_run_check.py) and those that need
// the record lists or the device (choose_kernel's own, uploads, launches).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_run_check.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) exit(1);
}
#define CHECK(cond) check((cond), #cond)

static Knobs defaults() {   // the values knobs() takes with an empty environment
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1, 1};
    return k;
}

static const int INV = EPGX_ERR_INVALID, UNS = EPGX_ERR_UNSUPPORTED;
static const int NOTRUNC = 1 << 20;

// ------------------------------------------------------------------ plans and requests
static epgx_op op(int opcode, int ia = 0, int ib = 0, int ncoef = 0) {
    epgx_op o;
    memset(&o, 0, sizeof(o));
    o.opcode = opcode, o.space = -1, o.ia = ia, o.ib = ib, o.ncoef = ncoef;
    return o;
}
static epgx_op T() { return op(EPGX_OP_T, 0, 0, 8); }
static epgx_op S(int n = 1) { return op(EPGX_OP_S, n, NOTRUNC); }
static epgx_op ADC(int slot = 0) { return op(EPGX_OP_ADC, slot); }
static epgx_op D(int K) { return op(EPGX_OP_D, 0, 0, 3 * K); }
static epgx_op GS(int K) { return op(EPGX_OP_GS, 0, 0, 3 * K / 2); }
static epgx_op X(int N, int ib = 1) { return op(EPGX_OP_X, N, ib, 3 * N * N); }

struct P {
    PlanHost h;
    PlanGeometry g;
};
// `ops` over a 1-D grid of `nvox` voxels; exchange between N compartments `ib` voxels apart when the list holds an X
static P plan(const std::vector<epgx_op> &ops, int64_t nvox = 8, int n_vars = 0) {
    P p;
    p.h.ops = ops;
    p.h.gather_tables.resize(ops.size());
    p.h.n_vars = n_vars;
    p.g.ndim = 1, p.g.shape[0] = nvox, p.g.nvox_total = nvox;
    for (const epgx_op &o : ops)
        if (o.opcode == EPGX_OP_X) p.g.x_ncomp = o.ia, p.g.x_span = (int64_t)o.ia * o.ib;
    return p;
}
static P xplan(int N, int64_t nvox, int n_vars = 0, std::vector<epgx_op> extra = {}) {   // T X S ADC (+ extra)
    std::vector<epgx_op> ops = {T(), X(N), S(), ADC()};
    ops.insert(ops.end(), extra.begin(), extra.end());
    return plan(ops, nvox, n_vars);
}

// the whole plan over the whole grid at capacity K, with a signal buffer that has room
static RunRequest request(const P &p, int K) {
    RunRequest rq;
    rq.op_begin = 0, rq.op_end = (int32_t)p.h.ops.size(), rq.vox0 = 0, rq.nvox = p.g.nvox_total, rq.K = K;
    rq.has_signal = true, rq.signal_ld = p.g.nvox_total, rq.signal_col0 = 0;
    return rq;
}
static StateFacts state(int K, int64_t nvox, bool foreign = false) {
    StateFacts s;
    s.present = true, s.K = K, s.nvox = nvox, s.foreign = foreign;
    return s;
}

static int n_refusals = 0;
static void refuse(const char *what, int code, const std::string &message, const P &p, const RunRequest &rq, const Knobs &kn = defaults()) {
    RunDecision d;
    g_err[0] = 0;
    const int rc = analyse_run(p.h, p.g, rq, kn, &d);
    printf("   %d: %s\n", rc, g_err);
    check(rc == code && message == g_err, what);
    ++n_refusals;
}
static RunDecision accept(const P &p, const RunRequest &rq, const Knobs &kn = defaults()) {
    RunDecision d;
    g_err[0] = 0;
    const int rc = analyse_run(p.h, p.g, rq, kn, &d);
    if (rc) printf("   %d: %s\n", rc, g_err);
    check(rc == EPGX_OK, "  accepted");
    return d;
}
static bool is(const RunDecision &d, RunRoute route, const char *name) { return d.route == route && std::string(name) == d.name; }

#define PRE "epgx_run: "
static const std::string RULE = "derivative states through an exchange (EPGX_OP_X) run on dxrun_kernel<N, K / 64, V>: N = 2 .. 4 compartments with "
                                "N * (K / 64) * (1 + V) <= 8, first order, from equilibrium (in = out = NULL), no D / gather shifts";
static const char *NO_ROOM_X = PRE "range contains an ADC but the signal buffer is NULL or too narrow";
static const char *BAD_K = PRE "K=%d not one of 16, 32, 2048 (state-resident only), 64, 128, 256, 512, 1024";
static std::string bad_k(int K) {
    char buf[256];
    snprintf(buf, sizeof(buf), BAD_K, K);
    return buf;
}

// ------------------------------------------------------------------ refusals of analyse_run
static void test_run_refusals() {
    const P base = plan({T(), S(), ADC()});
    printf("== refusals: the request\n");
    {
        RunRequest rq = request(base, 64);
        rq.op_end = 4;
        refuse("operator range: end", INV, PRE "operator range [0,4) outside [0,3)", base, rq);
        rq.op_begin = 2, rq.op_end = 1;
        refuse("operator range: begin > end", INV, PRE "operator range [2,1) outside [0,3)", base, rq);
        rq = request(base, 64), rq.op_begin = -1;
        refuse("operator range: begin < 0", INV, PRE "operator range [-1,3) outside [0,3)", base, rq);
    }
    {
        P big = base;
        big.g.nvox_total = (int64_t)1 << 40;
        RunRequest rq = request(big, 64);
        rq.nvox = (int64_t)4 * 0x7fffffff + 1;
        refuse("2^33 voxels", UNS, PRE "more than 2^33 voxels in one launch", big, rq);
        rq.nvox = (int64_t)4 * 0x7fffffff, rq.signal_ld = rq.nvox;
        CHECK(accept(big, rq).route == ROUTE_RECORDS);
    }
    {
        RunRequest rq = request(base, 64);
        rq.vox0 = 4;
        refuse("voxel range: past the end", INV, PRE "voxel range [4,12) outside the grid (8 voxels)", base, rq);
        rq.vox0 = -1, rq.nvox = 2;
        refuse("voxel range: vox0 < 0", INV, PRE "voxel range [-1,1) outside the grid (8 voxels)", base, rq);
        rq.vox0 = 0, rq.nvox = -1;
        refuse("voxel range: nvox < 0", INV, PRE "voxel range [0,-1) outside the grid (8 voxels)", base, rq);
    }
    printf("== refusals: states and capacities\n");
    {
        RunRequest rq = request(base, 64);
        rq.in = state(64, 8, true);
        refuse("foreign in", INV, PRE "`in` belongs to another context", base, rq);
        rq.in = state(64, 8), rq.out = state(64, 8, true);
        refuse("foreign out", INV, PRE "`out` belongs to another context", base, rq);
        rq.out = state(128, 8);
        refuse("capacities differ", INV, PRE "in/out capacities differ (64 vs 128)", base, rq);
        rq = request(base, 64), rq.in = state(16, 8);
        refuse("K = 16 with in", UNS, PRE "K = 16 / 32 keep no state in HBM: in and out must be NULL", base, rq);
        rq = request(base, 64), rq.out = state(32, 8);
        refuse("K = 32 with out", UNS, PRE "K = 16 / 32 keep no state in HBM: in and out must be NULL", base, rq);
        refuse("K = 96", UNS, bad_k(96), base, request(base, 96));
        refuse("K = 0", UNS, bad_k(0), base, request(base, 0));
        rq = request(base, 64), rq.in = state(2048, 8);
        refuse("K = 2048 with in", UNS, bad_k(2048), base, rq);
        rq = request(base, 64), rq.out = state(2048, 8);
        refuse("K = 2048 with out", UNS, bad_k(2048), base, rq);
        rq = request(base, 64), rq.in = state(64, 7);
        refuse("in: voxels", INV, PRE "`in` holds 7 voxels, range has 8", base, rq);
        rq = request(base, 64), rq.out = state(64, 9);
        refuse("out: voxels", INV, PRE "`out` holds 9 voxels, range has 8", base, rq);
    }
    printf("== refusals: operators against the capacity\n");
    refuse("shift >= K", INV, PRE "operator 1 shifts by -64, capacity K=64", plan({T(), S(-64), ADC()}), request(base, 64));
    refuse("K = 16: MAT", UNS, PRE "K = 16 / 32 do not handle general matrices (operator 0)", plan({op(EPGX_OP_MAT, 0, 0, 10), S(), ADC()}), request(base, 16));
    refuse("K = 32: MAT0", UNS, PRE "K = 16 / 32 do not handle general matrices (operator 2)", plan({T(), S(), op(EPGX_OP_MAT0, 0, 0, 14)}), request(base, 32));
    refuse("K = 32: D", UNS, PRE "diffusion and gather shifts run with K = 16 or K >= 64 (operator 1)", plan({T(), D(32), ADC()}), request(base, 32));
    refuse("K = 32: GS", UNS, PRE "diffusion and gather shifts run with K = 16 or K >= 64 (operator 0)", plan({GS(32), T(), ADC()}), request(base, 32));
    refuse("D table", INV, PRE "operator 1: D table has 192 doubles per entry, need 3*K=384", plan({T(), D(64), ADC()}), request(base, 128));
    refuse("gather table", INV, PRE "operator 1: gather table has 192 entries, need 3*K=384", plan({T(), GS(64), ADC()}), request(base, 128));
    {
        P p = plan({T(), GS(64), ADC()});
        p.h.gather_tables[1].assign(192, -1);
        p.h.gather_tables[1][0] = 63 | (1 << 30), p.h.gather_tables[1][5] = 0;   // (bit 30 marks a conjugated source; -1: no source)
        CHECK(accept(p, request(p, 64)).route == ROUTE_RECORDS);
        p.h.gather_tables[1][7] = 64;
        refuse("gather index: K", INV, PRE "operator 1: gather index 64 outside [0,64)", p, request(p, 64));
        p.h.gather_tables[1][7] = -2;
        refuse("gather index: negative", INV, PRE "operator 1: gather index -2 outside [0,64)", p, request(p, 64));
    }
    printf("== refusals: exchange\n");
    {
        const P x2 = xplan(2, 8);
        refuse("X at K = 2048", UNS, PRE "ranges with an exchange (EPGX_OP_X) keep the state in HBM: K = 64 .. 1024, not 2048", x2, request(x2, 2048));
        refuse("X at K = 16", UNS, PRE "ranges with an exchange (EPGX_OP_X) keep the state in HBM: K = 64 .. 1024, not 16", x2, request(x2, 16));
        const P x4 = plan({T(), X(2, 2), S(), ADC()});   // blocks of 4 voxels
        RunRequest rq = request(x4, 64);
        rq.vox0 = 2, rq.nvox = 4;
        refuse("group cut: vox0", INV, PRE "voxel range [2,6) cuts compartment groups (blocks of 4 voxels)", x4, rq);
        rq.vox0 = 4, rq.nvox = 2;
        refuse("group cut: nvox", INV, PRE "voxel range [4,6) cuts compartment groups (blocks of 4 voxels)", x4, rq);
        rq = request(x2, 64), rq.has_signal = false;
        refuse("X: no signal", INV, NO_ROOM_X, x2, rq);
        rq = request(x2, 64), rq.signal_col0 = -1;
        refuse("X: signal_col0 < 0", INV, NO_ROOM_X, x2, rq);
        rq = request(x2, 64), rq.signal_col0 = 1;
        refuse("X: signal too narrow", INV, NO_ROOM_X, x2, rq);
        rq = request(x2, 512), rq.has_signal = false;   // (the split path asks too when it meets the ADC in front of what splits the range ...
        CHECK(accept(x2, rq).route == ROUTE_XSPLIT);    //  ... and leaves the probes to its pieces when nothing could fuse to begin with)
        const P xd = xplan(2, 8, 0, {D(64)});
        rq = request(xd, 64), rq.has_signal = false;
        refuse("X, D behind the ADC: no signal", INV, NO_ROOM_X, xd, rq);
    }
    printf("== refusals: exchange with derivative states\n");
    {
        P x = xplan(2, 8, 1);
        x.h.second = true;
        refuse("second order", UNS, PRE "EPGX_DERIV_SECOND: " + RULE, x, request(x, 64));
        x.h.second = false;
        RunRequest rq = request(x, 64);
        rq.in = state(64, 8);
        refuse("in", UNS, PRE "a state in HBM: " + RULE, x, rq);
        rq = request(x, 64), rq.out = state(64, 8);
        refuse("out", UNS, PRE "a state in HBM: " + RULE, x, rq);
        rq = request(x, 64), rq.vox0 = 1, rq.nvox = 2;
        refuse("group cut", INV, PRE "voxel range [1,3) cuts compartment groups (blocks of 2 voxels)", x, rq);
        const P xd = xplan(2, 8, 1, {D(64)}), xg = xplan(2, 8, 1, {GS(64)});
        refuse("D", UNS, PRE "operator 4 (opcode 9): " + RULE, xd, request(xd, 64));
        refuse("GS", UNS, PRE "operator 4 (opcode 10): " + RULE, xg, request(xg, 64));
        rq = request(x, 64), rq.has_signal = false;
        refuse("no signal", INV, NO_ROOM_X, x, rq);
        rq = request(x, 64), rq.signal_ld = 7;
        refuse("signal too narrow", INV, NO_ROOM_X, x, rq);
    }
    printf("== refusals: the signal room of the records route\n");
    {
        RunRequest rq = request(base, 64);
        g_err[0] = 0;
        CHECK(signal_room(rq, false) == EPGX_OK && signal_room(rq, true) == EPGX_OK);
        rq.has_signal = false;
        CHECK(signal_room(rq, false) == INV && std::string(g_err) == PRE "range contains an ADC but signal is NULL");
        rq.has_signal = true, rq.signal_col0 = 2, rq.signal_ld = 9;
        CHECK(signal_room(rq, false) == INV && std::string(g_err) == PRE "signal columns [2,10) exceed signal_ld=9");
        rq.signal_col0 = -1;
        CHECK(signal_room(rq, false) == INV && std::string(g_err) == PRE "signal columns [-1,7) exceed signal_ld=9");
        rq.has_signal = false;   // both at once: the NULL buffer is named
        CHECK(signal_room(rq, false) == INV && std::string(g_err) == PRE "range contains an ADC but signal is NULL");
        n_refusals += 2;
        CHECK(accept(base, rq).route == ROUTE_RECORDS);   // (analyse_run leaves it to the caller, who knows the lists)
    }
}

// ------------------------------------------------------------------ order of the checks
static void test_order() {
    printf("== check order\n");
    const P base = plan({T(), S(), ADC()});
    RunRequest rq = request(base, 64);
    rq.op_end = 9, rq.vox0 = 4;
    refuse("operator range before voxel range", INV, PRE "operator range [0,9) outside [0,3)", base, rq);
    rq = request(base, 64), rq.vox0 = 4, rq.in = state(64, 8, true);
    refuse("voxel range before a foreign in", INV, PRE "voxel range [4,12) outside the grid (8 voxels)", base, rq);
    rq = request(base, 64), rq.in = state(64, 8, true), rq.out = state(128, 8);
    refuse("foreign in before differing capacities", INV, PRE "`in` belongs to another context", base, rq);
    rq = request(base, 64), rq.in = state(64, 8), rq.out = state(128, 8, true);
    refuse("foreign out before differing capacities", INV, PRE "`out` belongs to another context", base, rq);
    rq = request(base, 100), rq.in = state(32, 8);
    refuse("K = 32 with a state before an unsupported K argument", UNS, PRE "K = 16 / 32 keep no state in HBM: in and out must be NULL", base, rq);
    rq = request(base, 64), rq.in = state(32, 8), rq.out = state(100, 8);
    refuse("differing capacities before K = 32 with a state", INV, PRE "in/out capacities differ (32 vs 100)", base, rq);
    rq = request(base, 96), rq.in = state(96, 7);
    refuse("unsupported K before the voxels of in", UNS, bad_k(96), base, rq);
    {
        P p = plan({S(70), GS(64), ADC()});
        p.h.gather_tables[1].assign(192, 99);
        refuse("a shift >= K in front of a bad gather index", INV, PRE "operator 0 shifts by 70, capacity K=64", p, request(p, 64));
        P q = plan({GS(64), S(70), ADC()});
        q.h.gather_tables[0].assign(192, 99);
        refuse("a bad gather index in front of a shift >= K", INV, PRE "operator 0: gather index 99 outside [0,64)", q, request(q, 64));
    }
    {
        const P x = xplan(2, 8, 0, {S(64)});
        RunRequest r = request(x, 64);
        r.vox0 = 1, r.nvox = 2;
        refuse("the operator loop before the exchange checks", INV, PRE "operator 4 shifts by 64, capacity K=64", x, r);
        const P x2 = xplan(2, 8);
        r = request(x2, 64), r.vox0 = 1, r.nvox = 2, r.has_signal = false;
        refuse("the group cut in front of a missing signal", INV, PRE "voxel range [1,3) cuts compartment groups (blocks of 2 voxels)", x2, r);
        r = request(x2, 32), r.vox0 = 1, r.nvox = 2;
        refuse("X: the capacity in front of the group cut", UNS, PRE "ranges with an exchange (EPGX_OP_X) keep the state in HBM: K = 64 .. 1024, not 32", x2, r);
    }
    {
        P x = xplan(2, 8, 1);
        x.h.second = true;
        RunRequest r = request(x, 64);
        r.in = state(64, 8);
        refuse("EPGX_DERIV_SECOND in front of a state in HBM", UNS, PRE "EPGX_DERIV_SECOND: " + RULE, x, r);
        x.h.second = false, r.in = state(256, 8);
        refuse("a state in HBM in front of the register rule", UNS, PRE "a state in HBM: " + RULE, x, r);
        r = request(x, 256), r.vox0 = 1, r.nvox = 2;
        refuse("the register rule in front of the group cut", UNS, PRE "N = 2, K = 256, V = 1: " + RULE, x, r);
        const P xd = xplan(2, 8, 1, {D(64)});
        r = request(xd, 64), r.has_signal = false;
        refuse("a D in front of a missing signal", UNS, PRE "operator 4 (opcode 9): " + RULE, xd, r);
    }
}

// ------------------------------------------------------------------ routes and names
static void test_routes() {
    printf("== routes: nothing to do\n");
    const P base = plan({T(), S(), ADC()});
    {
        RunRequest rq = request(base, 64);
        rq.op_begin = rq.op_end = 1;
        CHECK(is(accept(base, rq), ROUTE_NONE, "none"));
        rq = request(base, 64), rq.nvox = 0, rq.vox0 = 8;
        CHECK(is(accept(base, rq), ROUTE_NONE, "none"));
        const P x = xplan(2, 8);
        rq = request(x, 64), rq.nvox = 0, rq.has_signal = false;
        CHECK(is(accept(x, rq), ROUTE_NONE, "none"));
    }
    printf("== routes: records\n");
    for (int K : {16, 32, 64, 128, 256, 512, 1024, 2048}) {
        const RunDecision d = accept(base, request(base, K));
        printf("   K = %d: packed16 %d, wide %d\n", K, d.packed16, d.wide);
        check(is(d, ROUTE_RECORDS, "") && d.K == K && d.packed16 == (K <= 32) && d.wide == (K == 2048), "  records at K");
    }
    {
        RunRequest rq = request(base, 2048);   // the states override the argument
        rq.in = state(128, 8);
        CHECK(accept(base, rq).K == 128);
        rq.out = state(128, 8);
        CHECK(accept(base, rq).K == 128 && !accept(base, rq).wide);
        rq.in = StateFacts();
        CHECK(accept(base, rq).K == 128);
    }
    printf("== routes: exchange, fused\n");
    struct Fused { int NC, K; int64_t nvox; const char *eq, *from_state; } fused[] = {
        {2, 256, 8, "xrun_kernel<2, 4, false>", "xrun_kernel<2, 4, true>"},
        {3, 128, 6, "xrun_kernel<3, 2, false>", "xrun_kernel<3, 2, true>"},
        {4, 128, 8, "xrun_kernel<4, 2, false>", "xrun_kernel<4, 2, true>"},
        {2, 64, 8, "xrun_kernel<2, 1, false>", "xrun_kernel<2, 1, true>"},
    };
    for (const Fused &f : fused) {
        const P x = xplan(f.NC, f.nvox);
        RunRequest rq = request(x, f.K);
        RunDecision d = accept(x, rq);
        printf("   N = %d, K = %d: %s\n", f.NC, f.K, d.name);
        check(is(d, ROUTE_XRUN, f.eq) && d.NC == f.NC && d.M == f.K / 64 && d.has_adc && d.K == f.K, "  from equilibrium");
        rq.in = state(f.K, f.nvox), rq.out = state(f.K, f.nvox);
        check(is(accept(x, rq), ROUTE_XRUN, f.from_state), "  from a state");
        rq.in = StateFacts();
        check(is(accept(x, rq), ROUTE_XRUN, f.eq), "  into a state");
    }
    printf("== routes: exchange, split\n");
    {
        const char *split = "split<exchange_kernel>";
        const P x3 = xplan(3, 6), x4 = xplan(4, 8), x2 = xplan(2, 8), x5 = xplan(5, 10), x8 = xplan(8, 8);
        CHECK(is(accept(x3, request(x3, 256)), ROUTE_XSPLIT, split));   // N M = 12
        CHECK(is(accept(x4, request(x4, 256)), ROUTE_XSPLIT, split));   // 16
        CHECK(is(accept(x2, request(x2, 512)), ROUTE_XSPLIT, split));   // M = 8
        CHECK(is(accept(x2, request(x2, 1024)), ROUTE_XSPLIT, split));
        CHECK(is(accept(x5, request(x5, 64)), ROUTE_XSPLIT, split));    // N = 5
        CHECK(is(accept(x8, request(x8, 64)), ROUTE_XSPLIT, split));
        const P xd = xplan(2, 8, 0, {D(64)}), xg = xplan(2, 8, 0, {GS(64)});
        CHECK(is(accept(xd, request(xd, 64)), ROUTE_XSPLIT, split));
        CHECK(is(accept(xg, request(xg, 64)), ROUTE_XSPLIT, split));
        Knobs off = defaults();
        off.xrun = false;
        CHECK(is(accept(x2, request(x2, 64), off), ROUTE_XSPLIT, split));
        CHECK(is(accept(x2, request(x2, 64)), ROUTE_XRUN, "xrun_kernel<2, 1, false>"));
    }
    printf("== routes: exchange with derivative states\n");
    struct Fit { int NC, K, V; const char *name; } fits[] = {
        {2, 64, 1, "dxrun_kernel<2, 1, 1>"}, {2, 64, 2, "dxrun_kernel<2, 1, 2>"}, {2, 64, 3, "dxrun_kernel<2, 1, 3>"},
        {2, 128, 1, "dxrun_kernel<2, 2, 1>"}, {3, 64, 1, "dxrun_kernel<3, 1, 1>"}, {4, 64, 1, "dxrun_kernel<4, 1, 1>"},
    };
    for (const Fit &f : fits) {
        const P x = xplan(f.NC, 2 * f.NC, f.V);
        const RunDecision d = accept(x, request(x, f.K));
        printf("   %s\n", d.name);
        check(is(d, ROUTE_DXRUN, f.name) && d.NC == f.NC && d.M == f.K / 64 && d.V == f.V && d.has_adc, "  fits");
    }
    struct Out { int NC, K, V; } outside[] = {{2, 64, 4}, {2, 128, 2}, {2, 256, 1}, {3, 64, 2}, {3, 128, 1}, {4, 64, 2}, {4, 128, 1}, {5, 64, 1}};
    for (const Out &o : outside) {
        const P x = xplan(o.NC, 2 * o.NC, o.V);
        char msg[640];
        snprintf(msg, sizeof(msg), PRE "N = %d, K = %d, V = %d: %s", o.NC, o.K, o.V, RULE.c_str());
        refuse("one step outside the register rule", UNS, std::string(msg).substr(0, sizeof(g_err) - 1), x, request(x, o.K));
    }
    {
        const P x = xplan(2, 8, 1);
        refuse("derivative states at K = 32", UNS, (PRE "N = 2, K = 32, V = 1: " + RULE).substr(0, sizeof(g_err) - 1), x, request(x, 32));
        Knobs off = defaults();
        off.xrun = false;   // (there is no split path for derivatives: the knob does not apply)
        CHECK(is(accept(x, request(x, 64), off), ROUTE_DXRUN, "dxrun_kernel<2, 1, 1>"));
    }
    printf("== naming only: no signal buffer is looked at, everything else is\n");
    {
        const P x = xplan(2, 8), xv = xplan(2, 8, 1);
        RunRequest rq = request(x, 64);
        rq.has_signal = false, rq.signal_ld = 0, rq.naming = true;
        CHECK(is(accept(x, rq), ROUTE_XRUN, "xrun_kernel<2, 1, false>"));
        CHECK(is(accept(xv, rq), ROUTE_DXRUN, "dxrun_kernel<2, 1, 1>"));
        CHECK(signal_room(rq, false) == EPGX_OK && signal_room(rq, true) == EPGX_OK);
        rq.vox0 = 1, rq.nvox = 2;
        refuse("naming: the group cut", INV, PRE "voxel range [1,3) cuts compartment groups (blocks of 2 voxels)", x, rq);
        refuse("naming: the group cut, derivative states", INV, PRE "voxel range [1,3) cuts compartment groups (blocks of 2 voxels)", xv, rq);
        rq = request(base, 96), rq.naming = true;
        refuse("naming: an unsupported K", UNS, bad_k(96), base, rq);
        rq = request(base, 64), rq.naming = true, rq.in = state(64, 8, true);
        refuse("naming: a foreign in", INV, PRE "`in` belongs to another context", base, rq);
    }
}

// ------------------------------------------------------------------ tiled runs
static void refuse_tiled(const char *what, int code, const std::string &message, const char *who, bool deriv, const P &p, int Kbuf,
                         const TiledRequest *rq, int top0 = 0) {
    TiledShape s;
    g_err[0] = 0;
    const int rc = analyse_tiled(who, deriv, p.h, p.g, Kbuf, 8, rq, top0, &s);
    printf("   %d: %s\n", rc, g_err);
    check(rc == code && message == g_err, what);
    ++n_refusals;
}

static void test_tiled() {
    const P base = plan({T(), S(), ADC()}), var1 = plan({T(), S(), ADC()}, 8, 1), var3 = plan({T(), S(), ADC()}, 8, 3);
    TiledRequest whole;
    whole.nvox = 8;
    const char *RUN = "epgx_run_tiled", *DRUN = "epgx_run_tiled_deriv", *INFO = "epgx_tiled_info", *DINFO = "epgx_tiled_deriv_info";
    printf("== tiled refusals: the plan and Kbuf\n");
    refuse_tiled("Kbuf < 64", INV, "epgx_run_tiled: Kbuf=0 is not a multiple of 64 in [64, 2^24]", RUN, false, base, 0, &whole);
    refuse_tiled("Kbuf % 64", INV, "epgx_tiled_info: Kbuf=100 is not a multiple of 64 in [64, 2^24]", INFO, false, base, 100, nullptr);
    refuse_tiled("Kbuf > 2^24", INV, "epgx_run_tiled_deriv: Kbuf=16777280 is not a multiple of 64 in [64, 2^24]", DRUN, true, var1, (1 << 24) + 64, &whole);
    refuse_tiled("plain: derivative plan", UNS, "epgx_run_tiled: plans with derivative states run at K <= 1024 (epgx_run)", RUN, false, var1, 4096, &whole);
    {
        P second = var1;
        second.h.n_vars = 2, second.h.second = true;
        refuse_tiled("deriv: second order", UNS, "epgx_run_tiled_deriv: second-order plans (EPGX_DERIV_SECOND) run at K <= 512 (epgx_run)", DRUN, true, second, 4096, &whole);
    }
    refuse_tiled("deriv: no variables", UNS, "epgx_tiled_deriv_info: the plan has 0 derivative states, a launch carries 1 .. 2", DINFO, true, base, 4096, nullptr);
    refuse_tiled("deriv: three variables", UNS, "epgx_run_tiled_deriv: the plan has 3 derivative states, a launch carries 1 .. 2", DRUN, true, var3, 4096, &whole);
    CHECK(TILED_DERIV_V == 2);
    const std::string nd = ": exchange, gather shifts and diffusion run at K <= 1024 (epgx_run)";
    refuse_tiled("X", UNS, "epgx_run_tiled: operator 1" + nd, RUN, false, xplan(2, 8), 4096, &whole);
    refuse_tiled("GS", UNS, "epgx_tiled_info: operator 3" + nd, INFO, false, plan({T(), S(), ADC(), GS(64)}), 4096, nullptr);
    refuse_tiled("D", UNS, "epgx_run_tiled_deriv: operator 0" + nd, DRUN, true, plan({D(64), T(), ADC()}, 8, 1), 4096, &whole);
    printf("== tiled refusals: the request\n");
    TiledRequest rq = whole;
    rq.vox0 = 1;
    refuse_tiled("voxel range", INV, "epgx_run_tiled: voxel range [1,9) outside the grid (8 voxels)", RUN, false, base, 4096, &rq);
    rq = whole, rq.nvox = -1;
    refuse_tiled("nvox < 0", INV, "epgx_run_tiled_deriv: voxel range [0,-1) outside the grid (8 voxels)", DRUN, true, var1, 4096, &rq);
    rq = whole, rq.slab_voxels = -1;
    refuse_tiled("slab_voxels < 0", INV, "epgx_run_tiled: slab_voxels < 0", RUN, false, base, 4096, &rq);
    rq = whole, rq.in = state(64, 8, true);
    refuse_tiled("foreign in", INV, "epgx_run_tiled: `in` belongs to another context", RUN, false, base, 4096, &rq);
    refuse_tiled("foreign in, deriv", INV, "epgx_run_tiled_deriv: `in` belongs to another context", DRUN, true, var1, 4096, &rq);
    rq.in = state(64, 4);
    refuse_tiled("in: voxels", INV, "epgx_run_tiled: `in` holds 4 voxels, range has 8", RUN, false, base, 4096, &rq);
    rq.in = state(2048, 8);
    refuse_tiled("in: more than 1024 orders", UNS, "epgx_run_tiled: `in` has 2048 orders (at most 1024)", RUN, false, base, 4096, &rq);
    rq.in = state(1024, 8);
    refuse_tiled("in: more than Kbuf", INV, "epgx_run_tiled_deriv: `in` has 1024 orders, Kbuf=512", DRUN, true, var1, 512, &rq);
    refuse_tiled("top0 < 0", INV, "epgx_tiled_info: top0=-1 outside [0, Kbuf)", INFO, false, base, 4096, nullptr, -1);
    refuse_tiled("top0 = Kbuf", INV, "epgx_tiled_deriv_info: top0=4096 outside [0, Kbuf)", DINFO, true, var1, 4096, nullptr, 4096);
    printf("== tiled: order of the checks\n");
    rq = whole, rq.vox0 = 1, rq.slab_voxels = -1;
    refuse_tiled("Kbuf before the voxel range", INV, "epgx_run_tiled: Kbuf=32 is not a multiple of 64 in [64, 2^24]", RUN, false, base, 32, &rq);
    refuse_tiled("the plan before the voxel range", UNS, "epgx_run_tiled: plans with derivative states run at K <= 1024 (epgx_run)", RUN, false, var1, 4096, &rq);
    refuse_tiled("the voxel range before slab_voxels", INV, "epgx_run_tiled: voxel range [1,9) outside the grid (8 voxels)", RUN, false, base, 4096, &rq);
    rq = whole, rq.slab_voxels = -1, rq.in = state(64, 8, true);
    refuse_tiled("slab_voxels before a foreign in", INV, "epgx_run_tiled: slab_voxels < 0", RUN, false, base, 4096, &rq);
    rq = whole, rq.in = state(2048, 4, true);
    refuse_tiled("a foreign in before its voxels", INV, "epgx_run_tiled: `in` belongs to another context", RUN, false, base, 4096, &rq);
    rq.in = state(2048, 4);
    refuse_tiled("the voxels of in before its orders", INV, "epgx_run_tiled: `in` holds 4 voxels, range has 8", RUN, false, base, 4096, &rq);
    rq.in = state(2048, 8);
    refuse_tiled("1024 orders before Kbuf", UNS, "epgx_run_tiled: `in` has 2048 orders (at most 1024)", RUN, false, base, 512, &rq);
    printf("   %d refusals\n", n_refusals);

    printf("== tiled: M, H and top0\n");
    TiledShape s;
    CHECK(analyse_tiled(RUN, false, base.h, base.g, 4096, 8, &whole, 0, &s) == EPGX_OK && s.M == 8 && s.H == 32 && s.top0 == 0);
    CHECK(analyse_tiled(RUN, false, base.h, base.g, 4096, 16, &whole, 0, &s) == EPGX_OK && s.M == 16 && s.H == 64);
    CHECK(analyse_tiled(RUN, false, base.h, base.g, 4096, 12, &whole, 0, &s) == EPGX_OK && s.M == 8 && s.H == 32);   // (anything but 16)
    CHECK(analyse_tiled(DRUN, true, var1.h, var1.g, 4096, 16, &whole, 0, &s) == EPGX_OK && s.M == 8 && s.H == 32);   // derivative plans: 8 only
    CHECK(analyse_tiled(DINFO, true, var1.h, var1.g, 4096, 8, nullptr, 77, &s) == EPGX_OK && s.M == 8 && s.H == 32 && s.top0 == 77);
    CHECK(analyse_tiled(INFO, false, base.h, base.g, 64, 16, nullptr, 63, &s) == EPGX_OK && s.M == 16 && s.top0 == 63);
    rq = whole, rq.in = state(1024, 8), rq.slab_voxels = 3;
    CHECK(analyse_tiled(RUN, false, base.h, base.g, 1024, 8, &rq, 5, &s) == EPGX_OK && s.top0 == 1023);   // (a run takes top0 from `in`)
    rq = whole, rq.nvox = 0, rq.vox0 = 8;
    CHECK(analyse_tiled(RUN, false, base.h, base.g, 1 << 24, 8, &rq, 0, &s) == EPGX_OK && s.top0 == 0);
}

static void test_slabs() {
    printf("== slab_voxels\n");
    const int64_t two_legs = 3 * 512 * 16 + 8;   // bytes per voxel of the two-leg launch at 2048 orders
    CHECK(slab_voxels(1, two_legs, 0, 0) == 4);
    CHECK(slab_voxels(10, two_legs, 0, 0) == 12);   // rounded up to four ...
    CHECK(slab_voxels(8, two_legs, 0, 0) == 8);
    CHECK(slab_voxels(1 << 20, two_legs, 0, 0) == ((((int64_t)8 << 30) / two_legs) & ~(int64_t)3));   // ... or what 8 GiB hold, rounded down
    CHECK(slab_voxels(1 << 20, two_legs, 0, 0) == 349408);
    CHECK(slab_voxels(1 << 20, ((int64_t)2 << 30) + 16, 0, 0) == 4);   // more than 2 GiB per voxel: fewer than four fit, four it is
    CHECK(slab_voxels(1 << 20, (int64_t)2 << 30, 0, 0) == 4);
    CHECK(slab_voxels(1 << 20, ((int64_t)1 << 30) - 8, 0, 0) == 8);
    CHECK(slab_voxels(100, two_legs, 5, 0) == 8);      // the knob is rounded up to four
    CHECK(slab_voxels(100, two_legs, 8, 0) == 8);
    CHECK(slab_voxels(6, two_legs, 64, 0) == 8);       // ... and only ever lowers
    CHECK(slab_voxels(100, two_legs, -3, 0) == 100);
    CHECK(slab_voxels(100, two_legs, 0, 3) == 3);      // the request of a tiled call is taken as it is
    CHECK(slab_voxels(100, two_legs, 8, 3) == 3);      // a request below the knob wins
    CHECK(slab_voxels(100, two_legs, 8, 50) == 8);     // ... one above it does not
    CHECK(slab_voxels(10, two_legs, 0, 11) == 11 && slab_voxels(10, two_legs, 0, 13) == 12);
}

int main() {
    CHECK(supported_K(64) && supported_K(1024) && !supported_K(32) && !supported_K(2048) && !supported_K(192));
    test_run_refusals();
    test_order();
    test_routes();
    test_tiled();
    test_slabs();
    printf("run_check: all checks passed\n");
    return 0;
}

// plan_check.cpp -- plan analysis (epgpy_amd/csrc/epgx_plan_check.cpp) on a machine without a GPU.
//
// Builds epgx_plan_desc / epgx_plan_ext by hand from two small valid plans over a 2 x 2 grid, applies one mutation per case and
// runs the C++ that ships: every refusal with its code and message, the order of the checks, the geometry, the zero patterns and
// snaps of rotation, relaxation and partial tables, the recipes and the layout of the log tables.  One line per check; exits
// non-zero at the first failure.  `make plan_check` builds it, `make asan` with the address / undefined-behaviour sanitizers
// (tests/test_plan_check_host.py runs the plain build).
//
// Refusals this program cannot reach: none of the unit's own ("epgx_plan_create: host allocation failed" and the HIP errors
// belong to epgx_api.hip).  Inside operator_patterns the arm "a table in the generated part that is not an EPGX_OP_T0" shares its
// message with the reachable arm (no entry of `fuse`); check_operator refuses such an operator first.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_plan_check.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) exit(1);
}
#define CHECK(cond) check((cond), #cond)

static Knobs defaults() {   // the values knobs() takes with an empty environment
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1};
    return k;
}

// ------------------------------------------------------------------ plans
static const int NOTRUNC = 1 << 20;
typedef std::vector<double> Row;
// table entries (layouts: include/epgx.h)
static const Row T_X = {0.9, 0.3, 0, 0, 0.1, 0, -0.1, 0.8};            // Im m01 = Re m02 = Re m20 = 0, exactly
static const Row T_XR = {0.9, 0.3, 1.2e-16, 1.2e-16, 0.1, 1.2e-16, -0.1, 0.8};   // ... through residues of sin(pi)
static const Row T_YR = {0.5, 0.6, 6e-17, 0.3, 6e-17, 0.3, 6e-17, 0.7};          // Im m01 = Im m02 = Im m20 = residues of cos(pi/2)
static const Row T_GEN = {0.5, 0.6, 0.1, 0.3, 0.2, 0.3, 0.2, 0.7};
static const Row E_REAL = {0.9, 0, 0.95, 0.05};
static const Row E_PREC = {0.9, 0.1, 0.95, 0.05};
static const Row DT_X = {0.1, 0, 0.2, 0, 0, 0.3, 0, 0.4, 0.5, 0};       // ur ui pr pi qr qi tr ti c22 pad: ui = pi = qr = tr = 0
static const Row DT_XR = {0.1, 1e-17, 0.2, 1e-17, 1e-17, 0.3, 1e-17, 0.4, 0.5, 0};
static const Row DT_YR = {0.1, 1e-17, 0.2, 1e-17, 0.3, 1e-17, 0.4, 1e-17, 0.5, 0};   // all Im = residues
static const Row DT_GEN = {0.1, 0.2, 0.2, 0.1, 0.3, 0.3, 0.4, 0.4, 0.5, 0};
static const Row DE_REAL = {-0.1, 0, -0.2, 0.2};
static const Row DE_PREC = {-0.1, 0.3, -0.2, 0.2};

struct Plan {
    std::vector<int64_t> shape = {2, 2};
    std::vector<int64_t> strides;   // [n_spaces][EPGX_MAX_DIMS]
    std::vector<double> coef;
    std::vector<epgx_op> ops;
    std::vector<epgx_dop> dops;
    std::vector<epgx_fuse> fuse;
    std::vector<epgx_fuse_partial> fpart;
    std::vector<epgx_assemble> assemble;
    std::vector<epgx_chain> chains;
    std::vector<std::vector<epgx_chain_step>> steps;
    int n_adc = 0, n_vars = 0, flags = 0;
    int64_t n_gen = 0;
    epgx_plan_desc d;
    epgx_plan_ext x;

    void space(std::initializer_list<int64_t> st) {
        size_t at = strides.size();
        strides.resize(at + EPGX_MAX_DIMS, 0);
        for (int64_t s : st) strides[at++] = s;
    }
    int64_t table(const Row &entry, int64_t entries = 1) {
        const int64_t off = (int64_t)coef.size();
        for (int64_t j = 0; j < entries; ++j) coef.insert(coef.end(), entry.begin(), entry.end());
        return off;
    }
    int op(int opcode, int space, int ia, int ib, int64_t off, int ncoef) {
        epgx_op o;
        memset(&o, 0, sizeof(o));
        o.opcode = opcode, o.space = space, o.ia = ia, o.ib = ib, o.coef_off = off, o.ncoef = ncoef;
        ops.push_back(o);
        return (int)ops.size() - 1;
    }
    int T(int64_t off, int space = -1) { return op(EPGX_OP_T, space, 0, 0, off, 8); }
    int T0(int64_t off, int space = -1) { return op(EPGX_OP_T0, space, 0, 0, off, 12); }
    int E(int64_t off, int space = 0) { return op(EPGX_OP_E, space, 0, 0, off, 4); }
    int S(int n = 1) { return op(EPGX_OP_S, -1, n, NOTRUNC, 0, 0); }
    int ADC(int slot) { n_adc = slot + 1 + n_vars > n_adc ? slot + 1 + n_vars : n_adc; return op(EPGX_OP_ADC, -1, slot, 0, 0, 0); }
    // partial of operator i w.r.t. variable v (dops grows with the operator list)
    void fit_dops() {
        epgx_dop none;
        memset(&none, 0, sizeof(none));
        for (int k = 0; k < EPGX_MAX_VARS; ++k) none.coef_off[k] = none.space[k] = -1;
        dops.resize(ops.size(), none);
    }
    void partial(int i, int v, int64_t off, int space) {
        fit_dops();
        dops[(size_t)i].coef_off[v] = off;
        dops[(size_t)i].space[v] = space;
    }
    epgx_plan_desc *desc() {
        fit_dops();
        memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.n_ops = (int)ops.size(), d.ops = ops.data();
        d.ndim = (int)shape.size(), d.grid_shape = shape.data();
        d.n_spaces = (int)(strides.size() / EPGX_MAX_DIMS), d.space_strides = strides.data();
        d.n_coef = (int64_t)coef.size(), d.coef = coef.data();
        d.n_adc = n_adc, d.n_vars = n_vars, d.dops = n_vars > 0 ? dops.data() : nullptr, d.deriv_flags = flags;
        d.n_fuse = (int)fuse.size(), d.fuse = fuse.data(), d.n_coef_generated = n_gen;
        d.n_assemble = (int)assemble.size(), d.assemble = assemble.data();
        d.n_fuse_partial = (int)fpart.size(), d.fuse_partial = fpart.data();
        memset(&x, 0, sizeof(x));
        x.struct_size = sizeof(x);
        for (size_t i = 0; i < chains.size(); ++i) chains[i].steps = steps[i].data(), chains[i].n_steps = (int)steps[i].size();
        x.n_chain = (int)chains.size(), x.chain = chains.data();
        return &d;
    }
    const epgx_plan_ext *ext() const { return chains.empty() ? nullptr : &x; }
};

static epgx_fuse fuse_of(int64_t dst, int dst_space, int64_t src, int src_space, int src_ncoef, int64_t e, int e_space, int after = 1) {
    epgx_fuse f;
    memset(&f, 0, sizeof(f));
    f.dst_off = dst, f.src_off = src, f.e_off = e, f.dst_space = dst_space, f.src_space = src_space, f.e_space = e_space;
    f.src_ncoef = src_ncoef, f.after = after;
    return f;
}
static epgx_fuse_partial fpart_of(int64_t dst, int dst_space, int64_t src, int src_space, int src_ncoef, int64_t dsrc, int dsrc_space, int dsrc_ncoef,
                                  int64_t e, int e_space, int64_t de, int de_space, int after = 1) {
    epgx_fuse_partial f;
    memset(&f, 0, sizeof(f));
    f.dst_off = dst, f.src_off = src, f.dsrc_off = dsrc, f.e_off = e, f.de_off = de;
    f.dst_space = dst_space, f.src_space = src_space, f.dsrc_space = dsrc_space, f.e_space = e_space, f.de_space = de_space;
    f.src_ncoef = src_ncoef, f.dsrc_ncoef = dsrc_ncoef, f.after = after;
    return f;
}

// T | E S ADC over 2 x 2 voxels: a rotation for all voxels, a relaxation per voxel (space 0); space 1 varies along axis 0 only
struct Base : Plan {
    int64_t tT, tE;
    Base() {
        space({2, 1});
        space({1, 0});
        tT = table(T_X);
        tE = table(E_REAL, 4);
        T(tT), E(tE), S(), ADC(0);
    }
};

// the same with one variable and every kind of recipe: an assembled relaxation table A, a fused echo F = E . T with its partial
// FP, a collapsed table C;  T E S ADC | T0(F) E(A) MAT0(C) ADC
struct Full : Base {
    int64_t tdT, tdE, cols0, cols1, A, F, FP, C;
    int iT0;
    Full() {
        n_vars = 1;
        ops[3].ia = 0, n_adc = 2;
        tdT = table(DT_X);
        tdE = table(DE_REAL, 4);
        cols0 = table({0.9, 0}, 2);
        cols1 = table({0.95, 0.05}, 2);
        A = (int64_t)coef.size(), F = A + 16, FP = F + 48, C = FP + 56, n_gen = 16 + 48 + 56 + 56;
        iT0 = T0(F, 0), E(A, 0), op(EPGX_OP_MAT0, 0, 0, 0, C, 14), ADC(2);
        partial(0, 0, tdT, -1), partial(1, 0, tdE, 0), partial(iT0, 0, FP, 0);
        epgx_assemble as;
        memset(&as, 0, sizeof(as));
        as.dst_off = A, as.dst_space = 0, as.ncoef = 4, as.n_src = 2;
        as.src[0].off = cols0, as.src[0].ncol = 2, as.src[0].strides[0] = 1;
        as.src[1].off = cols1, as.src[1].ncol = 2, as.src[1].strides[1] = 1;
        const uint8_t cs[4] = {0, 0, 1, 1}, ci[4] = {0, 1, 0, 1};
        memcpy(as.col_src, cs, 4), memcpy(as.col_idx, ci, 4);
        assemble.push_back(as);
        fuse.push_back(fuse_of(F, 0, tT, -1, 8, tE, 0));
        fpart.push_back(fpart_of(FP, 0, tT, -1, 8, tdT, -1, 10, tE, 0, tdE, 0));
        epgx_chain ch;
        memset(&ch, 0, sizeof(ch));
        ch.dst_off = C, ch.dst_space = 0;
        chains.push_back(ch);
        epgx_chain_step s0 = {tT, 0, EPGX_OP_T, -1, 1, 2}, s1 = {tE, 0, EPGX_OP_E, 0, 0, 0};
        steps.push_back({s0, s1});
    }
};

template <class P> static int analyse(P &p, PlanAnalysis &a, const Knobs &kn = defaults()) {
    epgx_plan_desc *d = p.desc();
    return analyse_plan(d, p.ext(), kn, &a);
}

// ------------------------------------------------------------------ refusals
static int n_refusals = 0;
template <class P> static void refuse(const char *what, int code, const std::string &message, const std::function<void(P &)> &mutate,
                                      const std::function<void(epgx_plan_desc &)> &mutate_desc = nullptr) {
    P p;
    if (mutate) mutate(p);
    epgx_plan_desc *d = p.desc();
    if (mutate_desc) mutate_desc(*d);
    PlanAnalysis a;
    g_err[0] = 0;
    const int rc = analyse_plan(d, p.ext(), defaults(), &a);
    printf("   %d: %s\n", rc, g_err);
    check(rc == code && message == g_err, what);
    ++n_refusals;
}
#define PRE "epgx_plan_create: "
static void refuse_desc(const char *what, int code, const char *message, const std::function<void(epgx_plan_desc &)> &m) { refuse<Base>(what, code, message, nullptr, m); }
static void refuse_base(const char *what, const char *message, const std::function<void(Base &)> &m) { refuse<Base>(what, EPGX_ERR_INVALID, message, m); }
static void refuse_full(const char *what, const char *message, const std::function<void(Full &)> &m, int code = EPGX_ERR_INVALID) { refuse<Full>(what, code, message, m); }

static void test_refusals() {
    printf("== the base plans are accepted\n");
    {
        Base b;
        Full f;
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(analyse(f, a) == EPGX_OK);
    }
    printf("== refusals: the descriptor\n");
    const int INV = EPGX_ERR_INVALID, UNS = EPGX_ERR_UNSUPPORTED;
    refuse_desc("no operators", INV, PRE "empty operator list", [](epgx_plan_desc &d) { d.n_ops = 0; });
    refuse_desc("ndim", INV, PRE "ndim 9 not in [1,8]", [](epgx_plan_desc &d) { d.ndim = 9; });
    refuse_desc("n_spaces", UNS, PRE "5 index spaces, at most 4 supported", [](epgx_plan_desc &d) { d.n_spaces = 5; });
    refuse_desc("pool", INV, PRE "bad coefficient pool", [](epgx_plan_desc &d) { d.coef = nullptr; });
    refuse_desc("generated", INV, PRE "bad generated-table description", [](epgx_plan_desc &d) { d.n_fuse = -1; });
    refuse_desc("4 GiB", UNS, PRE "coefficient pool larger than 4 GiB (split the grid)", [](epgx_plan_desc &d) { d.n_coef_generated = (int64_t)1 << 29; });
    refuse_desc("n_adc", INV, PRE "n_adc < 0", [](epgx_plan_desc &d) { d.n_adc = -1; });
    refuse_desc("second: n_vars", INV, PRE "EPGX_DERIV_SECOND needs n_vars = 3 (S_a, S_b, H_ab) or 2 (S_a, H_aa), got 1",
                [](epgx_plan_desc &d) { d.deriv_flags = EPGX_DERIV_SECOND, d.n_vars = 1; });
    refuse_desc("second: dops", INV, PRE "EPGX_DERIV_SECOND without dops", [](epgx_plan_desc &d) { d.deriv_flags = EPGX_DERIV_SECOND, d.n_vars = 2; });
    const char *second_fold = PRE "EPGX_DERIV_SECOND without EPGX_PLAN_NO_FOLD: the run-time fold implements the first-order product rule only";
    refuse_full("second: fold", second_fold, [](Full &p) { p.flags = EPGX_DERIV_SECOND, p.n_vars = 2; }, UNS);
    refuse_full("second: fuse", PRE "EPGX_DERIV_SECOND with device-generated tables (n_fuse, n_fuse_partial): epgx_fuse_partial implements the first-order product rule only",
                [](Full &p) { p.flags = EPGX_DERIV_SECOND | EPGX_PLAN_NO_FOLD, p.n_vars = 2; }, UNS);
    refuse_full("second: chains", PRE "EPGX_DERIV_SECOND with chains: a collapsed run of operators has no second-order partials",
                [](Full &p) { p.flags = EPGX_DERIV_SECOND | EPGX_PLAN_NO_FOLD, p.n_vars = 2, p.fuse.clear(), p.fpart.clear(); }, UNS);

    printf("== refusals: the grid\n");
    refuse_base("shape", PRE "grid_shape[1] < 1", [](Base &p) { p.shape[1] = 0; });
    refuse<Base>("2^40 voxels", UNS, PRE "grid too large", [](Base &p) { p.shape = {(int64_t)1 << 21, (int64_t)1 << 20}; });
    refuse_base("negative stride", PRE "negative stride in space 1", [](Base &p) { p.strides[EPGX_MAX_DIMS] = -1; });
    refuse<Base>("2^31 entries", UNS, PRE "table of space 1 too large", [](Base &p) { p.strides[EPGX_MAX_DIMS] = (int64_t)1 << 31; });

    printf("== refusals: assembled tables\n");
#define ASM(what, why, body) refuse_full(what, PRE "assembled table 0: " why, [](Full &p) { epgx_assemble &as = p.assemble[0]; body; })
    ASM("space", "index space out of range", as.dst_space = 2);
    ASM("columns", "bad column / source count", as.ncoef = 17);
    ASM("destination", "destination outside the generated part of the pool", as.dst_off = 0);
    ASM("negative", "negative source stride", as.src[1].strides[0] = -1);
    ASM("varies", "a source varies along an axis the destination does not", as.dst_space = 1);
    ASM("source", "source columns outside the host part of the pool", as.src[1].off = p.A - 2);
    ASM("column", "column refers to a missing source column", as.col_idx[3] = 2);

    printf("== refusals: collapsed tables\n");
#define CHAIN(what, why, body) refuse_full(what, PRE "collapsed table 0: " why, [](Full &p) { epgx_chain &ch = p.chains[0]; std::vector<epgx_chain_step> &st = p.steps[0]; (void)ch, (void)st; body; })
    CHAIN("space", "index space of the destination out of range", ch.dst_space = -2);
    CHAIN("steps", "no steps", st.clear());
    CHAIN("destination", "destination outside the generated part of the pool", ch.dst_off = p.C + 1);
    CHAIN("group", "malformed group (1 .. EPGX_CHAIN_GROUP steps inside the list, count >= 1)", st[0].group = 3);
    CHAIN("kind", "unknown kind of source (EPGX_OP_T, EPGX_OP_MAT, EPGX_OP_MAT0 or EPGX_OP_E)", st[1].kind = EPGX_OP_S);
    CHAIN("source space", "index space of a source out of range", st[1].space = 7);
    CHAIN("negative", "negative source offset or stride", st[0].stride = -8);
    CHAIN("source", "source neither inside the host part of the pool nor an assembled table", (st[0].stride = 8, st[0].count = 1000));
    CHAIN("varies", "a source varies along an axis the destination does not", ch.dst_space = 1);

    printf("== refusals: operators\n");
#define OP(what, i, opcode, why, body) refuse_full(what, PRE "operator " #i " (opcode " #opcode "): " why, [](Full &p) { epgx_op &op = p.ops[i]; body; })
    OP("opcode", 0, 99, "unknown opcode", op.opcode = 99);
    OP("ncoef", 0, 1, "wrong ncoef for opcode", op.ncoef = 9);
    OP("no table", 2, 9, "table-driven operator without a table", op.opcode = EPGX_OP_D);
    OP("space", 1, 3, "index space out of range", op.space = 2);
    OP("pool", 1, 3, "coefficient table exceeds the pool", op.coef_off = p.C + 56);
    OP("recipe", 0, 1, "a table in the generated part of the pool needs a recipe (epgx_assemble, epgx_chain for EPGX_OP_MAT0, or epgx_fuse for EPGX_OP_T0)", op.coef_off = p.F);
    OP("shift 0", 2, 4, "shift by 0", op.ia = 0);
    OP("shift K", 2, 4, "shift exceeds EPGX_MAX_K", op.ia = -EPGX_MAX_K);
    OP("truncation", 2, 4, "negative truncation order", (op.ia = 0, op.ib = -1));   // (the last failing check of the block names it)
    OP("ADC slot", 3, 5, "ADC slot out of range", op.ia = 4);
    OP("ADC probe", 3, 5, "unknown ADC probe", (op.ia = 4, op.ib = 2));
    const int64_t x2 = 12;   // 3 N^2 doubles
#define XOP(what, why, body) refuse_base(what, PRE "operator 4 (opcode 13): " why, [](Base &p) { const int64_t off = p.table(Row(x2, 0.0)); p.op(EPGX_OP_X, -1, 2, 1, off, (int)x2); epgx_op &op = p.ops[4]; body; })
    XOP("X: N", "exchange between 2 .. 8 compartments", op.ia = 9);
    XOP("X: table", "X table needs 3 N^2 doubles per entry", op.ncoef = 11);
    XOP("X: axis", "no grid axis of extent N = ia with ib voxels behind it", op.ib = 3);
    refuse_base("X: two spans", PRE "operator 5 (opcode 13): X operators of one plan must share N and the compartment axis", [](Base &p) {
        const int64_t off = p.table(Row(x2, 0.0));
        p.op(EPGX_OP_X, -1, 2, 1, off, (int)x2), p.op(EPGX_OP_X, -1, 2, 2, off, (int)x2);
    });

    printf("== refusals: derivatives\n");
    refuse_desc("n_vars", INV, PRE "n_vars=4 (at most 3) or dops missing", [](epgx_plan_desc &d) { d.n_vars = 4; });
    auto second = [](Plan &p) { p.flags = EPGX_DERIV_SECOND | EPGX_PLAN_NO_FOLD, p.n_vars = 2, p.n_adc = 3; };
    refuse<Base>("second: T0", UNS, PRE "EPGX_DERIV_SECOND with an EPGX_OP_T0 operator: the constant term of a fused table has no second-order partial",
                 [&](Base &p) { second(p), p.T0(p.table(Row(12, 0.0))); });
    refuse<Base>("second: X", UNS, PRE "EPGX_DERIV_SECOND with exchange (EPGX_OP_X)", [&](Base &p) { second(p), p.op(EPGX_OP_X, -1, 2, 1, p.table(Row(x2, 0.0)), (int)x2); });
    refuse<Base>("second: cross term", INV, PRE "EPGX_DERIV_SECOND: a cross-term bit (epgx_dop::reserved) without its first-order partial",
                 [&](Base &p) { second(p), p.partial(1, 0, -1, -1), p.dops[1].reserved = EPGX_HESS_CROSS_A; });
#define DOP(what, i, why, body) refuse_full(what, PRE "operator " #i ", variable 0: " why, [](Full &p) { epgx_dop &dp = p.dops[i]; body; })
    refuse_full("beyond n_vars", PRE "operator 0, variable 1: partial for a variable beyond n_vars", [](Full &p) { p.dops[0].coef_off[1] = p.tdT, p.dops[0].space[1] = -1; });
    DOP("carrier", 2, "only T / MAT / E operators can carry partial derivatives", dp.coef_off[0] = p.tdT);
    DOP("space", 1, "index space of a partial out of range", dp.space[0] = 2);
    DOP("generated", 4, "generated partial table exceeds the pool", dp.coef_off[0] = p.C + 1);
    DOP("host part", 1, "partial table exceeds the host part of the pool", dp.coef_off[0] = p.A - 15);
    refuse_full("ADC rows", PRE "operator 7: ADC rows [2,3] exceed n_adc=3", [](Full &p) { p.n_adc = 3; });

    printf("== refusals: generated tables\n");
#define FUSE(what, why, body) refuse_full(what, PRE "generated table 0: " why, [](Full &p) { epgx_fuse &fu = p.fuse[0]; (void)fu; body; })
    FUSE("space", "index space out of range", fu.e_space = 2);
    FUSE("ncoef", "source must have 8 or 12 coefficients", fu.src_ncoef = 10);
    FUSE("destination", "destination outside the generated part of the pool", fu.dst_off = p.tT);
    FUSE("E source", "E source neither in the host part of the pool nor an assembled table", fu.e_off = p.A - 15);
    FUSE("rotation source", "rotation source outside the pool", fu.src_off = -1);
    FUSE("generated source", "a generated source must be the destination of an earlier entry", (fu.src_off = p.FP, fu.src_ncoef = 12));
    FUSE("varies", "a source varies along an axis the destination does not", fu.dst_space = 1);
    FUSE("precession", "E source has a precession term (Im e0 != 0)", p.coef[(size_t)p.tE + 9] = 0.1);
    refuse_desc("n_fuse_partial", INV, PRE "n_fuse_partial=1 without a list or without variables", [](epgx_plan_desc &d) { d.n_fuse_partial = 1; });
#define FPART(what, why, body) refuse_full(what, PRE "generated partial 0: " why, [](Full &p) { epgx_fuse_partial &fp = p.fpart[0]; (void)fp; body; })
    FPART("space", "index space out of range", fp.de_space = 2);
    FPART("no partial", "neither the rotation nor the relaxation has a partial", (fp.dsrc_off = -1, fp.de_off = -1));
    FPART("ncoef", "rotation source must have 8 or 12 coefficients", fp.src_ncoef = 9);
    FPART("partial ncoef", "rotation partial must have 10 or 14 coefficients", fp.dsrc_ncoef = 12);
    FPART("destination", "destination outside the generated part of the pool", fp.dst_off = p.C + 1);
    FPART("rotation source", "rotation source outside the pool", fp.src_off = p.C + 56);
    FPART("generated source", "a generated rotation source must be the destination of an entry of `fuse`", (fp.src_off = p.A, fp.src_ncoef = 12));
    FPART("E source", "E source neither in the host part of the pool nor an assembled table", fp.e_off = -4);
    FPART("precession", "E source has a precession term (Im e0 != 0)", (fp.e_off = p.tdE, p.coef[(size_t)p.tdE + 1] = 0.1));
    FPART("rotation partial", "rotation partial: 10 per entry in the host part of the pool, or 14 per entry written by an earlier entry", fp.dsrc_off = p.A - 9);
    FPART("E partial", "E partial outside the host part of the pool (and not an assembled table)", fp.de_off = p.A - 15);
    FPART("E partial precession", "E partial has a precession term (Im d e0 != 0)", p.coef[(size_t)p.tdE + 5] = 0.3);
    FPART("varies", "a source varies along an axis the destination does not", (fp.dst_space = 1, p.fuse[0].dst_space = 1, p.fuse[0].e_space = 1, fp.e_space = 1));

    printf("== refusals: behind the scan\n");
    refuse_full("no fuse entry", PRE "operator 4 refers to the generated part of the pool but no entry of `fuse` writes there",
                [](Full &p) { p.fuse[0].dst_off = p.C + 56, p.n_gen += 48, p.fpart[0].src_off = p.tT; });
    refuse_full("no fuse_partial entry", PRE "operator 4, variable 0: the partial refers to the generated part of the pool but no entry of `fuse_partial` writes there",
                [](Full &p) { p.fpart[0].dst_off = p.C + 56, p.n_gen += 56; });
    refuse<Base>("gather shift", UNS, PRE "operator 4: gather shifts must be the same for all voxels", [](Base &p) { p.op(EPGX_OP_GS, 0, 0, 0, 0, 2); });
    printf("   %d refusals\n", n_refusals);

    printf("== check order\n");
    refuse_full("second-order block before a bad operator", second_fold, [](Full &p) { p.flags = EPGX_DERIV_SECOND, p.n_vars = 2, p.ops[0].opcode = 99; }, UNS);
    refuse_full("assemble recipe before a bad operator", PRE "assembled table 0: bad column / source count", [](Full &p) { p.assemble[0].n_src = 0, p.ops[0].opcode = 99; });
    refuse_full("operators before n_vars", PRE "operator 0 (opcode 99): unknown opcode", [](Full &p) { p.n_vars = 4, p.ops[0].opcode = 99; });
    refuse_full("operators before n_fuse_partial", PRE "operator 0 (opcode 99): unknown opcode", [](Full &p) { p.ops[0].opcode = 99; }, EPGX_ERR_INVALID);
}

// ------------------------------------------------------------------ geometry
static void test_geometry() {
    printf("== geometry\n");
    {
        Base b;
        b.shape = {3, 1, 2};
        b.strides.clear();
        b.space({2, 777, 1});   // dense: the stride of the axis of extent 1 is irrelevant
        b.space({1, 0, 0});
        b.space({4, 0, 2});     // every entry of its own, but not in C order
        b.coef.resize(64, 0.0);
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(a.geo.ndim == 3 && a.geo.nvox_total == 6 && a.geo.shape[0] == 3 && a.geo.shape[1] == 1 && a.geo.shape[2] == 2 && a.geo.shape[7] == 1);
        CHECK(a.geo.space_extent[0] == 5 && a.geo.space_extent[1] == 2 && a.geo.space_extent[2] == 10);
        CHECK(a.geo.entries(0) == 6 && a.geo.entries(1) == 3 && a.geo.entries(-1) == 1);
        CHECK(a.geo.stride(2, 0) == 4 && a.geo.stride(-1, 0) == 0);
        CHECK(a.geo.dense_spaces == 1u);
        CHECK(a.geo.x_span == 0 && a.geo.x_ncomp == 0);
        CHECK(a.host.n_spaces == 3 && a.host.n_pool == 64 && a.host.fold && !a.host.second && a.host.n_vars == 0);
    }
    {   // the limits themselves pass: 2^31 - 1 as the largest index of an (unused) space, 2^40 voxels
        Base b;
        b.strides[EPGX_MAX_DIMS] = ((int64_t)1 << 31) - 1;
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK && a.geo.space_extent[1] == ((int64_t)1 << 31) - 1);
        Plan p;
        p.shape = {(int64_t)1 << 20, (int64_t)1 << 20};
        p.T(p.table(T_X)), p.S(), p.ADC(0);
        CHECK(analyse(p, a) == EPGX_OK && a.geo.nvox_total == (int64_t)1 << 40);
    }
    {   // exchange: N = 2 compartments along axis 0, 2 voxels behind it
        Base b;
        const int64_t off = b.table(Row(12, 0.0));
        b.op(EPGX_OP_X, -1, 2, 2, off, 12), b.op(EPGX_OP_X, -1, 2, 2, off, 12);
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(a.geo.x_span == 4 && a.geo.x_ncomp == 2);
        b.ops[4].ib = b.ops[5].ib = 1;   // along axis 1
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(a.geo.x_span == 2 && a.geo.x_ncomp == 2);
    }
}

// ------------------------------------------------------------------ zero patterns of rotation tables
static bool same_snap(const Snap &s, int64_t off, int64_t entries, int nc, uint32_t mask) {
    return s.off == off && s.entries == entries && s.nc == nc && s.mask == mask;
}
static uint32_t bits(std::initializer_list<int> b) {
    uint32_t m = 0;
    for (int i : b) m |= 1u << i;
    return m;
}

static void test_t_patterns() {
    printf("== zero patterns of T tables\n");
    struct Want { const char *what; const Row *entry; int pattern; uint32_t mask; } want[] = {
        {"T(alpha, 0): exact zeros", &T_X, 1, 0},
        {"phi = pi: residues of 1.2e-16", &T_XR, 1, bits({2, 3, 5})},
        {"phi = pi / 2: residues of 6e-17", &T_YR, 3, bits({2, 4, 6})},
        {"a general rotation", &T_GEN, 0, 0},
    };
    for (const Want &w : want)
        for (int nc : {8, 12}) {
            Plan p;
            p.space({2, 1});
            Row entry = *w.entry;
            uint32_t mask = w.mask;
            if (nc == 12) {   // the constant term: Re / Im o0 follow the pattern (columns 8, 9), o2, pad
                const double res = w.mask ? (w.pattern == 1 ? 1.2e-16 : 6e-17) : 0.0;
                entry.insert(entry.end(), {w.pattern == 1 ? res : 0.2, w.pattern == 3 ? res : 0.2, 0.1, 0});
                if (w.mask) mask |= 1u << (w.pattern == 1 ? 8 : 9);
            }
            const int64_t off = p.table(entry, 4);
            nc == 8 ? p.T(off, 0) : p.T0(off, 0);
            p.S(), p.ADC(0);
            PlanAnalysis a;
            CHECK(analyse(p, a) == EPGX_OK);
            printf("   %s, %d coefficients: pattern %d, %zu snaps\n", w.what, nc, a.host.zero_pattern[0], a.snaps.size());
            check(a.host.zero_pattern[0] == w.pattern && a.host.zero_pattern[1] == 0, w.what);
            check(mask ? (a.snaps.size() == 1 && same_snap(a.snaps[0], off, 4, nc, mask)) : a.snaps.empty(), "  ... and its snap");
        }
    for (int k : {47, 49}) {   // the 2^-48 rule: one entry of an otherwise clean table carries Im m01 = 2^-k of the entry's modulus
        Plan p;
        p.space({2, 1});
        const int64_t off = p.table(T_X, 4);
        p.coef[(size_t)off + 2 * 8 + 2] = std::ldexp(0.3, -k);   // (hypot(v, 0.3) rounds to 0.3)
        p.T(off, 0), p.S(), p.ADC(0);
        PlanAnalysis a;
        CHECK(analyse(p, a) == EPGX_OK);
        printf("   residue of 2^-%d: pattern %d, %zu snaps\n", k, a.host.zero_pattern[0], a.snaps.size());
        if (k == 47) CHECK(a.host.zero_pattern[0] == 0 && a.snaps.empty());
        else CHECK(a.host.zero_pattern[0] == 1 && a.snaps.size() == 1 && same_snap(a.snaps[0], off, 4, 8, bits({2, 3, 5})));
    }
    {   // a table referenced by two operators and one fuse recipe is scanned and snapped once
        Base b;
        const int64_t off = b.table(T_XR);
        b.ops[0].coef_off = off;
        b.T(off);
        b.n_gen = 48;
        const int64_t F = (int64_t)b.coef.size();
        b.T0(F, 0);
        b.fuse.push_back(fuse_of(F, 0, off, -1, 8, b.tE, 0));
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(a.snaps.size() == 1 && same_snap(a.snaps[0], off, 1, 8, bits({2, 3, 5})));
        CHECK(a.host.zero_pattern[0] == 1 && a.host.zero_pattern[4] == 1 && a.host.zero_pattern[5] == 1);
    }
}

// ------------------------------------------------------------------ zero patterns of relaxation tables
static void test_e_patterns() {
    printf("== zero patterns of E tables\n");
    {
        Base b;
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK && a.host.zero_pattern[1] == 2);
        b.coef[(size_t)b.tE + 3 * 4 + 1] = 1e-300;
        CHECK(analyse(b, a) == EPGX_OK && a.host.zero_pattern[1] == 0);
    }
    {   // 2^17 entries: the scan runs on four threads; the only non-zero Im e0 lies in the last quarter
        Plan p;
        p.shape = {1 << 17};
        p.space({1});
        const int64_t off = p.table(E_REAL, 1 << 17);
        p.E(off), p.S(), p.ADC(0);
        PlanAnalysis a;
        CHECK(analyse(p, a) == EPGX_OK && a.host.zero_pattern[0] == 2);
        p.coef[(size_t)off + (size_t)((1 << 17) - 5) * 4 + 1] = 0.25;
        CHECK(analyse(p, a) == EPGX_OK && a.host.zero_pattern[0] == 0);
    }
    {   // assembled: known from the source column behind column 1
        Full f;
        PlanAnalysis a;
        CHECK(analyse(f, a) == EPGX_OK && a.host.zero_pattern[5] == 2);
        f.coef[(size_t)f.cols0 + 3] = 0.1;
        CHECK(analyse(f, a) == EPGX_OK && a.host.zero_pattern[5] == 0);
    }
}

// ------------------------------------------------------------------ partial patterns
static void test_partial_patterns() {
    printf("== zero patterns of partial tables\n");
    for (int v = 0; v < 3; ++v) {
        Base b;
        b.n_vars = 3, b.n_adc = 4;
        const int64_t dx = b.table(DT_XR), dy = b.table(DT_YR), dg = b.table(DT_GEN), de = b.table(DE_REAL, 4), dp = b.table(DE_PREC, 4);
        const int i2 = b.T(b.tT), i3 = b.T(b.tT), i4 = b.E(b.tE), i5 = b.E(b.tE);
        b.partial(0, v, dx, -1), b.partial(i2, v, dy, -1), b.partial(i3, v, dg, -1), b.partial(i4, v, de, 0), b.partial(i5, v, dp, 0);
        b.partial(1, (v + 1) % 3, de, 0);
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        CHECK(a.host.dpattern[0] == (1u << (2 * v)) && a.host.dpattern[(size_t)i2] == (2u << (2 * v)) && a.host.dpattern[(size_t)i3] == 0);
        CHECK(a.host.dpattern[(size_t)i4] == (1u << (2 * v)) && a.host.dpattern[(size_t)i5] == 0);
        CHECK(a.host.dpattern[1] == (1u << (2 * ((v + 1) % 3))));
        // (scanned in operator order; the relaxation partial shared by two operators once)
        CHECK(a.snaps.size() == 2 && same_snap(a.snaps[0], dx, 1, 10, bits({1, 3, 4, 6})) && same_snap(a.snaps[1], dy, 1, 10, bits({1, 3, 5, 7})));
    }
    {   // exact zeros need no snap
        Full f;
        PlanAnalysis a;
        CHECK(analyse(f, a) == EPGX_OK && a.snaps.empty());
        CHECK(a.host.dpattern[0] == 1 && a.host.dpattern[1] == 1);
        CHECK(a.host.dpattern[(size_t)f.iT0] == (1u | 256u));   // generated: bit 8 + v, pattern 1 from T_X and DT_X
        // an assembled relaxation partial: pattern from its column
        f.n_gen += 16;
        epgx_assemble as = f.assemble[0];
        as.dst_off = f.C + 56;
        f.assemble.push_back(as);
        f.partial(5, 0, as.dst_off, 0);
        CHECK(analyse(f, a) == EPGX_OK && a.host.dpattern[5] == 1);
        f.coef[(size_t)f.cols0 + 1] = 0.5;
        CHECK(analyse(f, a) == EPGX_OK && a.host.dpattern[5] == 0);
    }
}

// ------------------------------------------------------------------ recipes
static void test_recipes() {
    printf("== recipes\n");
    {   // a pattern passes through a chain of two fuse entries
        for (const Row *t : {&T_X, &T_YR, &T_GEN}) {
            Base b;
            const int64_t off = b.table(*t);
            const int64_t F1 = (int64_t)b.coef.size(), F2 = F1 + 48;
            b.n_gen = 96;
            b.fuse.push_back(fuse_of(F1, 0, off, -1, 8, b.tE, 0, 1));
            b.fuse.push_back(fuse_of(F2, 0, F1, 0, 12, b.tE, 0, 0));
            const int i = b.T0(F2, 0);
            PlanAnalysis a;
            CHECK(analyse(b, a) == EPGX_OK);
            CHECK(a.host.zero_pattern[(size_t)i] == (t == &T_X ? 1 : (t == &T_YR ? 3 : 0)));
        }
    }
    // generated_dpattern: (pattern of the rotation, pattern of its partial; 255 = no rotation partial) -> 1 / 2 / 0
    struct Rule { const Row *t, *dt; int want; } rules[] = {
        {&T_X, &DT_X, 1}, {&T_X, nullptr, 1}, {&T_YR, &DT_YR, 2}, {&T_YR, nullptr, 2},
        {&T_X, &DT_YR, 0}, {&T_YR, &DT_X, 0}, {&T_X, &DT_GEN, 0}, {&T_GEN, &DT_X, 0}, {&T_GEN, nullptr, 0},
    };
    for (const Rule &r : rules) {
        Full f;
        for (size_t k = 0; k < 8; ++k) f.coef[(size_t)f.tT + k] = (*r.t)[k];
        for (size_t k = 0; k < 10; ++k) f.coef[(size_t)f.tdT + k] = r.dt ? (*r.dt)[k] : 0.0;
        if (!r.dt) f.fpart[0].dsrc_off = -1;
        PlanAnalysis a;
        CHECK(analyse(f, a) == EPGX_OK);
        CHECK(a.host.dpattern[(size_t)f.iT0] == (uint16_t)(r.want | 256));
    }
}

// ------------------------------------------------------------------ log tables
static void test_log_tables() {
    printf("== log tables\n");
    {
        Base b;
        b.n_vars = 2, b.n_adc = 3;
        const int64_t de = b.table(DE_REAL, 4), de2 = b.table(DE_REAL, 4), dprec = b.table(DE_PREC, 4), e1 = b.table(E_REAL, 2), de1 = b.table(DE_REAL, 2);
        const int i4 = b.E(b.tE), i5 = b.E(e1, 1), i6 = b.E(b.tE);
        b.partial(1, 0, de, 0), b.partial(1, 1, de2, 0), b.partial(i4, 1, de, 0), b.partial(i5, 0, de1, 1), b.partial(i6, 0, dprec, 0);
        b.partial(i6, 1, de1, 1);   // another index space than its operator's: no log table
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        const int64_t n_pool = (int64_t)b.coef.size();
        CHECK(a.host.n_pool == n_pool && !a.host.fold);
        CHECK(a.host.logtabs.size() == 3 && a.log_jobs.size() == 3 && a.host.n_log == 2 * 4 + 2 * 4 + 2 * 2);
        CHECK(a.host.logtabs[0].off == n_pool + 32 && a.host.logtabs[1].off == n_pool + 32 + 8 && a.host.logtabs[2].off == n_pool + 32 + 16);
        CHECK(a.host.logtabs[0].space == 0 && a.host.logtabs[2].space == 1);
        CHECK(a.log_jobs[0].e_off == b.tE && a.log_jobs[0].de_off == de && a.log_jobs[0].entries == 4);
        CHECK(a.log_jobs[1].de_off == de2 && a.log_jobs[2].e_off == e1 && a.log_jobs[2].de_off == de1 && a.log_jobs[2].entries == 2);
        auto log_of = [&](int i, int v) { return a.host.log_of[(size_t)i * EPGX_MAX_VARS + (size_t)v]; };
        CHECK(a.host.log_of.size() == b.ops.size() * EPGX_MAX_VARS);
        CHECK(log_of(1, 0) == 0 && log_of(1, 1) == 1 && log_of(i4, 1) == 0 && log_of(i4, 0) == -1 && log_of(i5, 0) == 2);
        CHECK(log_of(i6, 0) == -1 && log_of(i6, 1) == -1 && log_of(0, 0) == -1 && log_of(1, 2) == -1);
        CHECK(a.host.t0_log.empty() && a.host.t0_logd.empty());
        // empty without the fold: Knobs::fold off, EPGX_PLAN_NO_FOLD, no variables
        Knobs off = defaults();
        off.fold = false;
        CHECK(analyse(b, a, off) == EPGX_OK && a.host.logtabs.empty() && a.host.log_of.empty() && a.log_jobs.empty() && a.host.n_log == 0);
        b.flags = EPGX_PLAN_NO_FOLD;
        CHECK(analyse(b, a) == EPGX_OK && a.host.logtabs.empty() && a.host.log_of.empty() && a.log_jobs.empty() && a.host.n_log == 0);
        Base plain;
        CHECK(analyse(plain, a) == EPGX_OK && a.host.fold && a.host.logtabs.empty() && a.host.log_of.empty() && a.log_jobs.empty());
        CHECK(analyse(plain, a, off) == EPGX_OK && !a.host.fold);
        plain.flags = EPGX_PLAN_NO_FOLD;
        CHECK(analyse(plain, a) == EPGX_OK && !a.host.fold);
    }
    // the fuse_partial walk behind the partial of a fused echo E_a . T . E_b (relaxations alone: no rotation partial)
    struct Echo : Base {
        int64_t de, F1, F2, P1, P2;
        int iT0;
        Echo() {
            n_vars = 1, n_adc = 2;
            de = table(DE_REAL, 4);
            F1 = (int64_t)coef.size(), F2 = F1 + 48, P1 = F2 + 48, P2 = P1 + 56, n_gen = 96 + 112;
            fuse.push_back(fuse_of(F1, 0, tT, -1, 8, tE, 0, 1));
            fuse.push_back(fuse_of(F2, 0, F1, 0, 12, tE, 0, 0));
            fpart.push_back(fpart_of(P1, 0, tT, -1, 8, -1, -1, 0, tE, 0, de, 0, 1));
            fpart.push_back(fpart_of(P2, 0, F1, 0, 12, P1, 0, 14, tE, 0, de, 0, 0));
            iT0 = T0(F2, 0);
            partial(1, 0, de, 0), partial(iT0, 0, P2, 0);
        }
    };
    {
        Echo e;
        PlanAnalysis a;
        CHECK(analyse(e, a) == EPGX_OK);
        const size_t at = (size_t)e.iT0 * EPGX_MAX_VARS;
        CHECK(a.host.logtabs.size() == 1 && a.host.log_of[1 * EPGX_MAX_VARS] == 0);   // (the E operator's table, shared by both sides)
        CHECK(a.host.t0_log.size() == e.ops.size() * EPGX_MAX_VARS * 2 && a.host.t0_logd.size() == e.ops.size() * EPGX_MAX_VARS);
        CHECK(a.host.t0_logd[at] == 1 && a.host.t0_log[at * 2] == 0 && a.host.t0_log[at * 2 + 1] == 0);
        CHECK(a.host.t0_logd[at + 1] == 0 && a.host.t0_log[at * 2 + 2] == -1);
        // one side only
        e.fpart[1].de_off = -1;
        CHECK(analyse(e, a) == EPGX_OK && a.host.t0_logd[at] == 1 && a.host.t0_log[at * 2] == 0 && a.host.t0_log[at * 2 + 1] == -1);
    }
    {   // a second relaxation on one side: not logarithmic
        Echo e;
        e.fpart[1].after = 1;
        PlanAnalysis a;
        CHECK(analyse(e, a) == EPGX_OK);
        CHECK(a.host.t0_logd[(size_t)e.iT0 * EPGX_MAX_VARS] == 0 && a.host.t0_log[(size_t)e.iT0 * EPGX_MAX_VARS * 2] == -1);
    }
    {   // a rotation partial of the host: not logarithmic
        Echo e;
        e.fpart[0].dsrc_off = e.table(DT_X), e.fpart[0].dsrc_space = -1, e.fpart[0].dsrc_ncoef = 10;
        for (int64_t *off : {&e.F1, &e.F2, &e.P1, &e.P2}) *off += 10;
        e.fuse[0].dst_off = e.F1, e.fuse[1].dst_off = e.F2, e.fuse[1].src_off = e.F1, e.fpart[0].dst_off = e.P1;
        e.fpart[1].dst_off = e.P2, e.fpart[1].src_off = e.F1, e.fpart[1].dsrc_off = e.P1;
        e.ops[(size_t)e.iT0].coef_off = e.F2, e.dops[(size_t)e.iT0].coef_off[0] = e.P2;
        PlanAnalysis a;
        CHECK(analyse(e, a) == EPGX_OK);
        CHECK(a.host.t0_logd[(size_t)e.iT0 * EPGX_MAX_VARS] == 0);
    }
    for (int depth : {7, 8}) {   // a chain of `depth` + 1 recipes: eight are walked, nine are not
        Base b;
        b.n_vars = 1, b.n_adc = 2;
        const int64_t dE = b.table(DE_REAL, 4), F = (int64_t)b.coef.size(), P = F + 48;
        b.n_gen = 48 + 56 * (depth + 1);
        b.fuse.push_back(fuse_of(F, 0, b.tT, -1, 8, b.tE, 0, 1));
        for (int k = 0; k <= depth; ++k)   // the first recipe differentiates the relaxation, every later one the recipe before it
            b.fpart.push_back(k == 0 ? fpart_of(P, 0, b.tT, -1, 8, -1, -1, 0, b.tE, 0, dE, 0, 1)
                                     : fpart_of(P + 56 * k, 0, F, 0, 12, P + 56 * (k - 1), 0, 14, b.tE, 0, -1, -1, 1));
        const int i = b.T0(F, 0);
        b.partial(i, 0, P + 56 * depth, 0);
        PlanAnalysis a;
        CHECK(analyse(b, a) == EPGX_OK);
        printf("   %d recipes behind the partial: %s\n", depth + 1, a.host.t0_logd[(size_t)i * EPGX_MAX_VARS] ? "logarithmic" : "not logarithmic");
        CHECK(a.host.t0_logd[(size_t)i * EPGX_MAX_VARS] == (depth == 7 ? 1 : 0));
    }
}

int main() {
    test_refusals();
    test_geometry();
    test_t_patterns();
    test_e_patterns();
    test_partial_patterns();
    test_recipes();
    test_log_tables();
    printf("plan_check: all checks passed\n");
    return 0;
}

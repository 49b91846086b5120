// signal_check.cpp -- the argument checks of the signal consumers (epgpy_amd/csrc/epgx_signal_check.cpp) on a machine without a GPU.
//
// Describes a call of epgx_signal_crlb, _crlb_grad, _norms(_c64), _match(_c64), _refine, _component_gram, _nnls, _nnls_chi2, _gram
// or _project by its arguments -- device pointers are made-up addresses (0x1000 aligned to 16 bytes, + 8, + 4, + 2 for the
// misaligned ones) that nothing dereferences -- and runs the C++ that ships: every refusal the GPU tests provoke through raw calls
// (the bad_* lists of test_entry_point_errors and their siblings in tests/test_gpu_{match,match32,refine,nnls,nnls_chi2,compress,
// stats,stats_grad}.py) with its code and its full message, the accepting calls next to them, both sides of the extent and count
// limits that no GPU test reaches, and the launch facts: the split rule, the LDS chunks, the scratch lengths.  One line per check;
// exits non-zero at the first failure.  `make signal_check` builds it, `make asan` with the address / undefined-behaviour
// sanitizers (tests/test_signal_check_host.py runs the plain build).
//
// The message texts are those of epgx_api.hip before the checks moved out of it; the expected launch facts are worked out by hand
// from the formulas that file had.  What this program cannot reach is each entry's guard against a NULL context (the GPU tests).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_signal_check.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) exit(1);
}
#define CHECK(cond) check((cond), #cond)
// a copy of the default call `T` with some members changed
#define WITH(T, ...) ([&] { T c; __VA_ARGS__; return c; }())

static int n_refusals = 0;
static void refuse(const std::string &what, int rc, const std::string &message) {
    printf("   %d: %s\n", rc, g_err);
    check(rc == EPGX_ERR_INVALID && message == g_err, what.c_str());
    ++n_refusals;
}
static void accept(const std::string &what, int rc) {
    if (rc) printf("   %d: %s\n", rc, g_err);
    check(rc == EPGX_OK, what.c_str());
}

static const void *at(uintptr_t address) { return (const void *)address; }
static const int64_t BIG = (int64_t)1 << 62, L16 = INT64_MAX / 16, L8 = INT64_MAX / 8;      // L16 = 576460752303423487, L8 = 1152921504606846975
static const int32_t IMAX = 0x7fffffff;
static const double INF = INFINITY, NaN = NAN;

// ------------------------------------------------------------------ the shared predicates
static void extents() {
    for (int64_t bytes : {16, 8}) {
        const int64_t L = bytes == 16 ? L16 : L8;
        CHECK(records_extent_ok(2, L - 17, 17, bytes));            // (nrec - 1) * row_stride + cols = L exactly
        CHECK(!records_extent_ok(2, L - 16, 17, bytes));           // L + 1
        CHECK(records_extent_ok(1, L, L, bytes) && !records_extent_ok(1, L + 1, L + 1, bytes));
        CHECK(records_extent_ok(5, 17, 17, bytes) && !records_extent_ok(5, 16, 17, bytes));      // row_stride == cols, cols - 1
        CHECK(records_extent_ok(5, 0, 0, bytes) && !records_extent_ok(5, -1, 0, bytes));
        CHECK(!records_extent_ok(IMAX, BIG, 17, bytes));           // the product overflows
        CHECK(!records_extent_ok(2, INT64_MAX, INT64_MAX, bytes)); // the sum overflows
    }
    CHECK(L16 == 576460752303423487 && L8 == 1152921504606846975);
    // the Jacobian block: (nrec - 1) * record_stride + nrow * row_stride <= L16
    accept("jacobian block: span == INT64_MAX / 16", jacobian_block_check("who", L16 - 51, 17, 3, 2));
    refuse("jacobian block: span one above", jacobian_block_check("who", L16 - 50, 17, 3, 2),
           "who: nrec = 2 records of record_stride = 576460752303423437 elements overflow the address range");
    accept("jacobian block: record_stride == nrow * row_stride", jacobian_block_check("who", 51, 17, 3, 5));
    refuse("jacobian block: record_stride one short", jacobian_block_check("who", 50, 17, 3, 5),
           "who: record_stride = 50 holds fewer than nrow = 3 rows of 17");
    refuse("jacobian block: the sum overflows", jacobian_block_check("who", BIG, BIG, 1, 2),
           "who: nrec = 2 records of record_stride = 4611686018427387904 elements overflow the address range");
}

// ------------------------------------------------------------------ Cramer-Rao bounds (tests/test_gpu_stats.py, test_gpu_stats_grad.py)
struct Crlb {      // 6 records x 4 rows x 32 voxels
    const void *signal = at(0x1000), *out = at(0x2000);
    int64_t record_stride = 128, row_stride = 32, vox0 = 0, nvox = 32;
    int32_t nrow = 4, nrec = 6, nparam = 2, flags = 0;
    std::vector<int32_t> rows = {0, 1, 0, 0, 0, 0, 0, 0};
    std::vector<double> w;
    bool no_rows = false;
    double sigma2 = 1.0;
};
static int call(const Crlb &c) {
    g_err[0] = 0;
    return crlb_check("epgx_signal_crlb", c.signal, c.record_stride, c.row_stride, c.nrow, c.nrec, c.nparam, c.no_rows ? nullptr : c.rows.data(),
                      c.vox0, c.nvox, c.w.empty() ? nullptr : c.w.data(), c.sigma2, c.flags, c.out);
}
static void crlb() {
    accept("crlb: the call of the GPU test", call(Crlb()));
    accept("crlb: nvox = 0", call(WITH(Crlb, c.nvox = 0)));
    accept("crlb: both flags, weights", call(WITH(Crlb, c.flags = EPGX_CRLB_SPLIT | EPGX_CRLB_LOG10, c.w = {1.0, 2.0})));
    for (int k = 0; k < 3; ++k)
        refuse("crlb: NULL argument " + std::to_string(k), call(WITH(Crlb, k == 0 ? (void)(c.signal = 0) : k == 1 ? (void)(c.no_rows = true) : (void)(c.out = 0))),
               "epgx_signal_crlb: NULL argument");
    refuse("crlb: out + 4", call(WITH(Crlb, c.out = at(0x2004))), "epgx_signal_crlb: out must be aligned to 8 bytes");
    refuse("crlb: signal + 8", call(WITH(Crlb, c.signal = at(0x1008))), "epgx_signal_crlb: signal must be aligned to 16 bytes");
    refuse("crlb: nparam = 0", call(WITH(Crlb, c.nparam = 0)), "epgx_signal_crlb: nparam = 0 not in [1, 4]");
    refuse("crlb: nparam = 5", call(WITH(Crlb, c.nparam = 5, c.rows = {0, 1, 2, 3, 0})), "epgx_signal_crlb: nparam = 5 not in [1, 4]");
    refuse("crlb: rows = (0, 4)", call(WITH(Crlb, c.rows = {0, 4})), "epgx_signal_crlb: rows[1] = 4 not in [0, nrow = 4)");
    refuse("crlb: nvox = -1", call(WITH(Crlb, c.nvox = -1)), "epgx_signal_crlb: voxels [0, 0 + -1) outside a row of 32");
    refuse("crlb: vox0 = 1", call(WITH(Crlb, c.vox0 = 1)), "epgx_signal_crlb: voxels [1, 1 + 32) outside a row of 32");
    refuse("crlb: nrec = 0", call(WITH(Crlb, c.nrec = 0)), "epgx_signal_crlb: nrec = 0, nrow = 4: both must be >= 1");
    refuse("crlb: sigma2 = 0", call(WITH(Crlb, c.sigma2 = 0.0)), "epgx_signal_crlb: sigma2 = 0 is not a positive finite number");
    refuse("crlb: sigma2 = inf", call(WITH(Crlb, c.sigma2 = INF)), "epgx_signal_crlb: sigma2 = inf is not a positive finite number");
    refuse("crlb: flags = 4", call(WITH(Crlb, c.flags = 4)), "epgx_signal_crlb: unknown flags 0x4");
    refuse("crlb: nrow = 5", call(WITH(Crlb, c.nrow = 5)), "epgx_signal_crlb: record_stride = 128 holds fewer than nrow = 5 rows of 32");
    refuse("crlb: weights = (1, inf)", call(WITH(Crlb, c.w = {1.0, INF})), "epgx_signal_crlb: weights[1] is not finite");
    refuse("crlb: record_stride = 2^62", call(WITH(Crlb, c.record_stride = BIG)),
           "epgx_signal_crlb: nrec = 6 records of record_stride = 4611686018427387904 elements overflow the address range");
    // nvox / 64 at 0x7fffffff
    const int64_t many = (int64_t)64 * IMAX;      // 137438953408
    accept("crlb: nvox / 64 = 0x7ffffffe", call(WITH(Crlb, c.nrec = 1, c.row_stride = many, c.record_stride = 4 * many, c.nvox = many - 1)));
    refuse("crlb: nvox / 64 = 0x7fffffff", call(WITH(Crlb, c.nrec = 1, c.row_stride = many, c.record_stride = 4 * many, c.nvox = many)),
           "epgx_signal_crlb: 137438953408 voxels in one call");
    // the order of the checks: alignment of out before anything about the block, nparam before nrec
    refuse("crlb: out + 4 and nparam = 0", call(WITH(Crlb, c.out = at(0x2004), c.nparam = 0)), "epgx_signal_crlb: out must be aligned to 8 bytes");
    refuse("crlb: nparam = 0 and nrec = 0", call(WITH(Crlb, c.nparam = 0, c.nrec = 0)), "epgx_signal_crlb: nparam = 0 not in [1, 4]");
}

struct Grad : Crlb {      // P = 2 columns, nx = 3 design variables: entry i = a * nx + x at offset 192 i, records 32 apart; entry (0, 1) all zero
    const void *hess = at(0x3000), *cost = at(0x2000), *grad = at(0x2100);
    int64_t hess_len = 1152;      // 5 * 192 + 5 * 32 + 32: exactly what the last record of the last entry needs
    int32_t nx = 3;
    std::vector<int64_t> offsets = {0, -1, 384, 576, 768, 960}, steps = {32, 0, 32, 32, 32, 32};
    bool no_offsets = false, no_steps = false;
};
static int call(const Grad &c) {
    g_err[0] = 0;
    return crlb_grad_check("epgx_signal_crlb_grad", c.signal, c.record_stride, c.row_stride, c.nrow, c.nrec, c.nparam, c.no_rows ? nullptr : c.rows.data(),
                           c.vox0, c.nvox, c.hess, c.hess_len, c.nx, c.no_offsets ? nullptr : c.offsets.data(), c.no_steps ? nullptr : c.steps.data(),
                           c.w.empty() ? nullptr : c.w.data(), c.sigma2, c.flags, c.cost, c.grad);
}
static void crlb_grad() {
    const std::string W = "epgx_signal_crlb_grad";
    accept("crlb_grad: hess_len exactly what is read", call(Grad()));
    accept("crlb_grad: nvox = 0", call(WITH(Grad, c.nvox = 0)));
    accept("crlb_grad: EPGX_CRLB_LOG10", call(WITH(Grad, c.flags = EPGX_CRLB_LOG10)));
    refuse("crlb_grad: hess_len one element short", call(WITH(Grad, c.hess_len = 1151)),
           W + ": entry (1, 2) of H: offset = 960, record stride = 32, 6 records of voxels [0, 0 + 32) do not lie inside hess_len = 1151 elements "
               "(or the records overlap)");
    refuse("crlb_grad: one short, voxels [1, 32)", call(WITH(Grad, c.vox0 = 1, c.nvox = 31, c.hess_len = 1151)),
           W + ": entry (1, 2) of H: offset = 960, record stride = 32, 6 records of voxels [1, 1 + 31) do not lie inside hess_len = 1151 elements "
               "(or the records overlap)");
    refuse("crlb_grad: records that overlap", call(WITH(Grad, c.steps = {31, 0, 31, 31, 31, 31})),
           W + ": entry (0, 0) of H: offset = 0, record stride = 31, 6 records of voxels [0, 0 + 32) do not lie inside hess_len = 1152 elements "
               "(or the records overlap)");
    refuse("crlb_grad: a negative record stride", call(WITH(Grad, c.steps[3] = -32)),
           W + ": entry (1, 0) of H: offset = 576, record stride = -32, 6 records of voxels [0, 0 + 32) do not lie inside hess_len = 1152 elements "
               "(or the records overlap)");
    refuse("crlb_grad: flags = EPGX_CRLB_SPLIT", call(WITH(Grad, c.flags = 1)), W + ": unknown flags 0x1");
    refuse("crlb_grad: nx = 0", call(WITH(Grad, c.nx = 0)), W + ": nx = 0 must be >= 1");
    refuse("crlb_grad: hess_len = -1", call(WITH(Grad, c.hess_len = -1)), W + ": hess_len = -1");
    refuse("crlb_grad: hess_len above INT64_MAX / 16", call(WITH(Grad, c.hess_len = L16 + 1)), W + ": hess_len = 576460752303423488");
    accept("crlb_grad: hess_len = INT64_MAX / 16", call(WITH(Grad, c.hess_len = L16)));
    refuse("crlb_grad: an offset whose end overflows", call(WITH(Grad, c.offsets[5] = INT64_MAX - 100, c.hess_len = L16)),
           W + ": entry (1, 2) of H: offset = 9223372036854775707, record stride = 32, 6 records of voxels [0, 0 + 32) do not lie inside hess_len = "
               "576460752303423487 elements (or the records overlap)");
    for (int k = 0; k < 7; ++k)
        refuse("crlb_grad: NULL argument " + std::to_string(k),
               call(WITH(Grad, k == 0 ? (void)(c.signal = 0) : k == 1 ? (void)(c.no_rows = true) : k == 2 ? (void)(c.hess = 0) : k == 3 ? (void)(c.no_offsets = true)
                                 : k == 4 ? (void)(c.no_steps = true) : k == 5 ? (void)(c.cost = 0) : (void)(c.grad = 0))),
               W + ": NULL argument");
    for (int k = 0; k < 3; ++k)
        refuse("crlb_grad: misaligned " + std::to_string(k),
               call(WITH(Grad, k == 0 ? (void)(c.hess = at(0x3008)) : k == 1 ? (void)(c.cost = at(0x2004)) : (void)(c.grad = at(0x2104)))),
               W + ": hess must be aligned to 16 bytes, out_cost and out_grad to 8");
    refuse("crlb_grad: the Jacobian's checks come before nx", call(WITH(Grad, c.nx = 0, c.nrow = 5)),
           W + ": record_stride = 128 holds fewer than nrow = 5 rows of 32");
}

// ------------------------------------------------------------------ matching in both precisions (tests/test_gpu_match.py, test_gpu_match32.py)
struct Norms {      // 17 atoms x 5 records
    bool c64 = false;
    const void *dict = at(0x1000), *out = at(0x2000);
    int64_t stride = 17, natoms = 17;
    int32_t nrec = 5;
};
static const char *norms_name(bool c64) { return c64 ? "epgx_signal_norms_c64" : "epgx_signal_norms"; }
static int call(const Norms &c) {
    g_err[0] = 0;
    return norms_check(norms_name(c.c64), c.dict, c.stride, c.nrec, c.natoms, c.out, c.c64 ? 8 : 16);
}
static void norms() {
    for (bool c64 : {false, true}) {
        const std::string W = norms_name(c64), tag = W.substr(12) + ": ";
        const std::string align = c64 ? W + ": dict and out must be aligned to 8 bytes" : W + ": dict must be aligned to 16 bytes, out to 8";
        const uintptr_t odd = c64 ? 0x1004 : 0x1008;
#define N(...) call(WITH(Norms, c.c64 = c64, __VA_ARGS__))
        accept(tag + "the call of the GPU test", N((void)0));
        refuse(tag + "dict NULL", N(c.dict = 0), W + ": NULL argument");
        refuse(tag + "out NULL", N(c.out = 0), W + ": NULL argument");
        refuse(tag + "dict misaligned", N(c.dict = at(odd)), align);
        refuse(tag + "out + 4", N(c.out = at(0x2004)), align);
        refuse(tag + "nrec = 0", N(c.nrec = 0), W + ": nrec = 0, natoms = 17: both must be >= 1");
        refuse(tag + "natoms = 0", N(c.natoms = 0), W + ": nrec = 5, natoms = 0: both must be >= 1");
        refuse(tag + "natoms = -1", N(c.natoms = -1), W + ": nrec = 5, natoms = -1: both must be >= 1");
        refuse(tag + "stride = natoms - 1", N(c.stride = 16), W + ": 5 records of row_stride = 16 do not hold 17 atoms each (or overflow the address range)");
        refuse(tag + "stride = 2^62, nrec = 2^31 - 1", N(c.stride = BIG, c.nrec = IMAX),
               W + ": 2147483647 records of row_stride = 4611686018427387904 do not hold 17 atoms each (or overflow the address range)");
        // the extent at INT64_MAX / elem_bytes, through the entry's check
        const int64_t L = c64 ? L8 : L16;
        accept(tag + "extent == INT64_MAX / elem_bytes", N(c.nrec = 2, c.stride = L - 17));
        refuse(tag + "extent one above", N(c.nrec = 2, c.stride = L - 16),
               W + ": 2 records of row_stride = " + std::to_string(L - 16) + " do not hold 17 atoms each (or overflow the address range)");
        const int64_t many = (int64_t)256 * IMAX;      // natoms / 256 at 0x7fffffff: 549755813632
        accept(tag + "natoms / 256 = 0x7ffffffe", N(c.nrec = 1, c.stride = many, c.natoms = many - 1));
        refuse(tag + "natoms / 256 = 0x7fffffff", N(c.nrec = 1, c.stride = many, c.natoms = many),
               W + ": 1 records of row_stride = 549755813632 do not hold 549755813632 atoms each (or overflow the address range)");
#undef N
    }
    accept("norms_c64: dict + 8 is aligned for complex64", call(WITH(Norms, c.c64 = true, c.dict = at(0x1008), c.natoms = 16)));
    accept("norms: an extent complex64 holds ...", call(WITH(Norms, c.c64 = true, c.nrec = 2, c.stride = L16 + 1)));
    refuse("norms: ... and complex128 does not", call(WITH(Norms, c.nrec = 2, c.stride = L16 + 1)),
           "epgx_signal_norms: 2 records of row_stride = 576460752303423488 do not hold 17 atoms each (or overflow the address range)");
}

struct Match {      // 17 atoms x 15 voxels x 5 records on 256 compute units
    bool c64 = false;
    const void *dict = at(0x1000), *norms = at(0x2000), *sig = at(0x3000), *index = at(0x4000), *scale = at(0x5000), *score = at(0x6000);
    int64_t dstride = 17, natoms = 17, sstride = 15, nmeas = 15;
    int32_t nrec = 5, nsplit = 0;
    int cu = 256;
};
static const char *match_name(bool c64) { return c64 ? "epgx_signal_match_c64" : "epgx_signal_match"; }
static MatchPlan plan;
static int call(const Match &c) {
    g_err[0] = 0;
    return match_check(match_name(c.c64), c.dict, c.dstride, c.norms, c.natoms, c.sig, c.sstride, c.nrec, c.nmeas, c.nsplit, c.index, c.scale, c.score,
                       c.cu, c.c64 ? 8 : 16, c.c64 ? MATCH32_CHUNK : MATCH_CHUNK, &plan);
}
static bool plan_is(int64_t nvt, int32_t nsplit, int64_t scratch_len, int32_t chunk, int32_t nchunk) {
    printf("   nvt %lld nsplit %d scratch_len %lld chunk %d nchunk %d\n", (long long)plan.nvt, plan.nsplit, (long long)plan.scratch_len, plan.chunk, plan.nchunk);
    return plan.nvt == nvt && plan.nsplit == nsplit && plan.scratch_len == scratch_len && plan.chunk == chunk && plan.nchunk == nchunk;
}
static void match() {
    for (bool c64 : {false, true}) {
        const std::string W = match_name(c64), tag = W.substr(12) + ": ";
        const std::string align = c64 ? W + ": out_scale must be aligned to 16 bytes, dict, sig, norms, out_index and out_score to 8"
                                      : W + ": dict, sig and out_scale must be aligned to 16 bytes, norms, out_index and out_score to 8";
        const uintptr_t odd = c64 ? 4 : 8;
#define M(...) call(WITH(Match, c.c64 = c64, __VA_ARGS__))
        accept(tag + "the call of the GPU test", M((void)0));
        CHECK(plan_is(1, 1, 15, 8, 1));      // cu 256, 17 atoms, 15 voxels: most = max(17 / 64, 1) = 1 split; 5 records: one chunk of 8
        accept(tag + "nmeas = 0", M(c.nmeas = 0));
        CHECK(plan_is(0, 0, 0, 0, 0));
        accept(tag + "nmeas = 0, sig_row_stride = 0", M(c.nmeas = 0, c.sstride = 0));
        accept(tag + "nsplit = natoms", M(c.nsplit = 17));
        CHECK(plan_is(1, 17, 17 * 15, 8, 1));
        for (int k = 0; k < 6; ++k)
            refuse(tag + "NULL argument " + std::to_string(k),
                   M(k == 0 ? (void)(c.dict = 0) : k == 1 ? (void)(c.norms = 0) : k == 2 ? (void)(c.sig = 0) : k == 3 ? (void)(c.index = 0)
                     : k == 4 ? (void)(c.scale = 0) : (void)(c.score = 0)), W + ": NULL argument");
        refuse(tag + "dict misaligned", M(c.dict = at(0x1000 + odd)), align);
        refuse(tag + "sig misaligned", M(c.sig = at(0x3000 + odd)), align);
        refuse(tag + "out_scale + 8", M(c.scale = at(0x5008)), align);
        refuse(tag + "norms + 4", M(c.norms = at(0x2004)), align);
        refuse(tag + "out_index + 4", M(c.index = at(0x4004)), align);
        refuse(tag + "out_score + 4", M(c.score = at(0x6004)), align);
        refuse(tag + "nrec = 0", M(c.nrec = 0), W + ": nrec = 0, natoms = 17 (both >= 1), nmeas = 15 (>= 0)");
        refuse(tag + "nrec = -3", M(c.nrec = -3), W + ": nrec = -3, natoms = 17 (both >= 1), nmeas = 15 (>= 0)");
        refuse(tag + "natoms = 0", M(c.natoms = 0), W + ": nrec = 5, natoms = 0 (both >= 1), nmeas = 15 (>= 0)");
        refuse(tag + "nmeas = -1", M(c.nmeas = -1), W + ": nrec = 5, natoms = 17 (both >= 1), nmeas = -1 (>= 0)");
        refuse(tag + "nsplit = -1", M(c.nsplit = -1), W + ": nsplit = -1 not in [0, natoms = 17]");
        refuse(tag + "nsplit = natoms + 1", M(c.nsplit = 18), W + ": nsplit = 18 not in [0, natoms = 17]");
        refuse(tag + "dict_row_stride = natoms - 1", M(c.dstride = 16),
               W + ": 5 records of dict_row_stride = 16 do not hold 17 atoms each (or overflow the address range)");
        refuse(tag + "sig_row_stride = nmeas - 1", M(c.sstride = 14),
               W + ": 5 records of sig_row_stride = 14 do not hold 15 voxels each (or overflow the address range)");
        refuse(tag + "dict_row_stride = 2^62, nrec = 2^31 - 1", M(c.dstride = BIG, c.nrec = IMAX),
               W + ": 2147483647 records of dict_row_stride = 4611686018427387904 do not hold 17 atoms each (or overflow the address range)");
        refuse(tag + "sig_row_stride = 2^62, nrec = 2^31 - 1", M(c.sstride = BIG, c.nrec = IMAX),
               W + ": 2147483647 records of sig_row_stride = 4611686018427387904 do not hold 15 voxels each (or overflow the address range)");
        // both extents at INT64_MAX / elem_bytes
        const int64_t L = c64 ? L8 : L16;
        accept(tag + "dictionary extent == INT64_MAX / elem_bytes", M(c.nrec = 2, c.dstride = L - 17));
        refuse(tag + "dictionary extent one above", M(c.nrec = 2, c.dstride = L - 16),
               W + ": 2 records of dict_row_stride = " + std::to_string(L - 16) + " do not hold 17 atoms each (or overflow the address range)");
        accept(tag + "signal extent == INT64_MAX / elem_bytes", M(c.nrec = 2, c.sstride = L - 15));
        refuse(tag + "signal extent one above", M(c.nrec = 2, c.sstride = L - 14),
               W + ": 2 records of sig_row_stride = " + std::to_string(L - 14) + " do not hold 15 voxels each (or overflow the address range)");
        // the split rule for nsplit = 0: min(ceil(4 cu / nvt), max(natoms / 64, 1), 65536)
        accept(tag + "split rule 256 / 65536 / 64", M(c.natoms = c.dstride = 65536, c.nmeas = c.sstride = 64));
        CHECK(plan.nsplit == 1024 && plan.nvt == 1 && plan.scratch_len == 65536);
        accept(tag + "split rule 256 / 2^20 / 6400", M(c.natoms = c.dstride = 1 << 20, c.nmeas = c.sstride = 6400));
        CHECK(plan.nsplit == 11 && plan.nvt == 100 && plan.scratch_len == 70400);
        accept(tag + "split rule 20000 / 2^30 / 64: the cap", M(c.cu = 20000, c.natoms = c.dstride = 1 << 30, c.nmeas = c.sstride = 64));
        CHECK(plan.nsplit == 65536 && plan.nvt == 1 && plan.scratch_len == 4194304);
        accept(tag + "no compute units reported", M(c.cu = 0, c.natoms = c.dstride = 65536));
        CHECK(plan.nsplit == 4);
        // nvt * nsplit workgroups at 0x7fffffff
        accept(tag + "32767 voxel tiles x 65536 splits", M(c.natoms = c.dstride = 65536, c.nsplit = 65536, c.nmeas = c.sstride = 64 * 32767));
        CHECK(plan.nvt == 32767 && plan.scratch_len == (int64_t)65536 * 64 * 32767);
        refuse(tag + "32768 voxel tiles x 65536 splits", M(c.natoms = c.dstride = 65536, c.nsplit = 65536, c.nmeas = c.sstride = 64 * 32768),
               W + ": nsplit = 65536 splits of 2097152 voxels in one call");
        // nrec at its largest: the chunk arithmetic stays inside int32
        accept(tag + "nrec = 2^31 - 1", M(c.nrec = IMAX));
        CHECK(plan.chunk == (c64 ? 64 : 32) && plan.nchunk == (c64 ? 33554432 : 67108864));
#undef M
    }
    // records per LDS chunk: a multiple of 4, at most 32 (complex128) or 64 (complex64)
    accept("match: nrec = 33", call(WITH(Match, c.nrec = 33)));
    CHECK(plan.chunk == 32 && plan.nchunk == 2);
    accept("match: nrec = 32", call(WITH(Match, c.nrec = 32)));
    CHECK(plan.chunk == 32 && plan.nchunk == 1);
    accept("match_c64: nrec = 5", call(WITH(Match, c.c64 = true)));
    CHECK(plan.chunk == 8 && plan.nchunk == 1);
    accept("match_c64: nrec = 33", call(WITH(Match, c.c64 = true, c.nrec = 33)));
    CHECK(plan.chunk == 36 && plan.nchunk == 1);
    accept("match_c64: nrec = 65", call(WITH(Match, c.c64 = true, c.nrec = 65)));
    CHECK(plan.chunk == 64 && plan.nchunk == 2);
    CHECK(sizeof(MatchPartial) == 32);
}

// ------------------------------------------------------------------ Gauss-Newton refinement (tests/test_gpu_refine.py)
struct Refine {      // 17 atoms, 9 voxels, 5 records of 3 rows, columns (1, 2)
    const void *jac = at(0x1000), *sig = at(0x3000), *index = at(0x4000), *delta = at(0x5000), *scale = at(0x6000), *score = at(0x7000);
    int64_t rstride = 51, stride = 17, natoms = 17, sstride = 9, nmeas = 9;
    int32_t nrow = 3, nrec = 5;
    std::vector<int32_t> rows = {1, 2};
    std::vector<double> limit;
    bool no_rows = false;
    double rcond = 1e-10;
};
static int call(const Refine &c) {
    g_err[0] = 0;
    return refine_check("epgx_signal_refine", c.jac, c.rstride, c.stride, c.nrow, c.nrec, c.no_rows ? 2 : (int32_t)c.rows.size(),
                        c.no_rows ? nullptr : c.rows.data(), c.natoms, c.sig, c.sstride, c.nmeas, c.index, c.limit.empty() ? nullptr : c.limit.data(),
                        c.rcond, c.delta, c.scale, c.score);
}
static void refine() {
    const std::string W = "epgx_signal_refine";
    const std::string align = W + ": jac, sig and out_scale must be aligned to 16 bytes, index, out_delta and out_score to 8";
    accept("refine: the call of the GPU test", call(Refine()));
    accept("refine: nmeas = 0", call(WITH(Refine, c.nmeas = 0)));
    accept("refine: nmeas = 0, sig_row_stride = 0", call(WITH(Refine, c.nmeas = 0, c.sstride = 0)));
    accept("refine: limit = (inf, 2), rcond = 0", call(WITH(Refine, c.limit = {INF, 2.0}, c.rcond = 0.0)));
    for (int k = 0; k < 7; ++k)
        refuse("refine: NULL argument " + std::to_string(k),
               call(WITH(Refine, k == 0 ? (void)(c.jac = 0) : k == 1 ? (void)(c.no_rows = true) : k == 2 ? (void)(c.sig = 0) : k == 3 ? (void)(c.index = 0)
                                 : k == 4 ? (void)(c.delta = 0) : k == 5 ? (void)(c.scale = 0) : (void)(c.score = 0))),
               W + ": NULL argument");
    refuse("refine: jac + 8", call(WITH(Refine, c.jac = at(0x1008))), align);
    refuse("refine: sig + 8", call(WITH(Refine, c.sig = at(0x3008))), align);
    refuse("refine: out_scale + 8", call(WITH(Refine, c.scale = at(0x6008))), align);
    refuse("refine: index + 4", call(WITH(Refine, c.index = at(0x4004))), align);
    refuse("refine: out_delta + 4", call(WITH(Refine, c.delta = at(0x5004))), align);
    refuse("refine: out_score + 4", call(WITH(Refine, c.score = at(0x7004))), align);
    refuse("refine: no columns", call(WITH(Refine, c.rows = {})), W + ": nparam = 0 not in [1, 4]");
    refuse("refine: five columns", call(WITH(Refine, c.rows = {1, 2, 1, 2, 1})), W + ": nparam = 5 not in [1, 4]");
    refuse("refine: nrec = 0", call(WITH(Refine, c.nrec = 0)), W + ": nrec = 0, nrow = 3: both must be >= 1");
    refuse("refine: nrec = -3", call(WITH(Refine, c.nrec = -3)), W + ": nrec = -3, nrow = 3: both must be >= 1");
    refuse("refine: nrow = 0", call(WITH(Refine, c.nrow = 0)), W + ": nrec = 5, nrow = 0: both must be >= 1");
    refuse("refine: natoms = 0", call(WITH(Refine, c.natoms = 0)), W + ": natoms = 0 (>= 1), nmeas = 9 (>= 0)");
    refuse("refine: nmeas = -1", call(WITH(Refine, c.nmeas = -1)), W + ": natoms = 17 (>= 1), nmeas = -1 (>= 0)");
    refuse("refine: row_stride = natoms - 1", call(WITH(Refine, c.stride = 16)), W + ": 17 atoms outside a row of 16");
    refuse("refine: row_stride = 0", call(WITH(Refine, c.stride = 0)), W + ": 17 atoms outside a row of 0");
    refuse("refine: record_stride one short", call(WITH(Refine, c.rstride = 50)), W + ": record_stride = 50 holds fewer than nrow = 3 rows of 17");
    refuse("refine: record_stride = 2^62, nrec = 2^31 - 1", call(WITH(Refine, c.rstride = BIG, c.nrec = IMAX)),
           W + ": nrec = 2147483647 records of record_stride = 4611686018427387904 elements overflow the address range");
    accept("refine: Jacobian span == INT64_MAX / 16", call(WITH(Refine, c.nrec = 2, c.rstride = L16 - 51)));
    refuse("refine: Jacobian span one above", call(WITH(Refine, c.nrec = 2, c.rstride = L16 - 50)),
           W + ": nrec = 2 records of record_stride = 576460752303423437 elements overflow the address range");
    refuse("refine: sig_row_stride = nmeas - 1", call(WITH(Refine, c.sstride = 8)),
           W + ": 5 records of sig_row_stride = 8 do not hold 9 voxels each (or overflow the address range)");
    refuse("refine: sig_row_stride = 2^62, nrec = 2^31 - 1", call(WITH(Refine, c.sstride = BIG, c.nrec = IMAX)),
           W + ": 2147483647 records of sig_row_stride = 4611686018427387904 do not hold 9 voxels each (or overflow the address range)");
    refuse("refine: rows = (0, 1)", call(WITH(Refine, c.rows = {0, 1})), W + ": rows[0] = 0 not in [1, nrow = 3) (row 0 is the state)");
    refuse("refine: rows = (1, 3)", call(WITH(Refine, c.rows = {1, 3})), W + ": rows[1] = 3 not in [1, nrow = 3) (row 0 is the state)");
    refuse("refine: rows = (-1, 1)", call(WITH(Refine, c.rows = {-1, 1})), W + ": rows[0] = -1 not in [1, nrow = 3) (row 0 is the state)");
    refuse("refine: rows = (2, 2)", call(WITH(Refine, c.rows = {2, 2})), W + ": rows[0] = rows[1] = 2: a repeated row");
    refuse("refine: limit = (1, 0)", call(WITH(Refine, c.limit = {1.0, 0.0})), W + ": limit[1] = 0 is not positive");
    refuse("refine: limit = (-1, 1)", call(WITH(Refine, c.limit = {-1.0, 1.0})), W + ": limit[0] = -1 is not positive");
    refuse("refine: limit = (nan, 1)", call(WITH(Refine, c.limit = {NaN, 1.0})), W + ": limit[0] = nan is not positive");
    refuse("refine: rcond = -1e-3", call(WITH(Refine, c.rcond = -1e-3)), W + ": rcond = -0.001 not in [0, 1)");
    refuse("refine: rcond = 1", call(WITH(Refine, c.rcond = 1.0)), W + ": rcond = 1 not in [0, 1)");
    refuse("refine: rcond = nan", call(WITH(Refine, c.rcond = NaN)), W + ": rcond = nan not in [0, 1)");
    const int64_t many = (int64_t)64 * IMAX;
    accept("refine: nmeas / 64 = 0x7ffffffe", call(WITH(Refine, c.nrec = 1, c.sstride = many, c.nmeas = many - 1)));
    refuse("refine: nmeas / 64 = 0x7fffffff", call(WITH(Refine, c.nrec = 1, c.sstride = many, c.nmeas = many)), W + ": 137438953408 voxels in one call");
    refuse("refine: rcond is looked at before the rows", call(WITH(Refine, c.rcond = 1.0, c.rows = {0, 1})), W + ": rcond = 1 not in [0, 1)");
}

// ------------------------------------------------------------------ non-negative mixtures (tests/test_gpu_nnls.py, test_gpu_nnls_chi2.py)
struct Nnls {      // 8 records of 9 atoms: 3 components x 3 groups, 65 voxels
    int entry = 0;      // 0: epgx_signal_component_gram, 1: epgx_signal_nnls, 2: epgx_signal_nnls_chi2
    const void *ctx = at(0x100), *dict = at(0x1000), *gram = at(0x2000), *mask = at(0x3000), *sig = at(0x4000), *group = nullptr;
    const void *w = at(0x5000), *g = at(0x6000), *r = at(0x7000), *st = at(0x8000), *mu = at(0x9000), *ratio = at(0xa000), *ev = at(0xb000);
    int64_t stride = 9, astride = 3, nouter = 1, ninner = 3, sstride = 65, nmeas = 65;
    int32_t nrec = 8, A = 3, evals = 40;
    double reg = 1e-8, tol = 1e-10, chi2 = 1.02, rtol = 1e-3;
};
static const char *nnls_name(int entry) { return entry == 0 ? "epgx_signal_component_gram" : entry == 1 ? "epgx_signal_nnls" : "epgx_signal_nnls_chi2"; }
static int call(const Nnls &c) {      // the checks in the order in which the entry asks them
    g_err[0] = 0;
    const char *who = nnls_name(c.entry);
    if (c.entry == 0) return component_gram_check(who, c.dict, c.stride, c.nrec, c.A, c.astride, c.nouter, c.ninner, c.gram, c.mask);
    if (c.entry == 2)
        if (int rc = nnls_chi2_outputs_check(who, c.mu, c.ratio, c.ev)) return rc;
    if (int rc = nnls_check(who, c.ctx, c.dict, c.stride, c.nrec, c.A, c.astride, c.nouter, c.ninner, c.gram, c.mask, c.sig, c.sstride, c.nmeas, c.reg,
                            c.tol, c.group, c.w, c.g, c.r, c.st))
        return rc;
    return c.entry == 2 ? nnls_chi2_search_check(who, c.reg, c.chi2, c.rtol, c.evals) : EPGX_OK;
}
static void nnls() {
    for (int entry = 0; entry < 3; ++entry) {
        const std::string W = nnls_name(entry), tag = W.substr(12) + ": ";
        const std::string align = entry == 0 ? W + ": dict must be aligned to 16 bytes, out_gram and out_mask to 8"
                                             : W + ": dict and sig must be aligned to 16 bytes, out_status to 4, the others to 8";
#define C(...) call(WITH(Nnls, c.entry = entry, __VA_ARGS__))
        accept(tag + "the call of the GPU test", C((void)0));
        // the dictionary's shape: what all three share
        refuse(tag + "dict NULL", C(c.dict = 0), W + ": NULL argument");
        refuse(tag + "dict + 8", C(c.dict = at(0x1008)), align);
        refuse(tag + "ncomp = 0", C(c.A = 0), W + ": ncomp = 0 not in [1, 64]");
        refuse(tag + "ncomp = 65", C(c.A = 65), W + ": ncomp = 65 not in [1, 64]");
        refuse(tag + "ncomp = -1", C(c.A = -1), W + ": ncomp = -1 not in [1, 64]");
        accept(tag + "ncomp = 64", C(c.A = 64, c.astride = 3, c.stride = 64 * 3));
        refuse(tag + "nrec = 0", C(c.nrec = 0), W + ": nrec = 0 must be >= 1");
        refuse(tag + "nrec = -2", C(c.nrec = -2), W + ": nrec = -2 must be >= 1");
        refuse(tag + "nouter = 0", C(c.nouter = 0), W + ": nouter = 0, ninner = 3: both must be >= 1");
        refuse(tag + "ninner = 0", C(c.ninner = 0), W + ": nouter = 1, ninner = 0: both must be >= 1");
        refuse(tag + "axis_stride = -3", C(c.astride = -3), W + ": axis_stride = -3 below ninner = 3");
        refuse(tag + "axis_stride = 2", C(c.astride = 2), W + ": axis_stride = 2 below ninner = 3");
        refuse(tag + "row_stride = 8", C(c.stride = 8), W + ": 8 records of row_stride = 8 do not hold 1 x 3 atoms of stride 3 (or overflow the address range)");
        refuse(tag + "row_stride = -9", C(c.stride = -9), W + ": 8 records of row_stride = -9 do not hold 1 x 3 atoms of stride 3 (or overflow the address range)");
        refuse(tag + "row_stride = 2^62, nrec = 2^31 - 1", C(c.stride = BIG, c.nrec = IMAX),
               W + ": 2147483647 records of row_stride = 4611686018427387904 do not hold 1 x 3 atoms of stride 3 (or overflow the address range)");
        refuse(tag + "nouter = 2^62, ninner = 4", C(c.nouter = BIG, c.ninner = 4), W + ": axis_stride = 3 below ninner = 4");
        refuse(tag + "nouter = 2^62", C(c.nouter = BIG), W + ": nouter = 4611686018427387904 times ninner = 3 groups in one call");
        refuse(tag + "nouter = 2", C(c.nouter = 2), W + ": 8 records of row_stride = 9 do not hold 2 x 3 atoms of stride 3 (or overflow the address range)");
        accept(tag + "nouter = 2 in rows of 18", C(c.nouter = 2, c.stride = 18));
        refuse(tag + "nouter = 2 in rows of 17", C(c.nouter = 2, c.stride = 17),
               W + ": 8 records of row_stride = 17 do not hold 2 x 3 atoms of stride 3 (or overflow the address range)");
        // nouter * ninner groups at 0x7fffffff
        accept(tag + "0x7fffffff groups", C(c.nrec = 1, c.A = 1, c.astride = 1, c.ninner = 1, c.nouter = IMAX, c.stride = IMAX));
        refuse(tag + "0x80000000 groups", C(c.nrec = 1, c.A = 1, c.astride = 1, c.ninner = 1, c.nouter = (int64_t)IMAX + 1, c.stride = (int64_t)IMAX + 1),
               W + ": nouter = 2147483648 times ninner = 1 groups in one call");
        refuse(tag + "the last atom's column overflows", C(c.nrec = 1, c.nouter = IMAX / 3, c.astride = BIG, c.stride = INT64_MAX),
               W + ": 1 records of row_stride = 9223372036854775807 do not hold 715827882 x 3 atoms of stride 4611686018427387904 (or overflow the address range)");
        if (entry == 0) {
            refuse(tag + "out_gram NULL", C(c.gram = 0), W + ": NULL argument");
            refuse(tag + "out_mask NULL", C(c.mask = 0), W + ": NULL argument");
            refuse(tag + "out_gram + 4", C(c.gram = at(0x2004)), align);
            refuse(tag + "out_mask + 4", C(c.mask = at(0x3004)), align);
            continue;
        }
        // what epgx_signal_nnls adds
        accept(tag + "nmeas = 0", C(c.nmeas = 0));
        accept(tag + "nmeas = 0, sig_row_stride = 0", C(c.nmeas = 0, c.sstride = 0));
        accept(tag + "a group per voxel", C(c.group = at(0xc000)));
        for (int k = 0; k < 8; ++k)
            refuse(tag + "NULL argument " + std::to_string(k),
                   C(k == 0 ? (void)(c.gram = 0) : k == 1 ? (void)(c.mask = 0) : k == 2 ? (void)(c.sig = 0) : k == 3 ? (void)(c.w = 0) : k == 4 ? (void)(c.g = 0)
                     : k == 5 ? (void)(c.r = 0) : k == 6 ? (void)(c.st = 0) : (void)(c.ctx = 0)), W + ": NULL argument");
        refuse(tag + "sig + 8", C(c.sig = at(0x4008)), align);
        refuse(tag + "gram + 4", C(c.gram = at(0x2004)), align);
        refuse(tag + "mask + 4", C(c.mask = at(0x3004)), align);
        refuse(tag + "group + 4", C(c.group = at(0xc004)), align);
        refuse(tag + "out_weights + 4", C(c.w = at(0x5004)), align);
        refuse(tag + "out_group + 4", C(c.g = at(0x6004)), align);
        refuse(tag + "out_residual + 4", C(c.r = at(0x7004)), align);
        refuse(tag + "out_status + 2", C(c.st = at(0x8002)), align);
        accept(tag + "out_status + 4", C(c.st = at(0x8004)));
        refuse(tag + "nmeas = -1", C(c.nmeas = -1), W + ": nmeas = -1 must be >= 0");
        refuse(tag + "sig_row_stride = nmeas - 1", C(c.sstride = 64), W + ": 8 records of sig_row_stride = 64 do not hold 65 voxels each (or overflow the address range)");
        refuse(tag + "sig_row_stride = -1", C(c.sstride = -1), W + ": 8 records of sig_row_stride = -1 do not hold 65 voxels each (or overflow the address range)");
        refuse(tag + "sig_row_stride = 2^62, nrec = 2^31 - 1", C(c.sstride = BIG, c.nrec = IMAX),
               W + ": 2147483647 records of sig_row_stride = 4611686018427387904 do not hold 65 voxels each (or overflow the address range)");
        refuse(tag + "nmeas = 2^31", C(c.nmeas = (int64_t)1 << 31, c.sstride = (int64_t)1 << 31), W + ": 2147483648 voxels in one call");
        refuse(tag + "nmeas = 0x7fffffff", C(c.nmeas = IMAX, c.sstride = IMAX), W + ": 2147483647 voxels in one call");
        accept(tag + "nmeas = 0x7ffffffe", C(c.nmeas = IMAX - 1, c.sstride = IMAX));
        refuse(tag + "reg = -1e-9", C(c.reg = -1e-9), W + ": reg = -1e-09 is not a finite number >= 0");
        refuse(tag + "reg = nan", C(c.reg = NaN), W + ": reg = nan is not a finite number >= 0");
        refuse(tag + "reg = inf", C(c.reg = INF), W + ": reg = inf is not a finite number >= 0");
        refuse(tag + "tol = -1", C(c.tol = -1.0), W + ": tol = -1 is not a finite number >= 0");
        refuse(tag + "tol = nan", C(c.tol = NaN), W + ": tol = nan is not a finite number >= 0");
        refuse(tag + "tol = inf", C(c.tol = INF), W + ": tol = inf is not a finite number >= 0");
        if (entry == 1) {
            accept(tag + "a group per voxel, reg = tol = 0", C(c.group = at(0xc000), c.reg = 0.0, c.tol = 0.0));
            continue;
        }
        // what epgx_signal_nnls_chi2 adds: its outputs first, its parameters last
        const std::string mine = W + ": out_mu and out_chi2 must be aligned to 8 bytes, out_evals to 4";
        refuse(tag + "out_mu NULL", C(c.mu = 0), W + ": NULL argument");
        refuse(tag + "out_chi2 NULL", C(c.ratio = 0), W + ": NULL argument");
        refuse(tag + "out_evals NULL", C(c.ev = 0), W + ": NULL argument");
        refuse(tag + "out_mu + 4", C(c.mu = at(0x9004)), mine);
        refuse(tag + "out_chi2 + 4", C(c.ratio = at(0xa004)), mine);
        refuse(tag + "out_evals + 2", C(c.ev = at(0xb002)), mine);
        refuse(tag + "out_mu + 4 comes before dict + 8", C(c.mu = at(0x9004), c.dict = at(0x1008)), mine);
        refuse(tag + "reg = 0", C(c.reg = 0.0), W + ": reg = 0 must be > 0: the bracket grows from mu_0 = reg * mean H_aa");
        refuse(tag + "chi2 = 1", C(c.chi2 = 1.0), W + ": chi2 = 1 is not a finite number > 1");
        refuse(tag + "chi2 = 0", C(c.chi2 = 0.0), W + ": chi2 = 0 is not a finite number > 1");
        refuse(tag + "chi2 = nan", C(c.chi2 = NaN), W + ": chi2 = nan is not a finite number > 1");
        refuse(tag + "chi2 = inf", C(c.chi2 = INF), W + ": chi2 = inf is not a finite number > 1");
        refuse(tag + "chi2_rtol = 0", C(c.rtol = 0.0), W + ": chi2_rtol = 0 not in (0, 1)");
        refuse(tag + "chi2_rtol = 1", C(c.rtol = 1.0), W + ": chi2_rtol = 1 not in (0, 1)");
        refuse(tag + "chi2_rtol = nan", C(c.rtol = NaN), W + ": chi2_rtol = nan not in (0, 1)");
        refuse(tag + "max_evals = -1", C(c.evals = -1), W + ": max_evals = -1 not in [0, 40]");
        refuse(tag + "max_evals = 41", C(c.evals = 41), W + ": max_evals = 41 not in [0, 40]");
        accept(tag + "max_evals = 0", C(c.evals = 0));
        refuse(tag + "tol = -1 comes before chi2 = 1", C(c.tol = -1.0, c.chi2 = 1.0), W + ": tol = -1 is not a finite number >= 0");
#undef C
    }
}

// ------------------------------------------------------------------ dictionary compression (tests/test_gpu_compress.py)
struct Gram {      // 17 atoms x 5 records
    const void *dict = at(0x1000), *norms = at(0x2000), *out = at(0x3000);
    int64_t stride = 17, natoms = 17;
    int32_t nrec = 5, nsplit = 0;
};
static GramPlan gplan;
static int call(const Gram &c) {
    g_err[0] = 0;
    return gram_check("epgx_signal_gram", c.dict, c.stride, c.norms, c.nrec, c.natoms, c.nsplit, c.out, &gplan);
}
static bool gplan_is(int32_t nsplit, int32_t nblock, int32_t npair, int64_t scratch_len) {
    printf("   nsplit %d nblock %d npair %d scratch_len %lld\n", gplan.nsplit, gplan.nblock, gplan.npair, (long long)gplan.scratch_len);
    return gplan.nsplit == nsplit && gplan.nblock == nblock && gplan.npair == npair && gplan.scratch_len == scratch_len;
}
static void gram() {
    const std::string W = "epgx_signal_gram", align = W + ": dict and out must be aligned to 16 bytes, norms to 8";
    accept("gram: the call of the GPU test", call(Gram()));
    CHECK(gplan_is(1, 1, 1, 25));      // most = max(17 / 1024, 1) = 1
    accept("gram: nsplit = natoms", call(WITH(Gram, c.nsplit = 17)));
    CHECK(gplan_is(17, 1, 1, 17 * 25));
    refuse("gram: dict NULL", call(WITH(Gram, c.dict = 0)), W + ": NULL argument");
    refuse("gram: norms NULL", call(WITH(Gram, c.norms = 0)), W + ": NULL argument");
    refuse("gram: out NULL", call(WITH(Gram, c.out = 0)), W + ": NULL argument");
    refuse("gram: dict + 8", call(WITH(Gram, c.dict = at(0x1008))), align);
    refuse("gram: out + 8", call(WITH(Gram, c.out = at(0x3008))), align);
    refuse("gram: norms + 4", call(WITH(Gram, c.norms = at(0x2004))), align);
    refuse("gram: nrec = 0", call(WITH(Gram, c.nrec = 0)), W + ": nrec = 0, natoms = 17: both must be >= 1");
    refuse("gram: nrec = -2", call(WITH(Gram, c.nrec = -2)), W + ": nrec = -2, natoms = 17: both must be >= 1");
    refuse("gram: natoms = 0", call(WITH(Gram, c.natoms = 0)), W + ": nrec = 5, natoms = 0: both must be >= 1");
    refuse("gram: natoms = -1", call(WITH(Gram, c.natoms = -1)), W + ": nrec = 5, natoms = -1: both must be >= 1");
    refuse("gram: nsplit = -1", call(WITH(Gram, c.nsplit = -1)), W + ": nsplit = -1 not in [0, natoms = 17]");
    refuse("gram: nsplit = natoms + 1", call(WITH(Gram, c.nsplit = 18)), W + ": nsplit = 18 not in [0, natoms = 17]");
    refuse("gram: dict_row_stride = natoms - 1", call(WITH(Gram, c.stride = 16)),
           W + ": 5 records of dict_row_stride = 16 do not hold 17 atoms each (or overflow the address range)");
    refuse("gram: dict_row_stride = 2^62, nrec = 2^31 - 1", call(WITH(Gram, c.stride = BIG, c.nrec = IMAX)),
           W + ": 2147483647 records of dict_row_stride = 4611686018427387904 do not hold 17 atoms each (or overflow the address range)");
    refuse("gram: nrec = 2^31 - 1, nsplit = natoms", call(WITH(Gram, c.nrec = IMAX, c.nsplit = 17)),
           W + ": nsplit = 17 partial Gram matrices of 2147483647 x 2147483647 in one call");
    // the library's own nsplit = min(ceil(2048 / npair), max(natoms / 1024, 1)); blocks of 64 records
    accept("gram: 2047 atoms", call(WITH(Gram, c.natoms = c.stride = 2047)));
    CHECK(gplan_is(1, 1, 1, 25));
    accept("gram: 2048 atoms", call(WITH(Gram, c.natoms = c.stride = 2048)));
    CHECK(gplan_is(2, 1, 1, 50));
    accept("gram: 2^22 atoms x 64 records", call(WITH(Gram, c.natoms = c.stride = 1 << 22, c.nrec = 64)));
    CHECK(gplan_is(2048, 1, 1, (int64_t)2048 * 4096));
    accept("gram: 2^22 atoms x 65 records", call(WITH(Gram, c.natoms = c.stride = 1 << 22, c.nrec = 65)));
    CHECK(gplan_is(683, 2, 3, (int64_t)683 * 4225));      // ceil(2048 / 3)
    accept("gram: 2^20 atoms x 130 records", call(WITH(Gram, c.natoms = c.stride = 1 << 20, c.nrec = 130)));
    CHECK(gplan_is(342, 3, 6, (int64_t)342 * 16900));     // ceil(2048 / 6) below 1024
    // npair * nsplit workgroups at 0x7fffffff: 2^15 blocks give npair = 2^14 (2^15 + 1) = 536887296, times 4 = 0x80010000
    accept("gram: 2^21 records, nsplit = 3", call(WITH(Gram, c.nrec = 1 << 21, c.nsplit = 3)));
    CHECK(gplan_is(3, 1 << 15, 536887296, (int64_t)3 << 42));
    refuse("gram: 2^21 records, nsplit = 4", call(WITH(Gram, c.nrec = 1 << 21, c.nsplit = 4)),
           W + ": nsplit = 4 partial Gram matrices of 2097152 x 2097152 in one call");
}

struct Project {      // 17 columns x 5 records onto rank 3
    const void *basis = at(0x1000), *src = at(0x2000), *out = at(0x3000);
    int64_t sstride = 17, ncol = 17, ostride = 17;
    int32_t rank = 3, nrec = 5;
};
static int call(const Project &c) {
    g_err[0] = 0;
    return project_check("epgx_signal_project", c.basis, c.rank, c.src, c.sstride, c.nrec, c.ncol, c.out, c.ostride);
}
static void project() {
    const std::string W = "epgx_signal_project", align = W + ": basis, src and out must be aligned to 16 bytes";
    accept("project: the call of the GPU test", call(Project()));
    accept("project: ncol = 0", call(WITH(Project, c.ncol = 0)));
    accept("project: ncol = 0, strides 0", call(WITH(Project, c.ncol = 0, c.sstride = 0, c.ostride = 0)));
    accept("project: rank = nrec", call(WITH(Project, c.rank = 5)));
    accept("project: rank = 64", call(WITH(Project, c.rank = 64, c.nrec = 100)));
    refuse("project: basis NULL", call(WITH(Project, c.basis = 0)), W + ": NULL argument");
    refuse("project: src NULL", call(WITH(Project, c.src = 0)), W + ": NULL argument");
    refuse("project: out NULL", call(WITH(Project, c.out = 0)), W + ": NULL argument");
    refuse("project: basis + 8", call(WITH(Project, c.basis = at(0x1008))), align);
    refuse("project: src + 8", call(WITH(Project, c.src = at(0x2008))), align);
    refuse("project: out + 8", call(WITH(Project, c.out = at(0x3008))), align);
    refuse("project: nrec = 0", call(WITH(Project, c.nrec = 0)), W + ": nrec = 0 (>= 1), ncol = 17 (>= 0)");
    refuse("project: nrec = -1", call(WITH(Project, c.nrec = -1)), W + ": nrec = -1 (>= 1), ncol = 17 (>= 0)");
    refuse("project: ncol = -1", call(WITH(Project, c.ncol = -1)), W + ": nrec = 5 (>= 1), ncol = -1 (>= 0)");
    refuse("project: rank = 0", call(WITH(Project, c.rank = 0)), W + ": rank = 0 not in [1, min(64, nrec = 5)]");
    refuse("project: rank = -1", call(WITH(Project, c.rank = -1)), W + ": rank = -1 not in [1, min(64, nrec = 5)]");
    refuse("project: rank = 65, nrec = 100", call(WITH(Project, c.rank = 65, c.nrec = 100)), W + ": rank = 65 not in [1, min(64, nrec = 100)]");
    refuse("project: rank = nrec + 1", call(WITH(Project, c.rank = 6)), W + ": rank = 6 not in [1, min(64, nrec = 5)]");
    refuse("project: src_row_stride = ncol - 1", call(WITH(Project, c.sstride = 16)),
           W + ": 5 records of src_row_stride = 16 do not hold 17 columns each (or overflow the address range)");
    refuse("project: out_row_stride = ncol - 1", call(WITH(Project, c.ostride = 16)),
           W + ": 3 rows of out_row_stride = 16 do not hold 17 columns each (or overflow the address range)");
    refuse("project: src_row_stride = 2^62, nrec = 2^31 - 1", call(WITH(Project, c.sstride = BIG, c.nrec = IMAX)),
           W + ": 2147483647 records of src_row_stride = 4611686018427387904 do not hold 17 columns each (or overflow the address range)");
    refuse("project: out_row_stride = 2^62", call(WITH(Project, c.ostride = BIG)),
           W + ": 3 rows of out_row_stride = 4611686018427387904 do not hold 17 columns each (or overflow the address range)");
    accept("project: output extent == INT64_MAX / 16", call(WITH(Project, c.rank = 2, c.ostride = L16 - 17)));
    refuse("project: output extent one above", call(WITH(Project, c.rank = 2, c.ostride = L16 - 16)),
           W + ": 2 rows of out_row_stride = 576460752303423471 do not hold 17 columns each (or overflow the address range)");
    const int64_t many = (int64_t)64 * IMAX;      // ncol / (4 waves x 16 columns) at 0x7fffffff
    accept("project: ncol / 64 = 0x7ffffffe", call(WITH(Project, c.rank = 1, c.nrec = 1, c.sstride = c.ostride = many, c.ncol = many - 1)));
    refuse("project: ncol / 64 = 0x7fffffff", call(WITH(Project, c.rank = 1, c.nrec = 1, c.sstride = c.ostride = c.ncol = many)),
           W + ": ncol = 137438953408 columns in one call");
}

int main() {
    extents();
    crlb();
    crlb_grad();
    norms();
    match();
    refine();
    nnls();
    gram();
    project();
    printf("%d refusals, each with its code and message\n", n_refusals);
    printf("signal_check: all checks passed\n");
    return 0;
}

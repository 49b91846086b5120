// epgx_plan_check.cpp -- plan analysis on host data alone (epgx_plan_check.h).  Plain C++17, no HIP.
#include "epgx_plan_check.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <thread>
#include <utility>

namespace epgx {
namespace {

int ncoef_expected(int opcode) {
    switch (opcode) {
    case EPGX_OP_T: return 8;
    case EPGX_OP_MAT: return 10;  // 9 used, padded to 10
    case EPGX_OP_MAT0: return 14;
    case EPGX_OP_T0: return 12;
    case EPGX_OP_E: return 4;
    case EPGX_OP_PD: return 1;
    case EPGX_OP_D: case EPGX_OP_GS: return -1;  // depends on K: checked in epgx_run
    case EPGX_OP_X: return -1;                  // 3 N^2: checked with N below
    default: return 0;
    }
}

// is column `col` zero in entries [j0, j1) of a table with `ncol` doubles per entry?
bool column_zero(const double *tab, int64_t j0, int64_t j1, int ncol, int col) {
    for (int64_t j = j0; j < j1; ++j)
        if (tab[j * ncol + col] != 0.0) return false;
    return true;
}

// Zero patterns of rotation tables (they select shorter fma chains in the kernels):
//   1 "TX": Im m01 = Re m02 = Re m20 (= Re o0) = 0 -- rotations about x, phi = 0 or 180 deg
//   3 "TY": Im m01 = Im m02 = Im m20 (= Im o0) = 0 -- real matrices, phi = +-90 deg
// The reference computes e^{i phi} with phi in radians, so only phi = 0 gives exact zeros:
// cos(pi/2) = 6e-17, sin(pi) = 1.2e-16.  A component below 2^-48 (3.6e-15) of its own entry's
// modulus in EVERY entry of the table counts as the rounding residue it is and is cleared in the
// device copy of the table (Snap), so that every kernel sees exact zeros: a deviation
// of <= 4e-15 relative from the reference's arithmetic, against a parity bar of 1e-6.
// The partial of a rotation about x or y (10 per entry: ur ui pr pi qr qi tr ti c22) has the zero pattern of its operator:
//   1 = Im m00 = Im m01 = Re m02 = Re m20 = 0, 2 = all Im = 0 -- exact, or residues, which are cleared like those above.
struct ColPair { int v, w; };   // the column that must vanish, and the other component of the same complex entry
struct PatternCols {
    int n_common, n_each;
    ColPair common[2], x[3], y[3];   // tested for both patterns; for the x pattern; for the y pattern
};
PatternCols rotation_cols(int nc) { return {1, nc == 8 ? 2 : 3, {{2, 1}}, {{3, 4}, {5, 6}, {8, 9}}, {{4, 3}, {6, 5}, {9, 8}}}; }
const PatternCols partial_cols = {2, 2, {{1, 0}, {3, 2}}, {{4, 5}, {6, 7}}, {{5, 4}, {7, 6}}};

// 1: the x pattern holds in every entry, 2: the y pattern, 0: neither.  *snap_mask = the pattern's columns where it holds
// through residues only, 0 where through exact zeros
int scan_residues(const double *tab, int64_t entries, int nc, const PatternCols &pc, uint32_t *snap_mask) {
    const double tol = 1.0 / 281474976710656.0;   // 2^-48
    // is column p.v zero / a rounding residue?  (hypot only when needed)
    auto residue = [&](const double *c, ColPair p, bool &exact) {
        const double v = c[p.v];
        if (v == 0.0) return true;
        exact = false;
        return std::fabs(v) <= tol * std::hypot(v, c[p.w]);
    };
    bool hold[2] = {true, true}, exact[2] = {true, true};
    for (int64_t j = 0; j < entries && (hold[0] || hold[1]); ++j) {
        const double *c = tab + j * nc;
        bool common = true, exact_common = true;
        for (int k = 0; k < pc.n_common && common; ++k) common = residue(c, pc.common[k], exact_common);
        for (int side = 0; side < 2; ++side) {
            const ColPair *cols = side ? pc.y : pc.x;
            exact[side] = exact[side] && exact_common;
            hold[side] = hold[side] && common;
            for (int k = 0; k < pc.n_each && hold[side]; ++k) hold[side] = residue(c, cols[k], exact[side]);
        }
    }
    *snap_mask = 0;
    for (int side = 0; side < 2; ++side) {
        if (!hold[side]) continue;
        const ColPair *cols = side ? pc.y : pc.x;
        if (!exact[side]) {
            for (int k = 0; k < pc.n_common; ++k) *snap_mask |= 1u << pc.common[k].v;
            for (int k = 0; k < pc.n_each; ++k) *snap_mask |= 1u << cols[k].v;
        }
        return side + 1;
    }
    return 0;
}

struct Assembled { int32_t ncoef, space; bool im_zero; };   // im_zero: column 1 of a 4-column (relaxation) table is all zero

class Analysis {
public:
    Analysis(const epgx_plan_desc &d_, const epgx_plan_ext *ext_, const Knobs &kn_, PlanAnalysis &a)
        : d(d_), ext(ext_), kn(kn_), host(a.host), geo(a.geo), snaps(a.snaps), log_jobs(a.log_jobs), n_chain(ext_ ? ext_->n_chain : 0) {}
    int run();

private:
    const epgx_plan_desc &d;
    const epgx_plan_ext *ext;
    const Knobs &kn;
    PlanHost &host;
    PlanGeometry &geo;
    std::vector<Snap> &snaps;
    std::vector<LogJob> &log_jobs;
    const int n_chain;
    int64_t n_pool = 0;   // host part + device-generated part
    bool may_fold = false;

    std::map<int64_t, Assembled> assembled;            // epgx_assemble: dst_off -> what lies there
    std::map<int64_t, int32_t> chained;                // epgx_chain: dst_off -> dst_space
    std::map<int64_t, uint8_t> generated_pattern;      // epgx_fuse: dst_off -> zero pattern (1 / 3 / 0)
    std::map<int64_t, uint8_t> generated_dpattern;     // epgx_fuse_partial: dst_off -> 1 (phi = 0 pattern) / 2 (real matrix) / 0
    // a table referenced by many operators / recipes is scanned once (and snapped once)
    std::map<std::pair<int64_t, int32_t>, bool> e_real_known;
    std::map<std::pair<int64_t, int32_t>, uint8_t> scanned, dscanned;
    std::map<std::pair<int64_t, int64_t>, int32_t> log_seen;   // (e_off, de_off) -> index into host.logtabs

    bool space_ok(int sp) const { return sp >= -1 && sp < d.n_spaces; }
    bool is_assembled(int64_t off, int ncoef, int space) const {
        const auto hit = assembled.find(off);
        return hit != assembled.end() && hit->second.ncoef == ncoef && hit->second.space == space;
    }
    bool is_chained(const epgx_op &op) const {
        const auto hit = chained.find(op.coef_off);
        return op.opcode == EPGX_OP_MAT0 && hit != chained.end() && hit->second == op.space;
    }
    // does one of `sources` (index spaces) vary along an axis that `dst_space` does not?
    bool varies_beyond(int dst_space, std::initializer_list<int> sources) const {
        for (int dd = 0; dd < geo.ndim; ++dd)
            for (int sp : sources)
                if (geo.fixed_along(dst_space, dd) && geo.stride(sp, dd) != 0) return true;
        return false;
    }

    int check_descriptor();
    int derive_geometry();
    const char *check_assemble(const epgx_assemble &as, int64_t *src_entries) const;
    int check_assembled();
    const char *check_chain(const epgx_chain &ch) const;
    int check_chains();
    const char *check_operator(const epgx_op &op);
    int check_operators();
    int check_second_order();
    const char *check_partial(const epgx_op &op, const epgx_dop &dp, int v) const;
    int check_derivatives();
    const char *check_fuse(const epgx_fuse &fu);
    int check_fuses();
    const char *check_fuse_partial(const epgx_fuse_partial &fp);
    int check_fuse_partials();
    bool e_is_real(int64_t off, int space);
    uint8_t t_pattern_once(int64_t off, int space, int nc);
    uint8_t d_pattern_once(int64_t off, int sp, bool is_e);
    int operator_patterns();
    int partial_patterns();
    int copy_gather_tables();
    int32_t log_table(int64_t e_off, int64_t de_off, int space);
    std::pair<int32_t, int32_t> walk_fuse_partials(int64_t doff, const std::map<int64_t, int> &recipe_of);
    void layout_log_tables();
};

int Analysis::check_descriptor() {
    if (d.n_ops <= 0 || !d.ops) return fail(EPGX_ERR_INVALID, "epgx_plan_create: empty operator list");
    if (d.ndim < 1 || d.ndim > EPGX_MAX_DIMS || !d.grid_shape)
        return fail(EPGX_ERR_INVALID, "epgx_plan_create: ndim %d not in [1,%d]", d.ndim, EPGX_MAX_DIMS);
    if (d.n_spaces < 0 || d.n_spaces > EPGX_MAX_SPACES || (d.n_spaces && !d.space_strides))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: %d index spaces, at most %d supported",
                    d.n_spaces, EPGX_MAX_SPACES);
    if (d.n_coef < 0 || (d.n_coef && !d.coef)) return fail(EPGX_ERR_INVALID, "epgx_plan_create: bad coefficient pool");
    if (d.n_coef_generated < 0 || d.n_fuse < 0 || (d.n_fuse && !d.fuse) || d.n_assemble < 0 || (d.n_assemble && !d.assemble))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create: bad generated-table description");
    n_pool = d.n_coef + d.n_coef_generated;
    if (n_pool >= ((int64_t)1 << 29) - 16)
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: coefficient pool larger than 4 GiB (split the grid)");
    if (d.n_adc < 0) return fail(EPGX_ERR_INVALID, "epgx_plan_create: n_adc < 0");
    if (d.deriv_flags & EPGX_DERIV_SECOND) {   // a one-pair second-order pass (hess_kernel): what such a plan cannot carry, before its lists are read
        if (d.n_vars != 2 && d.n_vars != 3)
            return fail(EPGX_ERR_INVALID, "epgx_plan_create: EPGX_DERIV_SECOND needs n_vars = 3 (S_a, S_b, H_ab) or 2 (S_a, H_aa), got %d", d.n_vars);
        if (!d.dops) return fail(EPGX_ERR_INVALID, "epgx_plan_create: EPGX_DERIV_SECOND without dops");
        if (!(d.deriv_flags & EPGX_PLAN_NO_FOLD))
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: EPGX_DERIV_SECOND without EPGX_PLAN_NO_FOLD: the run-time fold implements the first-order product rule only");
        if (d.n_fuse > 0 || d.n_fuse_partial > 0)
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: EPGX_DERIV_SECOND with device-generated tables (n_fuse, n_fuse_partial): epgx_fuse_partial implements the first-order product rule only");
        if (n_chain > 0)
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: EPGX_DERIV_SECOND with chains: a collapsed run of operators has no second-order partials");
    }
    host.n_spaces = d.n_spaces;
    host.n_pool = n_pool;
    may_fold = kn.fold && !(d.deriv_flags & EPGX_PLAN_NO_FOLD);   // (EPGX_FOLD=0: measurements)
    return EPGX_OK;
}

int Analysis::derive_geometry() {
    geo.ndim = d.ndim;
    int64_t nvox = 1;
    for (int i = 0; i < EPGX_MAX_DIMS; ++i) geo.shape[i] = 1;
    for (int i = 0; i < d.ndim; ++i) {
        if (d.grid_shape[i] < 1) return fail(EPGX_ERR_INVALID, "epgx_plan_create: grid_shape[%d] < 1", i);
        geo.shape[i] = d.grid_shape[i];
        nvox *= d.grid_shape[i];
        if (nvox > (int64_t)1 << 40) return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: grid too large");
    }
    geo.nvox_total = nvox;
    for (int s = 0; s < d.n_spaces; ++s) {
        int64_t extent = 0;
        for (int i = 0; i < d.ndim; ++i) {
            const int64_t st = d.space_strides[(size_t)s * EPGX_MAX_DIMS + i];
            if (st < 0) return fail(EPGX_ERR_INVALID, "epgx_plan_create: negative stride in space %d", s);
            geo.strides[s][i] = st;
            extent += (geo.shape[i] - 1) * st;
        }
        if (extent >= ((int64_t)1 << 31)) return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: table of space %d too large", s);
        geo.space_extent[s] = extent;
        bool dense = true;  // C-order strides of the full grid (axes of extent 1 are irrelevant)
        int64_t acc = 1;
        for (int i = d.ndim - 1; i >= 0; --i) {
            if (geo.shape[i] > 1 && geo.strides[s][i] != acc) dense = false;
            acc *= geo.shape[i];
        }
        if (dense) geo.dense_spaces |= 1u << s;
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ recipes the operators may refer to
const char *Analysis::check_assemble(const epgx_assemble &as, int64_t *src_entries) const {
    if (as.dst_space < -1 || as.dst_space >= d.n_spaces) return "index space out of range";
    if (as.ncoef < 1 || as.ncoef > EPGX_MAX_ASM_COLS || as.n_src < 1 || as.n_src > EPGX_MAX_ASM_SRC) return "bad column / source count";
    if (as.dst_off < d.n_coef || as.dst_off + geo.entries(as.dst_space) * as.ncoef > n_pool) return "destination outside the generated part of the pool";
    for (int k = 0; k < as.n_src; ++k) {
        const epgx_asm_src &sr = as.src[k];
        int64_t last = 0;
        for (int dd = 0; dd < d.ndim; ++dd) {
            if (sr.strides[dd] < 0) return "negative source stride";
            if (sr.strides[dd] != 0 && geo.fixed_along(as.dst_space, dd)) return "a source varies along an axis the destination does not";
            last += (geo.shape[dd] - 1) * sr.strides[dd];
        }
        if (sr.ncol < 1 || sr.off < 0 || sr.off + (last + 1) * sr.ncol > d.n_coef) return "source columns outside the host part of the pool";
        src_entries[k] = last + 1;
    }
    for (int c = 0; c < as.ncoef; ++c)
        if (as.col_src[c] >= as.n_src || as.col_idx[c] >= as.src[as.col_src[c]].ncol) return "column refers to a missing source column";
    return nullptr;
}

// device-assembled tables (epgx_assemble): checked first, operators and fuse recipes may refer to them
int Analysis::check_assembled() {
    for (int i = 0; i < d.n_assemble; ++i) {
        const epgx_assemble &as = d.assemble[i];
        int64_t src_entries[EPGX_MAX_ASM_SRC] = {0, 0, 0, 0};
        if (const char *why = check_assemble(as, src_entries)) return fail(EPGX_ERR_INVALID, "epgx_plan_create: assembled table %d: %s", i, why);
        bool im_zero = false;
        if (as.ncoef == 4) {   // relaxation layout: is Im e0 (column 1) zero in every entry?
            const epgx_asm_src &sr = as.src[as.col_src[1]];
            im_zero = column_zero(d.coef + sr.off, 0, src_entries[as.col_src[1]], sr.ncol, as.col_idx[1]);
        }
        assembled[as.dst_off] = {as.ncoef, as.dst_space, im_zero};
    }
    return EPGX_OK;
}

const char *Analysis::check_chain(const epgx_chain &ch) const {
    if (!space_ok(ch.dst_space)) return "index space of the destination out of range";
    if (ch.n_steps < 1 || !ch.steps) return "no steps";
    if (ch.dst_off < d.n_coef || ch.dst_off + geo.entries(ch.dst_space) * 14 > n_pool) return "destination outside the generated part of the pool";
    int64_t reps = 1;   // repetitions of the group the current step belongs to
    for (int k = 0, left = 0; k < ch.n_steps; ++k, --left) {
        const epgx_chain_step &st = ch.steps[k];
        if (left == 0) {   // first step of a group
            if (st.group < 1 || st.group > EPGX_CHAIN_GROUP || k + st.group > ch.n_steps || st.count < 1) return "malformed group (1 .. EPGX_CHAIN_GROUP steps inside the list, count >= 1)";
            left = st.group;
            reps = st.count;
        }
        const int nc = st.kind == EPGX_OP_T ? 8 : (st.kind == EPGX_OP_MAT ? 10 : (st.kind == EPGX_OP_MAT0 ? 14 : (st.kind == EPGX_OP_E ? 4 : 0)));
        if (!nc) return "unknown kind of source (EPGX_OP_T, EPGX_OP_MAT, EPGX_OP_MAT0 or EPGX_OP_E)";
        if (!space_ok(st.space)) return "index space of a source out of range";
        if (st.off < 0 || st.stride < 0) return "negative source offset or stride";
        if (!(is_assembled(st.off, nc, st.space) && (st.stride == 0 || reps == 1)) &&
            st.off + (reps - 1) * st.stride + geo.entries(st.space) * nc > d.n_coef)
            return "source neither inside the host part of the pool nor an assembled table";
        if (varies_beyond(ch.dst_space, {st.space})) return "a source varies along an axis the destination does not";
    }
    return nullptr;
}

// device-collapsed tables (epgx_chain): EPGX_OP_MAT0 operators may refer to their destinations
int Analysis::check_chains() {
    for (int i = 0; i < n_chain; ++i) {
        const epgx_chain &ch = ext->chain[i];
        if (const char *why = check_chain(ch)) return fail(EPGX_ERR_INVALID, "epgx_plan_create: collapsed table %d: %s", i, why);
        chained[ch.dst_off] = ch.dst_space;
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ operators and their partials
const char *Analysis::check_operator(const epgx_op &op) {
    if (op.opcode < 0 || op.opcode >= EPGX_OP__COUNT) return "unknown opcode";
    const int need = ncoef_expected(op.opcode);
    if (need >= 0 && op.ncoef != need) return "wrong ncoef for opcode";
    if (need < 0 && op.ncoef <= 0) return "table-driven operator without a table";
    if (need) {
        if (op.space < -1 || op.space >= d.n_spaces) return "index space out of range";
        if (op.coef_off < 0 || op.coef_off + geo.entries(op.space) * (int64_t)op.ncoef > n_pool) return "coefficient table exceeds the pool";
        if (op.opcode != EPGX_OP_T0 && !is_assembled(op.coef_off, op.ncoef, op.space) && !is_chained(op) &&
            op.coef_off + geo.entries(op.space) * (int64_t)op.ncoef > d.n_coef)
            return "a table in the generated part of the pool needs a recipe (epgx_assemble, epgx_chain for EPGX_OP_MAT0, or epgx_fuse for EPGX_OP_T0)";
    }
    const char *why = nullptr;   // (within an operator's own block the LAST failing check names the refusal)
    if (op.opcode == EPGX_OP_S) {
        if (op.ia == 0) why = "shift by 0";
        if (op.ia >= EPGX_MAX_K || op.ia <= -EPGX_MAX_K) why = "shift exceeds EPGX_MAX_K";
        if (op.ib < 0) why = "negative truncation order";
    }
    if (op.opcode == EPGX_OP_X) {
        // N compartments at stride ib: the grid axis of extent N behind which the grid holds ib voxels
        int ax = -1;
        int64_t behind = 1;
        for (int dd = d.ndim - 1; dd >= 0 && ax < 0; --dd) {
            if (geo.shape[dd] == op.ia && behind == op.ib) ax = dd;
            behind *= geo.shape[dd];
        }
        if (op.ia < 2 || op.ia > 8) why = "exchange between 2 .. 8 compartments";
        else if (op.ncoef != 3 * op.ia * op.ia) why = "X table needs 3 N^2 doubles per entry";
        else if (ax < 0) why = "no grid axis of extent N = ia with ib voxels behind it";
        else if (geo.x_span && geo.x_span != (int64_t)op.ia * op.ib) why = "X operators of one plan must share N and the compartment axis";
        else {
            geo.x_span = (int64_t)op.ia * op.ib;
            geo.x_ncomp = op.ia;
        }
    }
    if (op.opcode == EPGX_OP_ADC) {
        if (op.ia < 0 || op.ia >= d.n_adc) why = "ADC slot out of range";
        if (op.ib != 0 && op.ib != 1) why = "unknown ADC probe";
    }
    return why;
}

int Analysis::check_operators() {
    host.ops.assign(d.ops, d.ops + d.n_ops);
    for (int i = 0; i < d.n_ops; ++i)
        if (const char *why = check_operator(host.ops[i]))
            return fail(EPGX_ERR_INVALID, "epgx_plan_create: operator %d (opcode %d): %s", i, host.ops[i].opcode, why);
    return EPGX_OK;
}

// a one-pair second-order pass (hess_kernel)
int Analysis::check_second_order() {
    for (int i = 0; i < d.n_ops; ++i) {
        const epgx_dop &dp = d.dops[i];
        if (host.ops[i].opcode == EPGX_OP_T0)
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: %s", "EPGX_DERIV_SECOND with an EPGX_OP_T0 operator: the constant term of a fused table has no second-order partial");
        if (host.ops[i].opcode == EPGX_OP_X) return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: %s", "EPGX_DERIV_SECOND with exchange (EPGX_OP_X)");
        if ((dp.reserved & ~(EPGX_HESS_CROSS_A | EPGX_HESS_CROSS_B)) || ((dp.reserved & EPGX_HESS_CROSS_A) && dp.coef_off[0] < 0) ||
            ((dp.reserved & EPGX_HESS_CROSS_B) && (d.n_vars != 3 || dp.coef_off[1] < 0)))
            return fail(EPGX_ERR_INVALID, "epgx_plan_create: %s", "EPGX_DERIV_SECOND: a cross-term bit (epgx_dop::reserved) without its first-order partial");
    }
    host.second = true;
    return EPGX_OK;
}

const char *Analysis::check_partial(const epgx_op &op, const epgx_dop &dp, int v) const {
    const int64_t off = dp.coef_off[v];
    int nc = 0;
    if (v >= d.n_vars) return "partial for a variable beyond n_vars";
    else if (op.opcode == EPGX_OP_T || op.opcode == EPGX_OP_MAT || op.opcode == EPGX_OP_MAT0 || op.opcode == EPGX_OP_T0) nc = 10;
    else if (op.opcode == EPGX_OP_E) nc = 4;
    else if (op.opcode == EPGX_OP_X) nc = op.ncoef;   // d mT, d mL in the layout of X's own table (3 N^2 per group)
    else return "only T / MAT / E operators can carry partial derivatives";   // (and X, above)
    const int sp = dp.space[v];
    if (!space_ok(sp)) return "index space of a partial out of range";
    if (op.opcode == EPGX_OP_T0 && off >= d.n_coef) {   // generated next to the table itself (epgx_fuse_partial)
        if (off + geo.entries(sp) * 14 > n_pool) return "generated partial table exceeds the pool";
    } else if (is_assembled(off, nc, sp)) {              // assembled on the device from per-axis columns (epgx_assemble)
    } else if (off + geo.entries(sp) * nc > d.n_coef) return "partial table exceeds the host part of the pool";
    return nullptr;
}

int Analysis::check_derivatives() {
    if (d.n_vars < 0 || d.n_vars > EPGX_MAX_VARS || (d.n_vars > 0 && !d.dops))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create: n_vars=%d (at most %d) or dops missing", d.n_vars, EPGX_MAX_VARS);
    host.n_vars = d.n_vars;
    if (d.deriv_flags & EPGX_DERIV_SECOND)
        if (int rc = check_second_order()) return rc;
    host.fold = may_fold && d.n_vars == 0;
    if (d.n_vars == 0) return EPGX_OK;
    host.dops.assign(d.dops, d.dops + d.n_ops);
    for (int i = 0; i < d.n_ops; ++i) {
        const epgx_op &op = host.ops[i];
        for (int v = 0; v < EPGX_MAX_VARS; ++v) {
            if (host.dops[i].coef_off[v] < 0) continue;
            if (const char *why = check_partial(op, host.dops[i], v))
                return fail(EPGX_ERR_INVALID, "epgx_plan_create: operator %d, variable %d: %s", i, v, why);
        }
        if (op.opcode == EPGX_OP_ADC && op.ia + d.n_vars >= d.n_adc)
            return fail(EPGX_ERR_INVALID, "epgx_plan_create: operator %d: ADC rows [%d,%d] exceed n_adc=%d", i,
                        op.ia, op.ia + d.n_vars, d.n_adc);
        // dxrun_kernel<N, K / 64, V> keeps N K / 64 (1 + V) <= 8 state matrices of 64 orders in registers: at K = 64 already ...
        if (op.opcode == EPGX_OP_X && !xrun_deriv_fits(op.ia, 64, d.n_vars))
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: operator %d: exchange (EPGX_OP_X) between %d compartments with %d derivative "
                        "state(s): the fused kernel holds N * (K / 64) * (1 + n_vars) <= 8 with N <= 4 (no split path for derivatives)", i, op.ia, d.n_vars);
        // ... and the constant term of a generated EPGX_OP_T0 partial (14 per entry) is not read there
        if (geo.x_span && op.opcode == EPGX_OP_T0)
            for (int v = 0; v < d.n_vars; ++v)
                if (host.dops[i].coef_off[v] >= d.n_coef)
                    return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: operator %d: a generated partial (epgx_fuse_partial) in a plan with exchange "
                                "(EPGX_OP_X): keep the relaxations stages of their own", i);
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ scans of the pool's host part
// relaxation table without a precession term (Im e0 == 0 in every entry)?  Scanned once per table; a table over a
// 1024 x 1024 grid is 34 MB, so large tables are split over a few threads
bool Analysis::e_is_real(int64_t off, int space) {
    if (off >= d.n_coef) {   // assembled on the device: known from its column
        const auto as = assembled.find(off);
        return as != assembled.end() && as->second.ncoef == 4 && as->second.im_zero;
    }
    const auto key = std::make_pair(off, (int32_t)(space + 1));
    const auto hit = e_real_known.find(key);
    if (hit != e_real_known.end()) return hit->second;
    const int64_t entries = geo.entries(space);
    const double *tab = d.coef + off;
    std::atomic<bool> real{true};
    auto scan = [&](int64_t j0, int64_t j1) {
        if (!column_zero(tab, j0, j1, 4, 1)) real.store(false, std::memory_order_relaxed);
    };
    const int nthreads = entries >= (1 << 17) ? 4 : 1;
    if (nthreads == 1) scan(0, entries);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nthreads; ++t) pool.emplace_back(scan, entries * t / nthreads, entries * (t + 1) / nthreads);
        for (auto &th : pool) th.join();
    }
    e_real_known[key] = real.load();
    return real.load();
}

// zero pattern of a rotation table in the host part of the pool: 1 (TX), 3 (TY) or 0
uint8_t Analysis::t_pattern_once(int64_t off, int space, int nc) {
    const auto key = std::make_pair(off, (int32_t)(nc * 8 + space + 1));
    const auto hit = scanned.find(key);
    if (hit != scanned.end()) return hit->second;
    const int64_t entries = geo.entries(space);
    uint32_t mask = 0;
    const int side = scan_residues(d.coef + off, entries, nc, rotation_cols(nc), &mask);
    if (mask) snaps.push_back({off, entries, nc, mask});
    return scanned[key] = (uint8_t)(side == 2 ? 3 : side);
}

// zero pattern of a partial-derivative table (scanned once per table):
//   relaxation (4 per entry):  1 = Im d e0 = 0 in every entry
//   rotation (10 per entry):   1 / 2 = the pattern of a rotation about x / y (scan_residues)
uint8_t Analysis::d_pattern_once(int64_t off, int sp, bool is_e) {
    const auto key = std::make_pair(off, (int32_t)((is_e ? 8 : 0) + sp + 1));
    const auto hit = dscanned.find(key);
    if (hit != dscanned.end()) return hit->second;
    if (off >= d.n_coef) {   // assembled on the device: a relaxation partial's pattern is known from its column, a rotation's is general
        const auto as = assembled.find(off);
        return dscanned[key] = (is_e && as != assembled.end() && as->second.ncoef == 4 && as->second.im_zero) ? 1 : 0;
    }
    const int64_t entries = geo.entries(sp);
    if (is_e) return dscanned[key] = column_zero(d.coef + off, 0, entries, 4, 1) ? 1 : 0;
    uint32_t mask = 0;
    const int side = scan_residues(d.coef + off, entries, 10, partial_cols, &mask);
    if (mask) snaps.push_back({off, entries, 10, mask});
    return dscanned[key] = (uint8_t)side;
}

// ------------------------------------------------------------------------------ device-generated tables
const char *Analysis::check_fuse(const epgx_fuse &fu) {
    if (!space_ok(fu.dst_space) || !space_ok(fu.src_space) || !space_ok(fu.e_space)) return "index space out of range";
    if (fu.src_ncoef != 8 && fu.src_ncoef != 12) return "source must have 8 or 12 coefficients";
    if (fu.dst_off < d.n_coef || fu.dst_off + geo.entries(fu.dst_space) * 12 > n_pool) return "destination outside the generated part of the pool";
    if (!is_assembled(fu.e_off, 4, fu.e_space) && (fu.e_off < 0 || fu.e_off + geo.entries(fu.e_space) * 4 > d.n_coef))
        return "E source neither in the host part of the pool nor an assembled table";
    if (fu.src_off < 0 || fu.src_off + geo.entries(fu.src_space) * fu.src_ncoef > n_pool) return "rotation source outside the pool";
    if (fu.src_off >= d.n_coef && (fu.src_ncoef != 12 || !generated_pattern.count(fu.src_off))) return "a generated source must be the destination of an earlier entry";
    if (varies_beyond(fu.dst_space, {fu.src_space, fu.e_space})) return "a source varies along an axis the destination does not";
    if (!e_is_real(fu.e_off, fu.e_space)) return "E source has a precession term (Im e0 != 0)";
    return nullptr;
}

// epgx_fuse: the references, then the destination's zero pattern from its source's
int Analysis::check_fuses() {
    for (int i = 0; i < d.n_fuse; ++i) {
        const epgx_fuse &fu = d.fuse[i];
        if (const char *why = check_fuse(fu)) return fail(EPGX_ERR_INVALID, "epgx_plan_create: generated table %d: %s", i, why);
        generated_pattern[fu.dst_off] = fu.src_off >= d.n_coef ? generated_pattern[fu.src_off]
                                                                : t_pattern_once(fu.src_off, fu.src_space, fu.src_ncoef);
    }
    return EPGX_OK;
}

const char *Analysis::check_fuse_partial(const epgx_fuse_partial &fp) {
    const bool has_dt = fp.dsrc_off >= 0, has_de = fp.de_off >= 0;
    if (!space_ok(fp.dst_space) || !space_ok(fp.src_space) || !space_ok(fp.e_space) || (has_dt && !space_ok(fp.dsrc_space)) ||
        (has_de && !space_ok(fp.de_space)))
        return "index space out of range";
    if (!has_dt && !has_de) return "neither the rotation nor the relaxation has a partial";
    if (fp.src_ncoef != 8 && fp.src_ncoef != 12) return "rotation source must have 8 or 12 coefficients";
    if (has_dt && fp.dsrc_ncoef != 10 && fp.dsrc_ncoef != 14) return "rotation partial must have 10 or 14 coefficients";
    if (fp.dst_off < d.n_coef || fp.dst_off + geo.entries(fp.dst_space) * 14 > n_pool) return "destination outside the generated part of the pool";
    if (fp.src_off < 0 || fp.src_off + geo.entries(fp.src_space) * fp.src_ncoef > n_pool) return "rotation source outside the pool";
    if (fp.src_off >= d.n_coef && (fp.src_ncoef != 12 || !generated_pattern.count(fp.src_off)))
        return "a generated rotation source must be the destination of an entry of `fuse`";
    if (!is_assembled(fp.e_off, 4, fp.e_space) && (fp.e_off < 0 || fp.e_off + geo.entries(fp.e_space) * 4 > d.n_coef))
        return "E source neither in the host part of the pool nor an assembled table";
    if (!e_is_real(fp.e_off, fp.e_space)) return "E source has a precession term (Im e0 != 0)";
    if (has_dt && (fp.dsrc_ncoef == 10 ? fp.dsrc_off + geo.entries(fp.dsrc_space) * 10 > d.n_coef
                                       : (fp.dsrc_off < d.n_coef || !generated_dpattern.count(fp.dsrc_off) ||
                                          fp.dsrc_off + geo.entries(fp.dsrc_space) * 14 > n_pool)))
        return "rotation partial: 10 per entry in the host part of the pool, or 14 per entry written by an earlier entry";
    if (has_de && !is_assembled(fp.de_off, 4, fp.de_space) && fp.de_off + geo.entries(fp.de_space) * 4 > d.n_coef)
        return "E partial outside the host part of the pool (and not an assembled table)";
    if (has_de && d_pattern_once(fp.de_off, fp.de_space, true) != 1) return "E partial has a precession term (Im d e0 != 0)";
    if (varies_beyond(fp.dst_space, {fp.src_space, fp.e_space, has_dt ? fp.dsrc_space : -1, has_de ? fp.de_space : -1}))
        return "a source varies along an axis the destination does not";
    return nullptr;
}

// partials of generated tables (epgx_fuse_partial): the references, then the zero pattern from the sources'
int Analysis::check_fuse_partials() {
    if (d.n_fuse_partial < 0 || (d.n_fuse_partial > 0 && (!d.fuse_partial || d.n_vars == 0)))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create: n_fuse_partial=%d without a list or without variables", d.n_fuse_partial);
    for (int i = 0; i < d.n_fuse_partial; ++i) {
        const epgx_fuse_partial &fp = d.fuse_partial[i];
        if (const char *why = check_fuse_partial(fp)) return fail(EPGX_ERR_INVALID, "epgx_plan_create: generated partial %d: %s", i, why);
        const uint8_t vp = fp.src_off >= d.n_coef ? generated_pattern[fp.src_off] : t_pattern_once(fp.src_off, fp.src_space, fp.src_ncoef);
        const uint8_t dp = fp.dsrc_off < 0 ? (uint8_t)255 : (fp.dsrc_ncoef == 14 ? generated_dpattern[fp.dsrc_off] : d_pattern_once(fp.dsrc_off, fp.dsrc_space, false));
        generated_dpattern[fp.dst_off] = (vp == 1 && (dp == 1 || dp == 255)) ? 1 : ((vp == 3 && (dp == 2 || dp == 255)) ? 2 : 0);
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ what the plan keeps
// exact-zero patterns that let the kernel drop products without changing a single bit:
// T(alpha, 0): Im m01 = Re m02 = Re m20 = 0;  E with g = 0: Im e0 = 0
int Analysis::operator_patterns() {
    host.zero_pattern.assign((size_t)d.n_ops, 0);
    for (int i = 0; i < d.n_ops; ++i) {
        const epgx_op &op = host.ops[i];
        if (op.opcode != EPGX_OP_T && op.opcode != EPGX_OP_T0 && op.opcode != EPGX_OP_E) continue;
        if (op.opcode == EPGX_OP_E) {
            host.zero_pattern[i] = e_is_real(op.coef_off, op.space) ? 2 : 0;
            continue;
        }
        if (op.coef_off >= d.n_coef && op.opcode != EPGX_OP_T0 && is_assembled(op.coef_off, op.ncoef, op.space)) {
            host.zero_pattern[i] = 0;   // an assembled rotation table: general chains (no host copy to scan)
            continue;
        }
        if (op.coef_off >= d.n_coef) {   // generated on the device: pattern known from its sources
            const auto g = generated_pattern.find(op.coef_off);
            if (g == generated_pattern.end() || op.opcode != EPGX_OP_T0)
                return fail(EPGX_ERR_INVALID, "epgx_plan_create: operator %d refers to the generated part of the pool but no entry of `fuse` writes there", i);
            host.zero_pattern[i] = g->second;
            continue;
        }
        host.zero_pattern[i] = t_pattern_once(op.coef_off, op.space, op.ncoef);
    }
    return EPGX_OK;
}

int Analysis::partial_patterns() {
    if (d.n_vars == 0) return EPGX_OK;
    host.dpattern.assign((size_t)d.n_ops, 0);
    for (int i = 0; i < d.n_ops; ++i)
        for (int v = 0; v < d.n_vars; ++v) {
            const int64_t off = host.dops[i].coef_off[v];
            if (off < 0 || host.ops[i].opcode == EPGX_OP_X) continue;   // (X: no zero pattern is used)
            if (off >= d.n_coef && host.ops[i].opcode == EPGX_OP_T0) {   // a generated partial (checked above): pattern known from its sources
                const auto g = generated_dpattern.find(off);
                if (g == generated_dpattern.end())
                    return fail(EPGX_ERR_INVALID, "epgx_plan_create: operator %d, variable %d: the partial refers to the generated part of the pool but no entry of `fuse_partial` writes there", i, v);
                host.dpattern[i] |= (uint16_t)(((g->second & 3u) << (2 * v)) | (256u << v));
                continue;
            }
            host.dpattern[i] |= (uint16_t)((d_pattern_once(off, host.dops[i].space[v], host.ops[i].opcode == EPGX_OP_E) & 3u) << (2 * v));
        }
    return EPGX_OK;
}

int Analysis::copy_gather_tables() {
    host.gather_tables.resize((size_t)d.n_ops);
    for (int i = 0; i < d.n_ops; ++i) {
        const epgx_op &op = host.ops[i];
        if (op.opcode != EPGX_OP_GS) continue;
        if (op.space >= 0) return fail(EPGX_ERR_UNSUPPORTED, "epgx_plan_create: operator %d: gather shifts must be the same for all voxels", i);
        const int32_t *src = (const int32_t *)(d.coef + op.coef_off);
        host.gather_tables[i].assign(src, src + 2 * (size_t)op.ncoef);
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ tables of logarithmic partials
// the log table of (relaxation table, its partial), registered behind the pool's padding on first use
int32_t Analysis::log_table(int64_t e_off, int64_t de_off, int space) {
    const auto key = std::make_pair(e_off, de_off);
    const auto it = log_seen.find(key);
    if (it != log_seen.end()) return it->second;
    LogTab lt;
    lt.off = n_pool + 32 + host.n_log;
    lt.space = space;
    const int64_t entries = geo.entries(space);
    host.n_log += 2 * entries;
    log_jobs.push_back({e_off, de_off, entries});
    host.logtabs.push_back(lt);
    return log_seen[key] = (int32_t)host.logtabs.size() - 1;
}

// the epgx_fuse_partial chain behind the generated partial at `doff`: the log tables of E_a and E_b (-1: that side has no
// partial), or (-2, -2): not logarithmic
std::pair<int32_t, int32_t> Analysis::walk_fuse_partials(int64_t doff, const std::map<int64_t, int> &recipe_of) {
    const std::pair<int32_t, int32_t> not_log(-2, -2);
    int32_t side[2] = {-1, -1};
    int64_t cur = doff;
    for (int depth = 0; depth < 8; ++depth) {
        const auto r = recipe_of.find(cur);
        if (r == recipe_of.end()) return not_log;
        const epgx_fuse_partial &fp = d.fuse_partial[r->second];
        if (fp.de_off >= 0) {
            const int which = fp.after ? 0 : 1;
            if (side[which] != -1 || fp.de_space != fp.e_space) return not_log;
            side[which] = log_table(fp.e_off, fp.de_off, fp.e_space);
        }
        if (fp.dsrc_off < 0) return {side[0], side[1]};   // the rotation itself has no partial: relaxations alone
        if (fp.dsrc_off < d.n_coef) return not_log;        // a rotation partial of the host: not this route
        cur = fp.dsrc_off;
    }
    return not_log;   // (deeper than 8 recipes)
}

// derivative plans that may fold (drun_kernel): a table of logarithmic partials per (real relaxation table, real partial
// table over the same index space)
void Analysis::layout_log_tables() {
    if (d.n_vars == 0 || !may_fold) return;
    host.log_of.assign((size_t)d.n_ops * EPGX_MAX_VARS, -1);
    for (int i = 0; i < d.n_ops; ++i) {
        const epgx_op &op = host.ops[i];
        if (op.opcode != EPGX_OP_E || op.ncoef != 4 || host.zero_pattern[i] != 2) continue;
        for (int v = 0; v < d.n_vars; ++v) {
            const int64_t doff = host.dops[i].coef_off[v];
            if (doff < 0 || ((host.dpattern[i] >> (2 * v)) & 3u) != 1u || host.dops[i].space[v] != op.space) continue;
            host.log_of[(size_t)i * EPGX_MAX_VARS + v] = log_table(op.coef_off, doff, op.space);
        }
    }
    // fused echoes: walk the epgx_fuse_partial chain behind every generated partial of an EPGX_OP_T0 operator
    if (d.n_fuse_partial == 0) return;
    std::map<int64_t, int> recipe_of;
    for (int k = 0; k < d.n_fuse_partial; ++k) recipe_of[d.fuse_partial[k].dst_off] = k;
    host.t0_log.assign((size_t)d.n_ops * EPGX_MAX_VARS * 2, -1);
    host.t0_logd.assign((size_t)d.n_ops * EPGX_MAX_VARS, 0);
    std::map<int64_t, std::pair<int32_t, int32_t>> walked;   // partial offset -> (a, b)
    for (int i = 0; i < d.n_ops; ++i) {
        if (host.ops[i].opcode != EPGX_OP_T0) continue;
        for (int v = 0; v < d.n_vars; ++v) {
            const int64_t doff = host.dops[i].coef_off[v];
            if (doff < d.n_coef) continue;   // (no partial, or not a generated one)
            auto w = walked.find(doff);
            if (w == walked.end()) w = walked.emplace(doff, walk_fuse_partials(doff, recipe_of)).first;
            if (w->second.first == -2) continue;
            host.t0_log[((size_t)i * EPGX_MAX_VARS + v) * 2] = w->second.first;
            host.t0_log[((size_t)i * EPGX_MAX_VARS + v) * 2 + 1] = w->second.second;
            host.t0_logd[(size_t)i * EPGX_MAX_VARS + v] = 1;
        }
    }
}

int Analysis::run() {
    const Lap lap;
    if (int rc = check_descriptor()) return rc;
    if (int rc = derive_geometry()) return rc;
    if (int rc = check_assembled()) return rc;
    if (int rc = check_chains()) return rc;
    if (int rc = check_operators()) return rc;
    if (int rc = check_derivatives()) return rc;
    if (int rc = check_fuses()) return rc;
    if (int rc = check_fuse_partials()) return rc;
    lap("validated");
    if (int rc = operator_patterns()) return rc;
    if (int rc = partial_patterns()) return rc;
    lap("zero scan");
    if (int rc = copy_gather_tables()) return rc;
    layout_log_tables();
    return EPGX_OK;
}

}  // namespace

int analyse_plan(const epgx_plan_desc *d, const epgx_plan_ext *ext, const Knobs &kn, PlanAnalysis *out) {
    *out = PlanAnalysis();
    return Analysis(*d, ext, kn, *out).run();
}

}  // namespace epgx

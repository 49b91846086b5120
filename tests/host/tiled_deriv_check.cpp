// tiled_deriv_check.cpp -- the tiled schedule of a derivative plan (tiled_schedule, epgpy_amd/csrc/epgx_planner.cpp) on a
// machine without a GPU: what epgx_run_tiled_deriv walks.
//
//   * `drecs` stays parallel to `recs`; a record that carries a stage with a partial keeps that partial's table;
//   * the unit shifts the schedule makes out of a shift by 2 .. H, and the probe records it splits off a shift by more than H,
//     have no partials (present == 0);
//   * blocks, shift steps, tiles and the peak are those of the same plan without variables (both unfolded: the run-time fold
//     of a plain plan merges records, which derivative plans never do).
// One line per check; exits non-zero at the first failure (tests/test_tiled_jacobian_host.py compiles and runs it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../epgpy_amd/csrc/epgx_planner.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) exit(1);
}
#define CHECK(cond) check((cond), #cond)

static const int NOTRUNC = INT32_MAX;
static const int M = 8, H = 32, W = 64 * M - 2 * H;

struct Seq {
    PlanHost ph;
    int n_adc = 0;
    void push(int opcode, int ia, int ib, int64_t off, int ncoef, int space, int zero, int64_t partial) {
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
        epgx_dop d;
        memset(&d, 0, sizeof(d));
        for (int v = 0; v < EPGX_MAX_VARS; ++v) d.coef_off[v] = d.space[v] = -1;
        if (partial >= 0) d.coef_off[0] = partial, d.space[0] = 0;
        dops.push_back(d);
    }
    std::vector<epgx_dop> dops;
    void T(int64_t off, int64_t partial = -1) { push(EPGX_OP_T, 0, 0, off, 8, 0, 0, partial); }
    void E(int64_t off, int64_t partial = -1) { push(EPGX_OP_E, 0, 0, off, 4, 0, 2, partial); }
    void S(int n, int kmax = NOTRUNC) { push(EPGX_OP_S, n, kmax, 0, 0, -1, 0, -1); }
    void ADC() { push(EPGX_OP_ADC, n_adc, 0, 0, 0, -1, 0, -1), n_adc += 1 + ph.n_vars; }
    void RESET() { push(EPGX_OP_RESET, 0, 0, 0, 0, -1, 0, -1); }
    void finish() {
        if (ph.n_vars > 0) {
            ph.dops = dops;
            ph.dpattern.assign(ph.ops.size(), 0);
        }
    }
};

static Knobs defaults() {   // the values knobs() takes with an empty environment
    Knobs k = {true, true, true, true, true, true, true, true, true, 1, true, 0.1, true, 0, true, true, true, 1};
    return k;
}

// T | (S E T S E ADC) x n with partials of E and T, then the shifts the schedule rewrites, a truncation and a reset
static Seq plan(int n_vars) {
    Seq s;
    s.ph.n_spaces = 1;
    s.ph.n_pool = 1 << 20;
    s.ph.fold = false;
    s.ph.n_vars = n_vars;
    s.T(0, 9000);
    auto echoes = [&](int n, int kmax) {
        for (int i = 0; i < n; ++i) {
            s.S(1, kmax);
            s.E(64, 9100);
            s.T(16, 9200);
            s.S(1, kmax);
            s.E(64, 9100);
            s.ADC();
        }
    };
    echoes(300, NOTRUNC);
    s.E(64, 9100);
    s.T(16, 9200);
    s.S(5);              // five unit shifts: the stages and their partials on the first
    s.ADC();
    s.T(16, 9200);
    s.S(-3);
    s.E(64, 9100);
    s.S(40);             // more than H: a step of its own, the relaxation stays a record, the probe becomes one
    s.ADC();
    s.T(16, 9200);
    s.S(-300);
    s.S(300);
    s.ADC();
    echoes(260, 1100);   // truncation inside tile 2
    s.RESET();
    s.T(0, 9000);
    echoes(20, NOTRUNC);
    s.finish();
    return s;
}

static int shifts_of(const Rec &r) { return ((r.flags & F_S0) ? 1 : 0) + ((r.flags & F_S) ? 1 : 0); }

int main() {
    const int Kbuf = 1280;
    Seq d = plan(1), p = plan(0);
    TiledSchedule td, tp;
    CHECK(tiled_schedule(d.ph, Kbuf, 0, M, H, defaults(), td) == EPGX_OK);
    CHECK(tiled_schedule(p.ph, Kbuf, 0, M, H, defaults(), tp) == EPGX_OK);
    printf("== %zu records, %zu steps, %d shift steps, peak %d, %lld tile launches\n", td.recs.size(), td.steps.size(), td.n_shift, td.peak,
           (long long)td.tile_launches);

    // parallel lists; the plain plan has none
    CHECK(td.drecs.size() == td.recs.size());
    CHECK(tp.drecs.empty());
    CHECK(td.peak == 1248 && td.peak / W == 2);      // (600 + 5 + 3 + 40 + 300 + 300: shifts count by |n|)

    // a partial belongs to a stage: a record with a T / E stage carries the table of that stage's operator, any other record none
    bool stage_ok = true, bare_ok = true, unit_ok = true;
    int units_made = 0, with_partial = 0;
    for (size_t i = 0; i < td.recs.size(); ++i) {
        const Rec &r = td.recs[i];
        const DRec &dr = td.drecs[i];
        const bool t = (r.flags & F_T) != 0, e = (r.flags & F_E) != 0;
        if (t) stage_ok = stage_ok && (dr.present & 1u) && (dr.t_off[0] == 8u * 9000 || dr.t_off[0] == 8u * 9200);
        else stage_ok = stage_ok && !(dr.present & 1u);
        if (e) stage_ok = stage_ok && (dr.present & 16u) && dr.e_off[0] == 8u * 9100;
        else stage_ok = stage_ok && !(dr.present & 16u);
        if (!t && !e) bare_ok = bare_ok && dr.present == 0;
        if (dr.present) ++with_partial;
        // a unit shift made by the schedule: a bare S(+-1) (with the truncation or the probe of the shift it came from)
        if ((r.flags & 0xffffffu & ~(F_S | F_TRUNC | F_ADC | F_ADC_Z)) == 0 && (r.flags & F_S)) {
            ++units_made;
            unit_ok = unit_ok && dr.present == 0 && (r.shift == 1 || r.shift == -1);
        }
    }
    CHECK(stage_ok);
    CHECK(bare_ok);
    CHECK(unit_ok);
    CHECK(units_made >= 4 + 2);      // S(5) -> 1 + 4 units, S(-3) -> 1 + 2
    CHECK(with_partial > 1000);

    // no record of a block shifts by more than one, no block by more than H in all
    bool one_ok = true, block_ok = true;
    for (const Rec &r : td.recs) one_ok = one_ok && (!(r.flags & F_S) || r.shift == 1 || r.shift == -1);
    for (const TiledStep &st : td.steps) {
        int u = 0;
        for (int i = st.rec0; i < st.rec1; ++i) u += shifts_of(td.recs[(size_t)i]);
        block_ok = block_ok && (st.shift ? (st.rec1 == st.rec0 && std::abs(st.shift) > H) : (st.rec1 > st.rec0 && u <= H));
    }
    CHECK(one_ok);
    CHECK(block_ok);
    CHECK(td.n_shift == 3);          // 40, -300, 300

    // the same blocks, tiles and peak as the plan without variables
    CHECK(td.recs.size() == tp.recs.size() && td.steps.size() == tp.steps.size());
    CHECK(td.peak == tp.peak && td.n_shift == tp.n_shift && td.tile_launches == tp.tile_launches && td.has_adc == tp.has_adc);
    bool same = true;
    for (size_t j = 0; j < td.steps.size() && j < tp.steps.size(); ++j) {
        const TiledStep &a = td.steps[j], &b = tp.steps[j];
        same = same && a.rec0 == b.rec0 && a.rec1 == b.rec1 && a.shift == b.shift && a.kmax == b.kmax && a.tiles == b.tiles && a.top == b.top;
    }
    CHECK(same);
    bool same_flags = true;
    for (size_t i = 0; i < td.recs.size() && i < tp.recs.size(); ++i)
        same_flags = same_flags && (td.recs[i].flags & 0xffffffu) == (tp.recs[i].flags & 0xffffffu) && td.recs[i].shift == tp.recs[i].shift &&
                     td.recs[i].kmax == tp.recs[i].kmax;
    CHECK(same_flags);
    // the ADC rows of the derivative plan advance by 1 + n_vars
    int last = -2;
    bool rows_ok = true;
    for (const Rec &r : td.recs)
        if (r.flags & F_ADC) rows_ok = rows_ok && r.slot == last + 2, last = r.slot;
    CHECK(rows_ok);
    printf("tiled_deriv_check: all checks passed\n");
    return 0;
}

// lanes_odd_cells_check.cpp -- the cells of rows_grow_lanes_kernel_odd (epgpy_amd/csrc/epgx_lanes_odd_cells.h) on the host: the
// functions the kernel runs, compiled by the host compiler (under -fsanitize=address,undefined by tests/test_lanes_odd_host.py:
// every slot index is a compile-time constant into a stack array, so an index out of range is a sanitizer report).
//   * trains of 1 .. 23 echoes (L = 2 .. 24), at the capacity the library ships (12 cells) and at the smallest that holds L
//     (L / 2 cells): after every echo the probe (F+ slot 0) equals, bit for bit, that of a plain restatement of the FULL record
//     of rows_grow_lanes_kernel -- every order 0 .. lim, the constant term on order 0, slots from L on absent;
//   * windows the parity rule cannot produce (even, negative, beyond the capacity) touch nothing outside the state.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../epgpy_amd/csrc/epgx_lanes_odd_cells.h"

using namespace epgx;

static void check(bool ok, const char *what) {
    if (!ok) {
        printf("FAIL  %s\n", what);
        exit(1);
    }
}

// the folded echo of rows_grow_lanes_kernel (lanes_cell_body<D, 1, 1, J>, tk 2, t0, no relaxation) on slots 0 .. CAP + 1; slots from
// lcap on read as zero and drop what is written
constexpr int CAP = 24;
struct Full {
    double Ar[CAP + 2], Ai[CAP + 2], Br[CAP + 2], Bi[CAP + 2], Zr[CAP + 2], Zi[CAP + 2];
};
static void full_record(Full &s, int lcap, int lim, const LaneLine &k) {
    if (lim < 0) return;
    double pend[4] = {0.0, 0.0, 0.0, 0.0};
    auto get = [&](const double *re, const double *im, int idx, double &xr, double &xi) {
        xr = xi = 0.0;
        if (idx < lcap && idx < CAP) {
            xr = re[idx];
            xi = im[idx];
        }
    };
    auto put = [&](double *re, double *im, int idx, double xr, double xi) {
        if (idx >= 0 && idx < lcap && idx < CAP) {
            re[idx] = xr;
            im[idx] = xi;
        }
    };
    for (int j = lim; j >= 0; --j) {
        double ar, ai, br, bi, zr, zi;
        get(s.Br, s.Bi, j + 1, br, bi);
        if (j == 0) {
            ar = br;
            ai = -bi;
        } else {
            get(s.Ar, s.Ai, j - 1, ar, ai);
        }
        get(s.Zr, s.Zi, j, zr, zi);
        put(s.Br, s.Bi, j + 1, pend[2], pend[3]);
        pend[2] = pend[0];
        pend[3] = pend[1];
        lanes_tx_sumdiff(k, ar, ai, br, bi, zr, zi);
        if (j == 0) {   // cell_offset
            ai = __builtin_fma(k.c[13], 1.0, ai);
            bi = __builtin_fma(-k.c[13], 1.0, bi);
            zr = __builtin_fma(k.c[14], 1.0, zr);
        }
        put(s.Ar, s.Ai, j + 1, ar, ai);
        put(s.Zr, s.Zi, j, zr, zi);
        pend[0] = br;
        pend[1] = bi;
    }
    s.Br[0] = pend[2];
    s.Bi[0] = pend[3];
    s.Ar[0] = s.Br[0];
    s.Ai[0] = -s.Bi[0];
}

static LaneLine line() {   // a refocusing pulse of 150 degrees with relaxation folded in: no entry is zero, none is special
    LaneLine k;
    for (int j = 0; j < 15; ++j) k.c[j] = 0.0;
    k.c[0] = 0.0651;
    k.c[1] = 0.9017;
    k.c[4] = -0.2391;
    k.c[6] = -0.2442;
    k.c[7] = -0.8511;
    k.c[13] = 0.0123;
    k.c[14] = 0.0456;
    return k;
}

template <int C>
static int train(int necho) {
    const int L = necho + 1;
    check(lanes_odd_cells(L) <= C, "the capacity holds the launch");
    const LaneLine k = line();
    Full f;
    memset(&f, 0, sizeof(f));
    LaneOdd<C> s;
    memset(&s, 0, sizeof(s));
    // behind the excitation: F+0, F-0 = conj, Z0 (the even class: the odd cells never read it)
    f.Ar[0] = s.Pr[0] = 0.31;
    f.Ai[0] = s.Pi[0] = -0.94;
    f.Br[0] = s.Qr[0] = 0.31;
    f.Bi[0] = s.Qi[0] = 0.94;
    f.Zr[0] = 0.11;
    int top = 0, rem = 2 * necho, cells = 0;
    for (int e = 0; e < necho; ++e) {
        int lim = top + 1 < rem - 1 ? top + 1 : rem - 1;
        lim = lim < L - 1 ? lim : L - 1;
        check(lim % 2 == 1 && (lim + 1) / 2 <= C, "the window is odd and within the cells");
        full_record(f, L, lim, k);
        lanes_odd_record<C>(s, lim, k);
        cells += (lim + 1) / 2;
        top += 2;
        rem -= 2;
        check(memcmp(&f.Ar[0], &s.Pr[0], 8) == 0 && memcmp(&f.Ai[0], &s.Pi[0], 8) == 0, "the probe is that of the full record, bit for bit");
        check(f.Ar[0] != 0.0 && f.Ai[0] != 0.0, "the probe is not trivial");
    }
    return cells;
}

template <int C>
static void stray_windows() {
    const LaneLine k = line();
    LaneOdd<C> s;
    memset(&s, 0, sizeof(s));
    s.Pr[0] = 1.0;
    for (int lim = -5; lim <= 64; ++lim) lanes_odd_record<C>(s, lim, k);   // (the sanitizers are the check)
}

template <int... Cs>
static void all(std::integer_sequence<int, Cs...>) {
    int total = 0;
    // capacity Cs + 1: the trains it is the smallest for (L / 2 == Cs + 1: L = 2 Cs + 2, 2 Cs + 3) and every shorter one
    ((stray_windows<Cs + 1>(), [&] {
         for (int necho = 1; necho + 1 <= 2 * (Cs + 1) + 1 && necho <= 23; ++necho) total += train<Cs + 1>(necho);
     }()),
     ...);
    printf("capacities 1 .. %d: %d cells walked\n", (int)sizeof...(Cs), total);
}

int main() {
    static_assert(lanes_odd_cells(24) == 12 && lanes_odd_cells(21) == 10 && lanes_odd_cells(22) == 11, "cells for L");
    all(std::make_integer_sequence<int, 12>());
    check(train<12>(20) == 110, "the benchmark's train runs 110 cells per voxel");
    printf("lanes_odd_cells_check: all checks passed\n");
    return 0;
}

// epgx_nnls_active.hip.h -- the device functions that nnls_kernel (epgx_nnls.hip) and nnls_chi2_kernel (epgx_nnls_chi2.hip) share:
// the wave-level primitives, the projections E and f of a voxel, the ridge of a group and ONE ACTIVE-SET FIT of a (voxel, group)
// at a given ridge -- Lawson and Hanson on the Gram form, one wavefront per voxel, lane a owning atom a (epgx_nnls.hip has the
// layout).  Both kernels call the same code, so the fit of a group is the same bits in either.
#pragma once
#include "epgx_nnls.h"

namespace epgx {

// LDS written by some lanes of a wavefront, read by others
__device__ __forceinline__ void nnls_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane j's value, j wave-uniform
__device__ __forceinline__ int nnls_lane(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ double nnls_lane(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// (no NaN among the inputs: the callers pass +-Inf for the lanes that do not take part)
__device__ __forceinline__ double nnls_wave_max(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ double nnls_wave_min(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ unsigned long long nnls_below(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1ull; }
__device__ __forceinline__ int nnls_tri(int q) { return q * (q - 1) / 2; }      // row q of the strict lower triangle

// row q of the factor from the rows before it, for atom `atom` at position q: lane i < q computes L[q][i], lane q the inverse
// diagonal.  patom: the atom at this lane's position (positions < q); invd: 1 / L[i][i] of this lane's position.
// false: the pivot is not finite or <= 0 (nothing is written)
__device__ __forceinline__ bool nnls_chol_row(const double *Hs, double *Lw, int A, int q, int atom, double mu, int patom, double &invd,
                                              int lane) {
    double h = 0.0;
    if (lane < q) h = Hs[patom * A + atom];
    double piv = Hs[atom * A + atom] + mu;
    for (int j = 0; j < q; ++j) {
        const double rj = nnls_lane(h * invd, j);      // L[q][j]: lane j took its last update at step j - 1
        piv = fma(-rj, rj, piv);
        if (lane > j && lane < q) h = fma(-Lw[nnls_tri(lane) + j], rj, h);
    }
    if (!(piv > 0.0) || !__builtin_isfinite(piv)) return false;
    if (lane < q) Lw[nnls_tri(q) + lane] = h * invd;
    if (lane == q) invd = 1.0 / sqrt(piv);
    nnls_wave_sync();
    return true;
}

// s = (L L^T)^-1 rhs over the positions < k (rhs and s by position)
__device__ __forceinline__ double nnls_solve(const double *Lw, int k, double rhs, double invd, int lane) {
    double z = lane < k ? rhs : 0.0;
    for (int j = 0; j < k; ++j) {
        const double zj = nnls_lane(z * invd, j);
        if (lane > j && lane < k) z = fma(-Lw[nnls_tri(lane) + j], zj, z);
    }
    double y = z * invd;
    for (int j = k - 1; j >= 0; --j) {
        const double sj = nnls_lane(y * invd, j);
        if (lane < j) y = fma(-Lw[nnls_tri(j) + lane], sj, y);
    }
    return y * invd;
}

// w_a = f_a - ((H + mu I) x)_a for every atom (lane), x by position, summed over the positions in ascending order
__device__ __forceinline__ double nnls_gradient(const double *Hs, int A, int k, double f, double mu, int patom, int pos, double xs,
                                                int lane) {
    double w = f;
    for (int q = 0; q < k; ++q) {
        const int b = nnls_lane(patom, q);
        const double xb = nnls_lane(xs, q);
        if (lane < A) w = fma(-Hs[b * A + lane], xb, w);
    }
    const double own = __shfl(xs, pos >= 0 ? pos : lane);
    if (pos >= 0) w = fma(-mu, own, w);
    return w;
}

// E = sum_t |S[t,m]|^2, records ascending
__device__ __forceinline__ double nnls_energy(const d2 *sig, int64_t sig_stride, int nrec, int64_t m) {
    double E = 0.0;
    for (int t = 0; t < nrec; ++t) {
        const d2 s = sig[(int64_t)t * sig_stride + m];
        E = fma(s.x, s.x, E);
        E = fma(s.y, s.y, E);
    }
    return E;
}

// f_a = Re sum_t conj(D[t,a,g]) S[t,m] of this lane's atom (0 where it is not valid), records ascending
__device__ __forceinline__ double nnls_project(const ComponentArgs &c, const d2 *sig, int64_t sig_stride, int64_t m, int64_t g, bool valid,
                                               int lane) {
    double f = 0.0;
    if (valid) {
        const d2 *col = c.dict + ((g / c.ninner) * c.ncomp + lane) * c.axis_stride + g % c.ninner;
        const d2 *scol = sig + m;
        for (int t = 0; t < c.nrec; ++t) {
            const d2 d = col[(int64_t)t * c.row_stride];
            const d2 s = scol[(int64_t)t * sig_stride];
            f = fma(d.x, s.x, f);
            f = fma(d.y, s.y, f);
        }
    }
    return f;
}

// mu_g = reg * mean over the valid atoms of H_g[a,a] (0 without a valid atom), atoms ascending
__device__ __forceinline__ double nnls_ridge(const double *Hs, int A, unsigned long long mask, double reg) {
    double trace = 0.0;
    for (int b = 0; b < A; ++b)
        if ((mask >> b) & 1ull) trace += Hs[b * A + b];
    const int nvalid = __builtin_popcountll(mask);
    return nvalid ? reg * (trace / nvalid) : 0.0;
}

// one fit of a (voxel, group) at the ridge mu, from x = 0 and an empty passive set.  Hs: the staged H_g; Lw, tmp: this wavefront's
// factor and scratch; by atom (lane a): valid, f, thr = tol sqrt(H_aa E).  status: 0, or 2 where E or an f_a is not finite.
// Returns the status (0; 1: the cap of solves, xa the last feasible iterate; 2: a pivot, a solution or J not finite) and, unless 2,
// xa (the weight of this lane's atom), J = E - sum_a x_a (f_a + w_a) and n2 = |x|^2, both summed over the atoms ascending.
__device__ __forceinline__ int nnls_active_set(const double *Hs, double *Lw, int *tmp, int A, int lane, bool valid, double f, double E,
                                               double thr, double mu, int cap, int status, double &xa, double &J, double &n2) {
    const double inf = __builtin_inf();
    // by atom (lane a): f, w, thr, valid, pos.  By position (lane i < k): patom, xs, invd
    double w = f, xs = 0.0, invd = 0.0;
    int pos = -1, patom = 0, k = 0, solves = 0;

    while (status == 0) {
        const bool cand = valid && pos < 0 && w > thr;
        if (!__ballot(cand)) break;
        const double wmax = nnls_wave_max(cand ? w : -inf);
        const int enter = __builtin_ctzll(__ballot(cand && w == wmax));      // the lowest atom among equal w
        if (lane == k) {
            patom = enter;
            xs = 0.0;
        }
        if (lane == enter) pos = k;
        if (!nnls_chol_row(Hs, Lw, A, k, enter, mu, patom, invd, lane)) {
            status = 2;
            break;
        }
        ++k;
        while (true) {
            if (solves == cap) {
                status = 1;      // xs is the last feasible iterate
                break;
            }
            ++solves;
            const double s = nnls_solve(Lw, k, __shfl(f, lane < k ? patom : lane), invd, lane);
            if (__ballot(lane < k && !__builtin_isfinite(s))) {
                status = 2;
                break;
            }
            const bool neg = lane < k && !(s > 0.0);
            if (!__ballot(neg)) {
                xs = lane < k ? s : 0.0;
                break;
            }
            // towards s as far as x >= 0 allows; the atoms that reach 0 leave
            const double al = neg ? (xs == 0.0 ? 0.0 : xs / (xs - s)) : inf;
            const double alpha = nnls_wave_min(al);
            const double xn = fma(alpha, s - xs, xs);
            const bool drop = neg && (!(xn > 0.0) || al == alpha);
            const unsigned long long dropped = __ballot(drop);
            const unsigned long long kept = nnls_below(k) & ~dropped;
            // by position: does this position stay, and where does it move (the kept positions below it)
            const int stays = (lane < k && !drop) ? 1 : 0;
            const int moved = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
            // by atom, before the positions move
            const int from = pos >= 0 ? pos : lane;
            const double xatom = __shfl(xn, from);
            const int astays = __shfl(stays, from), amoved = __shfl(moved, from);
            nnls_wave_sync();
            if (stays) tmp[moved] = patom;
            nnls_wave_sync();
            if (pos >= 0) pos = astays ? amoved : -1;
            const int first = __builtin_ctzll(dropped);                 // the rows before it keep their entries
            k = __builtin_popcountll(kept);
            if (lane < k) patom = tmp[lane];
            nnls_wave_sync();
            xs = __shfl(xatom, lane < k ? patom : lane);
            if (lane >= k) xs = 0.0;
            bool sound = true;
            for (int q = first; q < k && sound; ++q) sound = nnls_chol_row(Hs, Lw, A, q, nnls_lane(patom, q), mu, patom, invd, lane);
            if (!sound) {
                status = 2;
                break;
            }
            if (k == 0) break;
        }
        if (status == 2) break;
        w = nnls_gradient(Hs, A, k, f, mu, patom, pos, xs, lane);
    }
    if (status == 2) return 2;
    // J = E - sum_a x_a (f_a + w_a), atoms ascending
    // (every lane takes part in the shuffle: a lane that sat it out would hand 0 to the atom whose position it holds)
    const double xpos = __shfl(xs, pos >= 0 ? pos : lane);
    xa = pos >= 0 ? xpos : 0.0;
    const double term = pos >= 0 ? xa * (f + w) : 0.0;
    J = E;
    n2 = 0.0;
    for (int b = 0; b < A; ++b) {
        const double xb = nnls_lane(xa, b);
        if (xb != 0.0) {      // (wave-uniform)
            J -= nnls_lane(term, b);
            n2 = fma(xb, xb, n2);
        }
    }
    return __builtin_isfinite(J) ? status : 2;
}

}  // namespace epgx

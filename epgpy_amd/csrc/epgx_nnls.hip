// epgx_nnls.hip -- non-negative mixtures of the atoms along one grid axis of a dictionary that stays in HBM (include/epgx.h
// epgx_signal_component_gram, epgx_signal_nnls).  With D[t,a,g] (records t, atoms a < A <= 64 of the component axis, groups g) and
// S[t,m]:
//      H_g[a,b] = Re sum_t conj(D[t,a,g]) D[t,b,g]      f[a] = Re sum_t conj(D[t,a,g]) S[t,m]      E = sum_t |S[t,m]|^2
//      x* = argmin over x >= 0 of  x^T (H_g + mu_g I) x - 2 f^T x + E,      mu_g = reg * mean over the valid atoms of H_g[a,a]
//
// component_gram_kernel: one block per group; every entry of H_g is one sequential sum over the records (so H_g is symmetric to
// the bit), and the first wavefront votes the validity mask.
//
// nnls_kernel: Lawson and Hanson's active set on the Gram form, ONE WAVEFRONT PER VOXEL, lane a owning atom a: f_a, w_a, the
// threshold and the position of the atom in the passive set stay in registers.  The same lanes, counted as POSITIONS 0 .. k - 1 of
// the passive set in the order the atoms entered, hold the atom at each position, its weight and the inverse diagonal of the
// Cholesky factor of (H_g + mu_g I)[P,P]; the strict lower triangle of the factor lies in LDS, one per wavefront, and grows by one
// row when an atom enters.  When atoms leave, the rows from the first vacated position on are rebuilt.  A passive-set solve is a
// forward and a backward substitution of k steps each: the pivot lane's value goes round by v_readlane and every later lane
// takes one fused multiply-add against a column (forward) or a row (backward) of the factor.
// The block stages H_g in LDS once per group.  In the group search the 4 wavefronts of a block (4 voxels) walk the groups together,
// in ascending order, and each keeps the best group so far in registers: J < best replaces, so the lowest g wins among equal J
// and nothing depends on the order in which anything finishes.  With fixed groups a block is one wavefront and stages the H_g of
// its voxel.  No atomics; every sum runs in a fixed order (records ascending, passive positions ascending, atoms ascending) that
// depends on the voxel's own data alone, so a voxel's bits do not depend on the other voxels or on the launch.  Plain vector stores.
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

__global__ void __launch_bounds__(NNLS_WAVES * 64) nnls_kernel(const NnlsArgs a) {
    extern __shared__ double nnls_lds[];
    const int A = a.c.ncomp;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)(blockDim.x >> 6);
    double *Hs = nnls_lds;                                                     // [A][A]
    double *Lw = Hs + A * A + wave * (A * (A - 1) / 2);                        // this wavefront's factor
    int *tmp = (int *)(Hs + A * A + waves * (A * (A - 1) / 2)) + wave * 64;    // this wavefront's scratch
    const int64_t m = (int64_t)blockIdx.x * waves + wave;
    const bool live = m < a.nmeas;
    const int64_t G = a.c.nouter * a.c.ninner;
    const int cap = 3 * A;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    int64_t g0 = 0, g1 = G;
    if (a.group) {      // (a block is one wavefront)
        const int64_t g = live ? a.group[m] : -1;
        g0 = g >= 0 && g < G ? g : 0;
        g1 = g >= 0 && g < G ? g + 1 : 0;
    }

    double E = 0.0;
    if (live && g1 > g0) {
        for (int t = 0; t < a.c.nrec; ++t) {
            const d2 s = a.sig[(int64_t)t * a.sig_stride + m];
            E = fma(s.x, s.x, E);
            E = fma(s.y, s.y, E);
        }
    }

    double best_j = inf, best_x = nan, best_res = nan;
    int64_t best_g = -1;
    int best_status = 2;

    for (int64_t g = g0; g < g1; ++g) {
        __syncthreads();      // (the H of the group before has been read)
        for (int idx = threadIdx.x; idx < A * A; idx += blockDim.x) Hs[idx] = a.gram[g * A * A + idx];
        __syncthreads();
        if (!live) continue;

        const unsigned long long mask = a.mask[g];
        const bool valid = lane < A && ((mask >> lane) & 1ull);
        const double diag = valid ? Hs[lane * A + lane] : 0.0;
        double trace = 0.0;
        for (int b = 0; b < A; ++b)
            if ((mask >> b) & 1ull) trace += Hs[b * A + b];
        const int nvalid = __builtin_popcountll(mask);
        const double mu = nvalid ? a.reg * (trace / nvalid) : 0.0;

        double f = 0.0;
        if (valid) {
            const d2 *col = a.c.dict + ((g / a.c.ninner) * A + lane) * a.c.axis_stride + g % a.c.ninner;
            const d2 *scol = a.sig + m;
            for (int t = 0; t < a.c.nrec; ++t) {
                const d2 d = col[(int64_t)t * a.c.row_stride];
                const d2 s = scol[(int64_t)t * a.sig_stride];
                f = fma(d.x, s.x, f);
                f = fma(d.y, s.y, f);
            }
        }

        int status = 0;
        if (!__builtin_isfinite(E) || __ballot(valid && !__builtin_isfinite(f))) status = 2;
        const double thr = a.tol * sqrt(diag * E);

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

        if (status == 2) continue;
        // J = E - sum_a x_a (f_a + w_a), atoms ascending
        // (every lane takes part in the shuffle: a lane that sat it out would hand 0 to the atom whose position it holds)
        const double xpos = __shfl(xs, pos >= 0 ? pos : lane);
        const double xa = pos >= 0 ? xpos : 0.0;
        const double term = pos >= 0 ? xa * (f + w) : 0.0;
        double J = E, n2 = 0.0;
        for (int b = 0; b < A; ++b) {
            const double xb = nnls_lane(xa, b);
            if (xb != 0.0) {      // (wave-uniform)
                J -= nnls_lane(term, b);
                n2 = fma(xb, xb, n2);
            }
        }
        if (!__builtin_isfinite(J)) continue;
        if (J < best_j) {
            const double data = fma(-mu, n2, J);
            best_j = J;
            best_g = g;
            best_x = xa;
            best_res = sqrt(data > 0.0 ? data : 0.0);
            best_status = status;
        }
    }

    if (!live) return;
    if (lane < A) a.weights[(int64_t)lane * a.nmeas + m] = best_x;
    if (lane == 0) {
        a.out_group[m] = best_g;
        a.residual[m] = best_res;
        a.status[m] = best_status;
    }
}

__global__ void __launch_bounds__(NNLS_GRAM_THREADS) component_gram_kernel(const ComponentGramArgs a) {
    const int A = a.c.ncomp;
    const int64_t g = blockIdx.x;
    const d2 *base = a.c.dict + (g / a.c.ninner) * A * a.c.axis_stride + g % a.c.ninner;
    for (int idx = threadIdx.x; idx < A * A; idx += NNLS_GRAM_THREADS) {
        const d2 *ca = base + (idx / A) * a.c.axis_stride, *cb = base + (idx % A) * a.c.axis_stride;
        double h = 0.0;
        for (int t = 0; t < a.c.nrec; ++t) {
            const d2 x = ca[(int64_t)t * a.c.row_stride], y = cb[(int64_t)t * a.c.row_stride];
            h = fma(x.x, y.x, h);      // (the same bits for (a, b) and (b, a))
            h = fma(x.y, y.y, h);
        }
        a.gram[g * A * A + idx] = h;
    }
    if (threadIdx.x < 64) {      // the first wavefront: the diagonal once more, by the same sums, and the vote
        const int lane = threadIdx.x;
        double n = 0.0;
        if (lane < A) {
            const d2 *ca = base + lane * a.c.axis_stride;
            for (int t = 0; t < a.c.nrec; ++t) {
                const d2 x = ca[(int64_t)t * a.c.row_stride];
                n = fma(x.x, x.x, n);
                n = fma(x.y, x.y, n);
            }
        }
        const unsigned long long ok = __ballot(lane < A && n > 0.0 && __builtin_isfinite(n));
        if (lane == 0) a.mask[g] = ok;
    }
}

}  // namespace epgx

hipError_t epgx_launch_component_gram(hipStream_t stream, const epgx::ComponentGramArgs &a) {
    const int64_t G = a.c.nouter * a.c.ninner;
    hipLaunchKernelGGL(epgx::component_gram_kernel, dim3((unsigned)G), dim3(epgx::NNLS_GRAM_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_nnls(hipStream_t stream, const epgx::NnlsArgs &a) {
    const int waves = a.group ? 1 : epgx::NNLS_WAVES;
    const int64_t blocks = (a.nmeas + waves - 1) / waves;
    const size_t lds = epgx::nnls_lds_bytes(a.c.ncomp, waves);
    if (lds > 160 * 1024) return hipErrorInvalidValue;      // (A <= 64: 95.5 KiB at most)
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)epgx::nnls_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(epgx::nnls_kernel, dim3((unsigned)blocks), dim3((unsigned)(waves * 64)), lds, stream, a);
    return hipGetLastError();
}

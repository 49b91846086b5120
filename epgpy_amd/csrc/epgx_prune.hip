// epgx_prune.hip -- the per-voxel float shift (epgpy/shift.py:478-629 `shiftprune`; include/epgx.h epgx_state_prune_shift).
//
// A float shift that varies along a grid axis gives every voxel its own coordinate set: which rows meet in a cell of the grid
// depends on the voxel's own coordinates and on its own state (the weights of the merged coordinate, the trim by energy, the
// prune by norm).  Nothing of this can be planned on the host; prune_shift_kernel does all of it on the resident state.
//
// One wavefront (= one block) per voxel, grid-stride over the voxels, lanes over stored orders.  The voxel is stored in the half
// representation: stored order i holds A_i = F(row +i), B_i = column 1 of row +i, Z_i and the coordinate k_i of row +i; row -i
// holds conj(B_i), conj(A_i), conj(Z_i) at -k_i.  A stored order gives three candidate cells -- where its Z stays (L), where
// the F of row +i goes (P) and where the F of row -i goes (M) -- and each candidate, negated, is the cell of the mirrored row.
// Cells are canonicalised (first non-zero column positive, with the sign remembered), the distinct canonical cells are ranked
// in lexicographic order by counting (at most 192 candidates per voxel: two passes over LDS), and the rank is the stored order
// of the destination.  Every destination row then adds its sources in ascending row of the full matrix from +0 -- the bits of
// np.add.at on zeros, as merge_kernel -- first the rows of the negative half (stored orders descending), then the others.  The
// weighted coordinates follow the reference's own order: all L sources, then all 1T, then all 2T, into one accumulator.  Trim
// (keep the nmax rows of largest energy) ranks by counting again; prune and compaction go by wave ballots.  No atomics: a
// voxel's bits depend on the voxel alone.  A block leaves (largest live count, overflow flag) of its voxels in `partial`,
// prune_final_kernel folds those: two words cross PCIe per shift.
// A modulus is sqrt(re re + im im) with every operation rounded on its own: the unit is compiled without fma contraction.
#include "epgx_prune.h"

namespace epgx {

__device__ __forceinline__ double prune_modulus(const d2 z) {
#pragma clang fp contract(off)
    const double a = z.x * z.x;
    const double b = z.y * z.y;
    return __builtin_sqrt(a + b);
}

__device__ __forceinline__ double prune_energy(const d2 z) {
#pragma clang fp contract(off)
    const double a = z.x * z.x;
    const double b = z.y * z.y;
    return a + b;
}

// the reference's own `round` (shift.py:554-555) followed by astype(int): trunc(x - 0.5 + (x > 0)), half away from zero
__device__ __forceinline__ double prune_round(const double x) {
#pragma clang fp contract(off)
    const double y = x - 0.5;
    return __builtin_trunc(y + (x > 0.0 ? 1.0 : 0.0));
}

template <int KD>
__global__ void __launch_bounds__(64) prune_shift_kernel(const PruneArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_cell[KD][PRUNE_CAND];     // canonical cell of a candidate; NaN in column 0: no such candidate
    __shared__ int32_t s_sign[PRUNE_CAND];        // +1: the cell itself is canonical, -1: its negative is, 0: the zero cell
    __shared__ int32_t s_first[PRUNE_CAND];       // 1 for the first candidate of every distinct canonical cell
    __shared__ int32_t s_rank[PRUNE_CAND];        // stored order of the destination a candidate's canonical cell becomes
    __shared__ d2 s_val[3][PRUNE_K];
    __shared__ double s_k[KD][PRUNE_K];
    __shared__ double s_mag[PRUNE_CAND];
    __shared__ double s_par[4][KD];               // the voxel's shift, the grid and the two scales: read back into vector registers, so that the
                                                  // wave-uniform values of the voxel do not crowd the scalar file

    const int lane = (int)threadIdx.x;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int maxlive = 0, overflow = 0;

    for (int64_t v = (int64_t)blockIdx.x; v < a.nvox; v += (int64_t)gridDim.x) {
        int64_t si = 0, rem = v;
        for (int d = 0; d < a.ndim; ++d) {      // (vstride is the C-order stride: the quotient is the index along axis d)
            const int64_t i = rem / a.vstride[d];
            rem -= i * a.vstride[d];
            si += i * a.sstride[d];
        }
        __syncthreads();      // (the voxel before this one has been read out of LDS)
        if (lane < KD) {
            double gl = a.grid[0], si_ = a.scale_in[0], so_ = a.scale_out[0];
#pragma unroll
            for (int c = 1; c < KD; ++c) {
                gl = lane == c ? a.grid[c] : gl;
                si_ = lane == c ? a.scale_in[c] : si_;
                so_ = lane == c ? a.scale_out[c] : so_;
            }
            s_par[0][lane] = a.table[si * KD + lane];
            s_par[1][lane] = gl;
            s_par[2][lane] = si_;
            s_par[3][lane] = so_;
        }
        __syncthreads();
        int n = a.nsrc[v];
        n = n < 1 ? 1 : (n > PRUNE_K ? PRUNE_K : n);

        // ---- the voxel: state and wavenumbers of stored order `lane`
        const bool live = lane < n;
        d2 va = {0.0, 0.0}, vb = {0.0, 0.0}, vz = {0.0, 0.0};
        double k[KD];
#pragma unroll
        for (int c = 0; c < KD; ++c) k[c] = 0.0;
        if (live) {
            const d2 *p = a.src + v * 3 * PRUNE_K + lane;
            va = p[0];
            vb = p[PRUNE_K];
            vz = p[2 * PRUNE_K];
#pragma unroll
            for (int c = 0; c < KD; ++c) k[c] = a.ksrc[(v * KD + c) * PRUNE_K + lane] * s_par[2][c];
        }
        s_val[0][lane] = va;
        s_val[1][lane] = vb;
        s_val[2][lane] = vz;
#pragma unroll
        for (int c = 0; c < KD; ++c) s_k[c][lane] = k[c];

        double s[KD], g[KD];
#pragma unroll
        for (int c = 0; c < KD; ++c) {
            s[c] = s_par[0][c];
            g[c] = s_par[1][c];
        }
        // ---- candidates: L (Z stays), P (F of row +i), M (F of row -i; row -0 is row +0)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            double q[KD];
            const bool valid = live && !(t == 2 && lane == 0);
#pragma unroll
            for (int c = 0; c < KD; ++c) {
                double x;
                if (t == 0) x = lane == 0 ? 0.0 : (0.5 * (k[c] + k[c])) / g[c];      // 0.5 (k_i - k_mirror(i)) / g
                else if (t == 1) x = (k[c] + s[c]) / g[c];
                else x = (s[c] - k[c]) / g[c];
                q[c] = prune_round(x);
            }
            int sign = 0;
#pragma unroll
            for (int c = 0; c < KD; ++c)
                if (sign == 0 && q[c] != 0.0) sign = q[c] < 0.0 ? -1 : 1;
#pragma unroll
            for (int c = 0; c < KD; ++c) {
                double w = sign < 0 ? -q[c] : q[c];
                if (w == 0.0) w = 0.0;      // (no -0)
                s_cell[c][t * PRUNE_K + lane] = (c == 0 && !valid) ? __builtin_nan("") : w;
            }
            s_sign[t * PRUNE_K + lane] = sign;
        }
        __syncthreads();

        // ---- the first candidate of every distinct cell
        int nd = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int me = t * PRUNE_K + lane;
            double q[KD];
#pragma unroll
            for (int c = 0; c < KD; ++c) q[c] = s_cell[c][me];
            bool first = q[0] == q[0];
            for (int tt = 0; tt <= t; ++tt) {
                const int end = tt < t ? n : lane;      // (candidates before this one: index tt * 64 + i)
                for (int i = 0; i < end; ++i) {
                    bool same = true;
#pragma unroll
                    for (int c = 0; c < KD; ++c) same = same && s_cell[c][tt * PRUNE_K + i] == q[c];
                    first = first && !same;
                }
            }
            s_first[me] = first ? 1 : 0;
            nd += __builtin_popcountll(__ballot(first));
        }
        __syncthreads();

        // ---- rank: the distinct cells that come before this one
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int me = t * PRUNE_K + lane;
            double q[KD];
#pragma unroll
            for (int c = 0; c < KD; ++c) q[c] = s_cell[c][me];
            int rank = 0;
            for (int tt = 0; tt < 3; ++tt)
                for (int i = 0; i < n; ++i) {
                    const int o = tt * PRUNE_K + i;
                    bool less = false, equal = true;
#pragma unroll
                    for (int c = 0; c < KD; ++c) {
                        const double x = s_cell[c][o];
                        less = less || (equal && x < q[c]);
                        equal = equal && x == q[c];
                    }
                    rank += (less && s_first[o]) ? 1 : 0;
                }
            s_rank[me] = q[0] == q[0] ? rank : -1;
        }
        __syncthreads();

        // ---- the destination rows j = slot * 64 + lane < nd
        d2 A[PRUNE_SLOTS], B[PRUNE_SLOTS], Z[PRUNE_SLOTS];
        double W[PRUNE_SLOTS], Kn[PRUNE_SLOTS][KD], mag[PRUNE_SLOTS];
#pragma unroll
        for (int u = 0; u < PRUNE_SLOTS; ++u) {
            A[u] = B[u] = Z[u] = d2{0.0, 0.0};
            W[u] = 0.0;
#pragma unroll
            for (int c = 0; c < KD; ++c) Kn[u][c] = 0.0;
        }
        const int nslot = (nd + 63) >> 6;      // (wave-uniform)

        // L: Z of row r stays in its (symmetrised) cell.  Rows -(n-1) .. -1, then 0 .. n-1
        for (int pass = 0; pass < 2; ++pass)
            for (int ii = pass ? 0 : n - 1; pass ? ii < n : ii >= 1; ii += pass ? 1 : -1) {
                const int r = s_rank[ii], sg = s_sign[ii];
                if (pass ? sg < 0 : sg > 0) continue;
                const d2 z = s_val[2][ii];
                const double w = prune_modulus(z);
#pragma unroll
                for (int u = 0; u < PRUNE_SLOTS; ++u)
                    if (u < nslot && r == u * 64 + lane) {
                        Z[u].x += z.x;
                        Z[u].y += pass ? z.y : -z.y;
                        W[u] += w;
#pragma unroll
                        for (int c = 0; c < KD; ++c) {
                            const double kk = pass ? s_k[c][ii] : -s_k[c][ii];
                            Kn[u][c] += kk * w;
                        }
                    }
            }
        // 1T: F of row r goes to the cell of k_r + s; column 1 of the destination is the conjugate of the mirrored cell's F
        for (int pass = 0; pass < 2; ++pass)
            for (int ii = pass ? 0 : n - 1; pass ? ii < n : ii >= 1; ii += pass ? 1 : -1) {
                const int o = (pass ? PRUNE_K : 2 * PRUNE_K) + ii;
                const int r = s_rank[o], sg = s_sign[o];
                d2 f = s_val[pass ? 0 : 1][ii];
                if (!pass) f.y = -f.y;
                const double w = prune_modulus(f);
#pragma unroll
                for (int u = 0; u < PRUNE_SLOTS; ++u)
                    if (u < nslot && r == u * 64 + lane) {
                        if (sg >= 0) {
                            A[u].x += f.x;
                            A[u].y += f.y;
                            W[u] += w;
#pragma unroll
                            for (int c = 0; c < KD; ++c) {
                                const double kk = pass ? s_k[c][ii] + s[c] : s[c] - s_k[c][ii];
                                Kn[u][c] += kk * w;
                            }
                        }
                        if (sg <= 0) {
                            B[u].x += f.x;
                            B[u].y += f.y;
                        }
                    }
            }
        // 2T: the mirror image of 1T; it carries weight and coordinate only.  Row -i mirrors P of order i; row +i mirrors M of
        // order i (row 0: its own P)
        for (int pass = 0; pass < 2; ++pass)
            for (int ii = pass ? 0 : n - 1; pass ? ii < n : ii >= 1; ii += pass ? 1 : -1) {
                const bool useP = !pass || ii == 0;
                const int o = (useP ? PRUNE_K : 2 * PRUNE_K) + ii;
                const int r = s_rank[o], sg = s_sign[o];
                if (sg > 0) continue;
                const double w = prune_modulus(s_val[pass ? 1 : 0][ii]);
#pragma unroll
                for (int u = 0; u < PRUNE_SLOTS; ++u)
                    if (u < nslot && r == u * 64 + lane) {
                        W[u] += w;
#pragma unroll
                        for (int c = 0; c < KD; ++c) {
                            const double kl = pass ? s_k[c][ii] : -s_k[c][ii];
                            Kn[u][c] += (kl - s[c]) * w;
                        }
                    }
            }

#pragma unroll
        for (int u = 0; u < PRUNE_SLOTS; ++u) {
            B[u].y = -B[u].y;
            const double den = W[u] + (W[u] < 1e-12 ? 1.0 : 0.0);
#pragma unroll
            for (int c = 0; c < KD; ++c) Kn[u][c] = Kn[u][c] / den;
            mag[u] = (prune_energy(A[u]) + prune_energy(B[u])) + prune_energy(Z[u]);
        }

        // ---- trim: the centre row and the nmax rows of largest energy (ties: the later row stays, a stable ascending sort)
        bool keep[PRUNE_SLOTS];
#pragma unroll
        for (int u = 0; u < PRUNE_SLOTS; ++u) keep[u] = u * 64 + lane < nd;
        if (a.nmax >= 0 && nd - 1 > a.nmax) {      // (wave-uniform)
#pragma unroll
            for (int u = 0; u < PRUNE_SLOTS; ++u) s_mag[u * 64 + lane] = (u == 0 && lane == 0) ? __builtin_inf() : mag[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PRUNE_SLOTS; ++u) {
                const int j = u * 64 + lane;
                const double mine = j == 0 ? __builtin_inf() : mag[u];
                int after = 0;
                for (int o = 0; o < nd; ++o) {
                    const double x = s_mag[o];
                    after += (x > mine || (x == mine && o > j)) ? 1 : 0;
                }
                keep[u] = keep[u] && after < a.nmax + 1;
            }
        }
        // ---- prune: the rows whose norm is <= tol leave; the centre row always stays
        if (a.prune) {
#pragma unroll
            for (int u = 0; u < PRUNE_SLOTS; ++u) keep[u] = keep[u] && ((u == 0 && lane == 0) || __builtin_sqrt(mag[u]) > a.tol);
        }
        // ---- compact
        int pos[PRUNE_SLOTS], nl = 0;
#pragma unroll
        for (int u = 0; u < PRUNE_SLOTS; ++u) {
            const unsigned long long m = __ballot(keep[u]);
            pos[u] = nl + __builtin_popcountll(m & below);
            nl += __builtin_popcountll(m);
        }
        if (nl > PRUNE_K) {      // (wave-uniform) the voxel does not fit: the call fails, the destination is dropped
            overflow = 1;
            if (lane == 0) a.ndst[v] = 0;
            continue;
        }
        maxlive = nl > maxlive ? nl : maxlive;
        d2 *pd = a.dst + v * 3 * PRUNE_K;
        double *pk = a.kdst + v * KD * PRUNE_K;
        if (lane >= nl) {
            pd[lane] = pd[PRUNE_K + lane] = pd[2 * PRUNE_K + lane] = d2{0.0, 0.0};
#pragma unroll
            for (int c = 0; c < KD; ++c) pk[c * PRUNE_K + lane] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < PRUNE_SLOTS; ++u)
            if (keep[u]) {      // (pos < nl <= 64)
                pd[pos[u]] = A[u];
                pd[PRUNE_K + pos[u]] = B[u];
                pd[2 * PRUNE_K + pos[u]] = Z[u];
#pragma unroll
                for (int c = 0; c < KD; ++c) pk[c * PRUNE_K + pos[u]] = Kn[u][c] / s_par[3][c];
            }
        if (lane == 0) a.ndst[v] = nl;
    }
    if (lane == 0) {
        a.partial[2 * blockIdx.x] = maxlive;
        a.partial[2 * blockIdx.x + 1] = overflow;
    }
}

// (largest live count, overflow flag) over the blocks' partials: one wavefront
__global__ void __launch_bounds__(64) prune_final_kernel(const PruneArgs a) {
    int m = 0, f = 0;
    for (int b = (int)threadIdx.x; b < a.nblocks; b += 64) {
        const int x = a.partial[2 * b];
        m = x > m ? x : m;
        f |= a.partial[2 * b + 1];
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int x = __shfl_xor(m, d);
        m = x > m ? x : m;
        f |= __shfl_xor(f, d);
    }
    if (threadIdx.x == 0) {
        a.result[0] = m;
        a.result[1] = f;
    }
}

// F0 with a time coordinate (statematrix.py:149-155): sum over the rows whose wavenumber is zero of F exp(-|t|), with the voxel's
// own coordinates.  Row -j has the weight of row +j and holds conj(B_j).  One wavefront per voxel, a butterfly over the lanes.
__global__ void __launch_bounds__(64) prune_read_kernel(const PruneReadArgs a) {
    const int lane = (int)threadIdx.x;
    for (int64_t v = (int64_t)blockIdx.x; v < a.nvox; v += (int64_t)gridDim.x) {
        int n = a.nlive[v];
        n = n < 1 ? 1 : (n > PRUNE_K ? PRUNE_K : n);
        d2 acc = {0.0, 0.0};
        if (lane < n) {
            const double *pk = a.k + v * 4 * PRUNE_K + lane;
            const bool zero = fabs(pk[0]) <= 1e-8 && fabs(pk[PRUNE_K]) <= 1e-8 && fabs(pk[2 * PRUNE_K]) <= 1e-8;      // np.isclose(k, 0)
            if (zero) {
                const double w = exp(-fabs(pk[3 * PRUNE_K] * a.tscale));
                const d2 *p = a.state + v * 3 * PRUNE_K + lane;
                const d2 fa = p[0];
                acc.x = fa.x * w;
                acc.y = fa.y * w;
                if (lane > 0) {
                    const d2 fb = p[PRUNE_K];
                    acc.x += fb.x * w;
                    acc.y -= fb.y * w;
                }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            acc.x += __shfl_xor(acc.x, d);
            acc.y += __shfl_xor(acc.y, d);
        }
        if (lane == 0) a.out[v] = acc;
    }
}

// dst[v][c][j] = src[v or 0][c][j] for c < ks, else 0; the live counts follow: the upload of shared coordinates to every voxel
// and the step to a larger kdim
__global__ void __launch_bounds__(256) coords_widen_kernel(const CoordsWidenArgs a) {
    const int64_t total = a.nvox * a.kd * PRUNE_K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % PRUNE_K);
        const int c = (int)((i / PRUNE_K) % a.kd);
        const int64_t v = i / ((int64_t)PRUNE_K * a.kd);
        const int64_t vs = a.broadcast ? 0 : v;
        a.dst[i] = c < a.ks ? a.src[(vs * a.ks + c) * PRUNE_K + j] : 0.0;
        if (j == 0 && c == 0) a.ndst[v] = a.nsrc_rows[vs];
    }
}

}  // namespace epgx

hipError_t epgx_launch_prune_shift(hipStream_t stream, const epgx::PruneArgs &a) {
    using namespace epgx;
    const dim3 grid((unsigned)a.nblocks), block(64);
    switch (a.kdim) {
    case 1: hipLaunchKernelGGL(prune_shift_kernel<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(prune_shift_kernel<2>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(prune_shift_kernel<3>, grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(prune_shift_kernel<4>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prune_final_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_prune_read(hipStream_t stream, const epgx::PruneReadArgs &a) {
    using namespace epgx;
    const int64_t blocks = a.nvox < PRUNE_MAX_BLOCKS ? a.nvox : PRUNE_MAX_BLOCKS;
    hipLaunchKernelGGL(prune_read_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_coords_widen(hipStream_t stream, const epgx::CoordsWidenArgs &a) {
    using namespace epgx;
    const int64_t total = a.nvox * a.kd * PRUNE_K;
    const int64_t want = (total + 255) / 256;
    hipLaunchKernelGGL(coords_widen_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

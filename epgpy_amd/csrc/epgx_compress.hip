// epgx_compress.hip -- SVD compression of a dictionary that stays in HBM (include/epgx.h epgx_signal_gram, epgx_signal_project):
//      G[s,t]    = sum over valid a of D[s,a] conj(D[t,a])         (gram_kernel + gram_reduce_kernel; Hermitian, nrec x nrec)
//      out[r,c]  = sum_t conj(B[t,r]) X[t,c]                       (project_kernel; B = the leading eigenvectors of G, from the host)
// Both are complex products on v_mfma_f64_16x16x4_f64, four instructions per tile and step of 4 along the summed index, as in
// epgx_match.hip.  A operand: lane l holds row (l & 15), summed index (l >> 4); B operand: lane l holds summed index (l >> 4),
// column (l & 15); C/D: register r of lane l is row (l >> 4) + 4 r, column (l & 15).
//
// gram_kernel.  The summed index is the atom, the contiguous one of the dictionary, while both operands want 16 records x 4
// atoms: read from HBM that would be 16 rows one row stride apart per load.  So a workgroup of GRAM_WAVES = 4 wavefronts, which
// owns one 64 x 64 block (I, J), I <= J, of G and one split of the atoms, stages [64 records][GRAM_KC = 16 atoms] of record block
// I and of record block J through LDS: thread i loads atom (i & 15) of records (i >> 4) + 16 u -- 16 lanes read 256 contiguous
// bytes -- one chunk ahead in registers, so the loads of chunk c + 1 fly while chunk c is multiplied.  Atoms whose n_a is not a
// finite number > 0 and atoms beyond the split are replaced by zeros THERE, by a select (NaN * 0 is NaN), records beyond nrec
// likewise.  The LDS image has a row pitch of 17 elements (272 bytes): the stores are conflict-free, and of the four 16-lane
// groups of the ds_read_b128 that fetches an operand (rows 0-3, 12-15 of one atom with rows 4-11 of the next) two lanes meet
// on one bank -- 2-way on 20 reads per 64 MFMAs of 64 cycles each, which is noise; an unpadded pitch of 256 bytes would put
// all 16 rows on one bank.
// Wavefront w takes row tile w of block I against the four column tiles of block J (64 accumulator registers); on a diagonal
// block only the column tiles j >= w, so that of the 16 x 16 tiles of G only the pairs I <= J are computed:
//      Re G += ar br,  Im G += ai br,  Re G += ai bi,  Im G += (-ar) bi
// Every (split, block) writes its entries s <= t into the split's partial Gram in scratch; nothing else is written.
//
// gram_reduce_kernel: one lane per entry s <= t sums the partials in ascending split order and writes G[s,t] and G[t,s] = the
// same real part, the negated imaginary part; the diagonal gets an imaginary part of exactly 0.  No atomics.
//
// Determinism of G.  A split consumes its atoms in steps of 4 from its first atom, in the order above, whatever the workgroup;
// the splits are added in ascending order.  The bits of G depend on the valid columns of D, nrec, natoms and nsplit only.
//
// project_kernel<NR, NC>.  A wavefront owns NC tiles of 16 columns of X and all NR = ceil(rank / 16) tiles of basis vectors
// (NR x NC = 1 x 4, 2 x 2 or 4 x 1: 64 accumulator registers), so every column of X is read once per launch whatever the rank:
// lane l loads X[t + (l >> 4)][c0 + (l & 15)], 16 lanes 256 contiguous bytes, PROJ_UNROLL = 4 steps (16 records) in flight per
// wavefront before their MFMAs.  The basis (16 nrec rank bytes, at most 1 MiB at 1000 x 64) is read through L2 by the same kind
// of load: every wavefront walks it in the same order, it stays resident, and without LDS there is no barrier -- the wavefronts
// of a workgroup share nothing.
//      Re out += br xr,  Im out += br xi,  Re out += bi xi,  Im out += (-bi) xr
// The records are consumed in steps of 4 from t = 0, the tail padded with zeros in both operands: the bits of out[r,c] depend on
// column c of X, column r of B and nrec alone.  Non-finite values of X are not filtered: they reach every out[r,c] of their column.
// Plain vector stores only.
#include "epgx_compress.h"

namespace epgx {

typedef double v4d __attribute__((ext_vector_type(4)));

// atom atom0 + (thread & 15) of records rec0 + (thread >> 4) + 16 u, zeros for an invalid atom, beyond the split, beyond nrec
__device__ __forceinline__ void gram_fetch(const GramArgs &a, int64_t atom0, int64_t a1, int rec0, d2 (&x)[4]) {
    int64_t at = atom0 + (threadIdx.x & 15);
    const bool inside = at < a1;
    at = inside ? at : a1 - 1;
    const double n = a.norms[at];
    const bool valid = inside && n > 0.0 && __builtin_isfinite(n);
    const d2 *col = a.dict + at;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rec = rec0 + (int)(threadIdx.x >> 4) + 16 * u;
        const d2 v = col[(int64_t)(rec < a.nrec ? rec : a.nrec - 1) * a.dict_stride];
        x[u] = valid && rec < a.nrec ? v : d2{0.0, 0.0};
    }
}

__global__ void __launch_bounds__(GRAM_WAVES * 64) gram_kernel(const GramArgs a) {
    __shared__ d2 img[2][GRAM_BLOCK][GRAM_LD];                     // record blocks I and J, [record][atom of the chunk]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = lane & 15, grp = lane >> 4;
    const int pair = (int)(blockIdx.x % (unsigned)a.npair), split = (int)(blockIdx.x / (unsigned)a.npair);
    int bi = 0, rem = pair;
    while (rem >= a.nblock - bi) {                                 // pairs row by row: (0,0) .. (0,nblock-1), (1,1) ..
        rem -= a.nblock - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    int64_t a0, a1;
    match_split(a.natoms, a.nsplit, split, &a0, &a1);

    const int i0 = bi * GRAM_BLOCK + wave * GRAM_TILE;
    bool act[GRAM_WAVES];
#pragma unroll
    for (int j = 0; j < GRAM_WAVES; ++j) act[j] = i0 < a.nrec && bj * GRAM_BLOCK + j * GRAM_TILE < a.nrec && !(diag && j < wave);
    v4d cr[GRAM_WAVES], ci[GRAM_WAVES];
#pragma unroll
    for (int j = 0; j < GRAM_WAVES; ++j) cr[j] = ci[j] = v4d{0.0, 0.0, 0.0, 0.0};

    const int srow = threadIdx.x >> 4, scol = threadIdx.x & 15;
    const d2 (*imgj)[GRAM_LD] = img[diag ? 0 : 1];
    d2 x[4], y[4];
    const int64_t nchunk = (a1 - a0 + GRAM_KC - 1) / GRAM_KC;
    gram_fetch(a, a0, a1, bi * GRAM_BLOCK, x);
    if (!diag) gram_fetch(a, a0, a1, bj * GRAM_BLOCK, y);
    for (int64_t c = 0; c < nchunk; ++c) {
        __syncthreads();                                           // (the reads of chunk c - 1 are done)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            img[0][srow + 16 * u][scol] = x[u];
            if (!diag) img[1][srow + 16 * u][scol] = y[u];
        }
        __syncthreads();
        if (c + 1 < nchunk) {
            gram_fetch(a, a0 + (c + 1) * GRAM_KC, a1, bi * GRAM_BLOCK, x);
            if (!diag) gram_fetch(a, a0 + (c + 1) * GRAM_KC, a1, bj * GRAM_BLOCK, y);
        }
        d2 av[GRAM_KC / GRAM_STEP];
#pragma unroll
        for (int k = 0; k < GRAM_KC / GRAM_STEP; ++k) av[k] = img[0][wave * GRAM_TILE + col][k * GRAM_STEP + grp];
#pragma unroll
        for (int j = 0; j < GRAM_WAVES; ++j) {
            if (!act[j]) continue;                                 // (wave-uniform: one branch per tile and chunk)
#pragma unroll
            for (int k = 0; k < GRAM_KC / GRAM_STEP; ++k) {
                const d2 bv = imgj[j * GRAM_TILE + col][k * GRAM_STEP + grp];
                const double ar = av[k].x, ai = av[k].y, nar = -av[k].x;
                cr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bv.x, cr[j], 0, 0, 0);
                ci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bv.x, ci[j], 0, 0, 0);
                cr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bv.y, cr[j], 0, 0, 0);
                ci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nar, bv.y, ci[j], 0, 0, 0);
            }
        }
    }

    // register r of this lane: G[i0 + grp + 4 r][bj * 64 + 16 j + col]
    d2 *part = a.part + (int64_t)split * a.nrec * a.nrec;
#pragma unroll
    for (int j = 0; j < GRAM_WAVES; ++j) {
        if (!act[j]) continue;
        const int t = bj * GRAM_BLOCK + j * GRAM_TILE + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = i0 + grp + 4 * r;
            if (s < a.nrec && t < a.nrec && s <= t) part[(int64_t)s * a.nrec + t] = d2{cr[j][r], ci[j][r]};
        }
    }
}

__global__ void __launch_bounds__(256) gram_reduce_kernel(const GramReduceArgs a) {
    const int64_t nn = (int64_t)a.nrec * a.nrec;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nn) return;
    const int64_t s = idx / a.nrec, t = idx % a.nrec;
    if (s > t) return;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < a.nsplit; ++k) {
        const d2 p = a.part[(int64_t)k * nn + idx];
        re += p.x;
        im += p.y;
    }
    if (s == t) {
        a.out[idx] = d2{re, 0.0};
    } else {
        a.out[idx] = d2{re, im};
        a.out[t * a.nrec + s] = d2{re, -im};
    }
}

template <int NR, int NC>
__global__ void __launch_bounds__(PROJ_WAVES * 64) project_kernel(const ProjectArgs a) {
    static_assert(NR * NC == PROJ_TILES, "64 accumulator registers");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = lane & 15, grp = lane >> 4;
    const int64_t c0 = ((int64_t)blockIdx.x * PROJ_WAVES + wave) * (NC * PROJ_TILE);
    if (c0 >= a.ncol) return;                                      // (wave-uniform; the kernel has no barrier)

    const d2 *xp[NC];
#pragma unroll
    for (int v = 0; v < NC; ++v) {
        const int64_t c = c0 + v * PROJ_TILE + col;
        xp[v] = a.src + (c < a.ncol ? c : a.ncol - 1);             // columns beyond ncol repeat the last one and are not stored
    }
    int rr[NR];
    bool rok[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = q * PROJ_TILE + col;
        rok[q] = r < a.rank;
        rr[q] = rok[q] ? r : a.rank - 1;
    }
    v4d cr[NR][NC], ci[NR][NC];
#pragma unroll
    for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int v = 0; v < NC; ++v) cr[q][v] = ci[q][v] = v4d{0.0, 0.0, 0.0, 0.0};

    const int nstep = (a.nrec + PROJ_STEP - 1) / PROJ_STEP;
    for (int s0 = 0; s0 < nstep; s0 += PROJ_UNROLL) {
        d2 xv[PROJ_UNROLL][NC], bv[PROJ_UNROLL][NR];
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {
            const int t = (s0 + u) * PROJ_STEP + grp;
            const bool tok = t < a.nrec;
            const int64_t tc = tok ? t : a.nrec - 1;
#pragma unroll
            for (int v = 0; v < NC; ++v) {
                const d2 x = xp[v][tc * a.src_stride];
                xv[u][v] = tok ? x : d2{0.0, 0.0};
            }
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const d2 b = a.basis[tc * a.rank + rr[q]];
                bv[u][q] = tok && rok[q] ? b : d2{0.0, 0.0};
            }
        }
#pragma unroll
        for (int u = 0; u < PROJ_UNROLL; ++u) {
            if (s0 + u >= nstep) break;                            // (wave-uniform: no step beyond the padded tail)
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const double br = bv[u][q].x, bi = bv[u][q].y, nbi = -bv[u][q].y;
#pragma unroll
                for (int v = 0; v < NC; ++v) {
                    cr[q][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(br, xv[u][v].x, cr[q][v], 0, 0, 0);
                    ci[q][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(br, xv[u][v].y, ci[q][v], 0, 0, 0);
                    cr[q][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(bi, xv[u][v].y, cr[q][v], 0, 0, 0);
                    ci[q][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(nbi, xv[u][v].x, ci[q][v], 0, 0, 0);
                }
            }
        }
    }

    // register e of this lane: out[16 q + grp + 4 e][c0 + 16 v + col]
#pragma unroll
    for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = q * PROJ_TILE + grp + 4 * e;
#pragma unroll
            for (int v = 0; v < NC; ++v) {
                const int64_t c = c0 + v * PROJ_TILE + col;
                if (r < a.rank && c < a.ncol) a.out[(int64_t)r * a.out_stride + c] = d2{cr[q][v][e], ci[q][v][e]};
            }
        }
}

}  // namespace epgx

hipError_t epgx_launch_gram(hipStream_t stream, const epgx::GramArgs &a) {
    hipLaunchKernelGGL(epgx::gram_kernel, dim3((unsigned)((int64_t)a.npair * a.nsplit)), dim3(epgx::GRAM_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_gram_reduce(hipStream_t stream, const epgx::GramReduceArgs &a) {
    const int64_t blocks = ((int64_t)a.nrec * a.nrec + 255) / 256;
    hipLaunchKernelGGL(epgx::gram_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <int NR, int NC>
static hipError_t launch_project(hipStream_t stream, const epgx::ProjectArgs &a) {
    const int64_t per = (int64_t)epgx::PROJ_WAVES * NC * epgx::PROJ_TILE;
    hipLaunchKernelGGL((epgx::project_kernel<NR, NC>), dim3((unsigned)((a.ncol + per - 1) / per)), dim3(epgx::PROJ_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_project(hipStream_t stream, const epgx::ProjectArgs &a) {
    if (a.rank <= 16) return launch_project<1, 4>(stream, a);
    if (a.rank <= 32) return launch_project<2, 2>(stream, a);
    return launch_project<4, 1>(stream, a);
}

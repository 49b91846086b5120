// epgx_match.hip -- dictionary matching on records that stay in HBM (include/epgx.h epgx_signal_norms, epgx_signal_match):
//      n_a    = sum_t |D[t,a]|^2                          c[a,m] = sum_t conj(D[t,a]) S[t,m]
//      q[a,m] = |c[a,m]|^2 / n_a                          idx[m] = argmax_a q[a,m], the lowest a among equal q
// The correlation matrix [natoms][nmeas] is never stored: match_kernel is a complex GEMM whose epilogue keeps, per voxel, the
// best (q, a, c) seen so far in registers.
//
// match_kernel.  A workgroup of MATCH_WAVES wavefronts owns MATCH_VOX = 64 voxels and one split of the atoms.  The voxels'
// records lie in LDS ([chunk][64] complex128; nrec <= MATCH_CHUNK = 32: staged once, no barrier afterwards; longer signals in
// chunks of MATCH_CHUNK records, 32 KiB, with two barriers each).  Per pass every wavefront takes one tile of 16 atoms and accumulates
// Re c and Im c of 16 atoms x 64 voxels with v_mfma_f64_16x16x4_f64, four instructions per voxel tile and step of 4 records:
//      Re c += dr sr,  Re c += di si,  Im c += dr si,  Im c += (-di) sr
// A (atoms): lane l holds D[t + (l >> 4)][atom0 + (l & 15)] -- one 16-byte load, 16 lanes read 256 contiguous bytes.
// B (voxels): lane l holds S[t + (l >> 4)][voxel0 + (l & 15)] from LDS.  C/D: register r of lane l is atom atom0 + (l >> 4) + 4 r,
// voxel voxel0 + (l & 15).  fp64 MFMA and fp64 VALU share a pipe: the gain over a v_fma_f64 tile is not the rate but
// the operands -- no broadcast of the 16 x 4 atom values to every lane.
//
// Determinism.  The records of a pair are consumed in steps of 4 from t = 0, the tail padded with zeros (both operands), in
// the order above; LDS chunks only stage them.  The bits of c[a,m] depend on column a, column m and nrec alone -- not on nmeas,
// the place of the voxel or atom in a tile, the splits or other columns.  q = (cr^2 + ci^2) * (1 / n_a) and the rule "greater q
// wins, on equal q the lower a" is a total order, so the order in which lanes, wavefronts and splits meet does not matter.
// An atom whose n_a is not a finite number > 0 never takes part; a q that is NaN never wins.
//
// match_merge_kernel: one lane per voxel reduces the splits by the same rule, then scale = c / n and score = sqrt(q / sum |S|^2)
// (0 for an all-zero signal, at most 1).  No atomics.  Plain vector stores only.
#include "epgx_match.h"

namespace epgx {

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) norms_kernel(const d2 *dict, int64_t stride, int32_t nrec, int64_t natoms, double *out) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= natoms) return;
    const d2 *col = dict + a;
    double n = 0.0;
    int t = 0;
    for (; t + 4 <= nrec; t += 4) {      // four loads in flight; the sum itself in record order
        d2 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = col[(int64_t)(t + u) * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            n = fma(x[u].x, x[u].x, n);
            n = fma(x[u].y, x[u].y, n);
        }
    }
    for (; t < nrec; ++t) {
        const d2 x = col[(int64_t)t * stride];
        n = fma(x.x, x.x, n);
        n = fma(x.y, x.y, n);
    }
    out[a] = n;
}

// greater q wins, on equal q the lower atom; a NaN never wins (and nothing wins against one: the caller never stores one)
__device__ __forceinline__ bool match_better(double q, int64_t a, double bq, int64_t ba) {
    return q > bq || (q == bq && a < ba);
}

// records [c * chunk, (c + 1) * chunk) of the workgroup's 64 voxels -> LDS, zeros beyond nrec; voxels beyond nmeas repeat the last one
__device__ __forceinline__ void match_stage(const MatchArgs &a, d2 *lds, int c, int64_t m0) {
    for (int i = threadIdx.x; i < a.chunk * MATCH_VOX; i += MATCH_WAVES * 64) {
        const int t = c * a.chunk + (i >> 6);
        int64_t m = m0 + (i & 63);
        m = m < a.nmeas ? m : a.nmeas - 1;
        d2 v = d2{0.0, 0.0};
        if (t < a.nrec) v = a.sig[(int64_t)t * a.sig_stride + m];
        lds[i] = v;
    }
}

__global__ void __launch_bounds__(MATCH_WAVES * 64) match_kernel(const MatchArgs a) {
    extern __shared__ d2 match_sig[];                              // [chunk][MATCH_VOX]
    __shared__ MatchPartial match_best[MATCH_WAVES][MATCH_VOX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = lane & 15, grp = lane >> 4;
    const int64_t m0 = (int64_t)(blockIdx.x % a.nvt) * MATCH_VOX;
    const int split = (int)(blockIdx.x / a.nvt);
    int64_t a0, a1;
    match_split(a.natoms, a.nsplit, split, &a0, &a1);

    double bq[MATCH_VT], bcr[MATCH_VT], bci[MATCH_VT];
    int64_t ba[MATCH_VT];
#pragma unroll
    for (int v = 0; v < MATCH_VT; ++v) {
        bq[v] = -1.0;
        ba[v] = -1;
        bcr[v] = bci[v] = 0.0;
    }

    const int64_t ntile = (a1 - a0 + MATCH_TILE - 1) / MATCH_TILE;
    const int64_t npass = (ntile + MATCH_WAVES - 1) / MATCH_WAVES;
    if (a.nchunk == 1 && npass > 0) {
        match_stage(a, match_sig, 0, m0);
        __syncthreads();
    }
    for (int64_t pass = 0; pass < npass; ++pass) {      // (the same trip count in every wavefront: the barriers below)
        const int64_t atom0 = a0 + (pass * MATCH_WAVES + wave) * MATCH_TILE;
        const bool active = atom0 < a1;                   // (wave-uniform)
        int64_t arow = atom0 + col;
        arow = arow < a1 ? arow : a1 - 1;                 // rows beyond the split read its last atom and are not compared
        const d2 *dcol = a.dict + arow;

        v4d cr[MATCH_VT], ci[MATCH_VT];
#pragma unroll
        for (int v = 0; v < MATCH_VT; ++v) cr[v] = ci[v] = v4d{0.0, 0.0, 0.0, 0.0};

        for (int c = 0; c < a.nchunk; ++c) {
            if (a.nchunk > 1) {
                __syncthreads();
                match_stage(a, match_sig, c, m0);
                __syncthreads();
            }
            if (!active) continue;
            const int t0 = c * a.chunk;
            const int t1 = t0 + a.chunk < a.nrec ? t0 + a.chunk : a.nrec;
            for (int t = t0; t < t1; t += MATCH_STEP) {
                const int tt = t + grp;
                d2 d = dcol[(int64_t)(tt < a.nrec ? tt : a.nrec - 1) * a.dict_stride];
                if (tt >= a.nrec) d = d2{0.0, 0.0};
                const double dr = d.x, di = d.y, ndi = -d.y;
                const d2 *srow = match_sig + (t - t0 + grp) * MATCH_VOX + col;
#pragma unroll
                for (int v = 0; v < MATCH_VT; ++v) {
                    const d2 s = srow[v * MATCH_TILE];
                    cr[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(dr, s.x, cr[v], 0, 0, 0);
                    ci[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(dr, s.y, ci[v], 0, 0, 0);
                    cr[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(di, s.y, cr[v], 0, 0, 0);
                    ci[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(ndi, s.x, ci[v], 0, 0, 0);
                }
            }
        }
        if (!active) continue;

        // register r of this lane: atom atom0 + grp + 4 r against voxel m0 + 16 v + col
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t atom = atom0 + grp + 4 * r;
            const double n = a.norms[atom < a1 ? atom : a1 - 1];
            const bool valid = atom < a1 && n > 0.0 && __builtin_isfinite(n);
            const double inv = 1.0 / n;
#pragma unroll
            for (int v = 0; v < MATCH_VT; ++v) {
                const double q = fma(cr[v][r], cr[v][r], ci[v][r] * ci[v][r]) * inv;
                if (valid && match_better(q, atom, bq[v], ba[v])) {
                    bq[v] = q;
                    ba[v] = atom;
                    bcr[v] = cr[v][r];
                    bci[v] = ci[v][r];
                }
            }
        }
    }

    // the four lane groups of a wavefront hold candidates for the same voxels: meet over lanes l ^ 16, l ^ 32
#pragma unroll
    for (int v = 0; v < MATCH_VT; ++v) {
#pragma unroll
        for (int off = 16; off < 64; off *= 2) {
            const double oq = __shfl_xor(bq[v], off), ocr = __shfl_xor(bcr[v], off), oci = __shfl_xor(bci[v], off);
            const int64_t oa = __shfl_xor((long long)ba[v], off);
            if (oa >= 0 && (ba[v] < 0 || match_better(oq, oa, bq[v], ba[v]))) {
                bq[v] = oq;
                ba[v] = oa;
                bcr[v] = ocr;
                bci[v] = oci;
            }
        }
        if (grp == 0) match_best[wave][v * MATCH_TILE + col] = MatchPartial{bq[v], ba[v], bcr[v], bci[v]};
    }
    __syncthreads();
    if (threadIdx.x < MATCH_VOX && m0 + threadIdx.x < a.nmeas) {
        const MatchPartial *mine = &match_best[0][threadIdx.x];
        double q = mine->q, cr = mine->cr, ci = mine->ci;
        int64_t at = mine->a;
#pragma unroll
        for (int w = 1; w < MATCH_WAVES; ++w) {
            const MatchPartial *o = &match_best[w][threadIdx.x];
            const double oq = o->q, ocr = o->cr, oci = o->ci;
            const int64_t oa = o->a;
            if (oa >= 0 && (at < 0 || match_better(oq, oa, q, at))) {
                q = oq;
                at = oa;
                cr = ocr;
                ci = oci;
            }
        }
        MatchPartial *dst = a.part + (int64_t)split * a.nmeas + m0 + threadIdx.x;
        dst->q = q;
        dst->a = at;
        dst->cr = cr;
        dst->ci = ci;
    }
}

__global__ void __launch_bounds__(256) match_merge_kernel(const MatchMergeArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.nmeas) return;
    MatchPartial best = a.part[m];
    for (int s = 1; s < a.nsplit; ++s) {
        const MatchPartial o = a.part[(int64_t)s * a.nmeas + m];
        if (o.a >= 0 && (best.a < 0 || match_better(o.q, o.a, best.q, best.a))) best = o;
    }
    double energy = 0.0;
    const d2 *col = a.sig + m;
    for (int t = 0; t < a.nrec; ++t) {
        const d2 x = col[(int64_t)t * a.sig_stride];
        energy = fma(x.x, x.x, energy);
        energy = fma(x.y, x.y, energy);
    }
    int64_t index = -1;
    d2 scale = d2{0.0, 0.0};
    double score = 0.0;
    if (best.a >= 0 && __builtin_isfinite(best.q)) {
        const double n = a.norms[best.a];
        index = best.a;
        scale = d2{best.cr / n, best.ci / n};
        if (energy > 0.0) {
            score = fmin(sqrt(best.q / energy), 1.0);
        }
    }
    a.index[m] = index;
    a.scale[m] = scale;
    a.score[m] = score;
}

}  // namespace epgx

hipError_t epgx_launch_norms(hipStream_t stream, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, double *out) {
    const int64_t blocks = (natoms + 255) / 256;
    hipLaunchKernelGGL(epgx::norms_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const epgx::d2 *)dict, row_stride, nrec, natoms, out);
    return hipGetLastError();
}

hipError_t epgx_launch_match(hipStream_t stream, const epgx::MatchArgs &a) {
    const size_t lds = sizeof(epgx::d2) * (size_t)a.chunk * epgx::MATCH_VOX;      // <= 32 KiB, next to 8 KiB of match_best
    hipLaunchKernelGGL(epgx::match_kernel, dim3((unsigned)(a.nvt * a.nsplit)), dim3(epgx::MATCH_WAVES * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_match_merge(hipStream_t stream, const epgx::MatchMergeArgs &a) {
    const int64_t blocks = (a.nmeas + 255) / 256;
    hipLaunchKernelGGL(epgx::match_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

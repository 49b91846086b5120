// epgx_match32.hip -- single-precision dictionary matching (include/epgx.h epgx_signal_norms_c64, epgx_signal_match_c64).  A
// complex64 dictionary IS the complex128 one rounded once (epgx_signal_narrow: narrow_kernel of epgx_small_kernels.hip.h, round
// to nearest even per component); matching is defined on the rounded operands D32, S32:
//      n_a    = sum_t |D32[t,a]|^2                  in fp64, record order (f32 -> f64 is exact)
//      c[a,m] = sum_t conj(D32[t,a]) S32[t,m]       in fp32 on v_mfma_f32_16x16x4_f32 (an exact k-ordered fmaf chain)
//      q[a,m] = (Re c^2 + Im c^2) * (1 / n_a)       in fp64 from the fp32 c, the expression of match_kernel
// and the rule, the partial results of the splits (MatchPartial) and their reduction are those of epgx_match.hip.
//
// match32_kernel keeps the tiling of match_kernel: a workgroup of MATCH_WAVES wavefronts owns MATCH_VOX = 64 voxels and one split
// of the atoms; the voxels' records lie in LDS ([chunk][64] complex64; nrec <= MATCH32_CHUNK = 64 staged once, longer signals
// in chunks of 64 records, 32 KiB, with two barriers each).  Per pass a wavefront takes 16 atoms and accumulates Re c and Im c
// of 16 atoms x 64 voxels, four instructions per voxel tile and step of 4 records:
//      Re c += dr sr,  Im c += dr si,  Re c += di si,  Im c += (-di) sr
// A (atoms): lane l holds D32[t + (l >> 4)][atom0 + (l & 15)] -- one 8-byte load, 16 lanes read 128 contiguous bytes.
// B (voxels): lane l holds S32[t + (l >> 4)][voxel0 + (l & 15)] from LDS.  The operand maps are those of the f64 instruction;
// the ACCUMULATOR map is not: register r of lane l is atom atom0 + 4 (l >> 4) + r (f64: (l >> 4) + 4 r), voxel voxel0 + (l & 15).
// The instruction issues every 32 cycles and a dependent accumulator is ready after 40: the eight accumulators of a step are
// updated round robin (the two updates of one Re c lie 8 instructions apart), never back to back.
//
// Determinism: the records of a pair are consumed in steps of 4 from t = 0 in the order above, the tail padded with zeros in
// both operands; LDS chunks only stage them.  The bits of c[a,m] depend on column a, column m and nrec alone.
// No atomics.  Plain vector stores only.
#include "epgx_match32.h"

namespace epgx {

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) norms32_kernel(const f2 *dict, int64_t stride, int32_t nrec, int64_t natoms, double *out) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= natoms) return;
    const f2 *col = dict + a;
    double n = 0.0;
    int t = 0;
    for (; t + 4 <= nrec; t += 4) {      // four loads in flight; the sum itself in record order
        f2 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = col[(int64_t)(t + u) * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double xr = x[u].x, xi = x[u].y;
            n = fma(xr, xr, n);
            n = fma(xi, xi, n);
        }
    }
    for (; t < nrec; ++t) {
        const f2 x = col[(int64_t)t * stride];
        const double xr = x.x, xi = x.y;
        n = fma(xr, xr, n);
        n = fma(xi, xi, n);
    }
    out[a] = n;
}

// the rule of epgx_match.hip: greater q wins, on equal q the lower atom; a NaN never wins
__device__ __forceinline__ bool match32_better(double q, int64_t a, double bq, int64_t ba) {
    return q > bq || (q == bq && a < ba);
}

// records [c * chunk, (c + 1) * chunk) of the workgroup's 64 voxels -> LDS, zeros beyond nrec; voxels beyond nmeas repeat the last one
__device__ __forceinline__ void match32_stage(const Match32Args &a, f2 *lds, int c, int64_t m0) {
    for (int i = threadIdx.x; i < a.chunk * MATCH_VOX; i += MATCH_WAVES * 64) {
        const int t = c * a.chunk + (i >> 6);
        int64_t m = m0 + (i & 63);
        m = m < a.nmeas ? m : a.nmeas - 1;
        f2 v = f2{0.0f, 0.0f};
        if (t < a.nrec) v = a.sig[(int64_t)t * a.sig_stride + m];
        lds[i] = v;
    }
}

// 90 VGPRs, no AGPRs, no scratch at four waves per SIMD: four workgroups of 40 KiB LDS fill the 160 KiB of a compute unit
__global__ void __launch_bounds__(MATCH_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) match32_kernel(const Match32Args a) {
    extern __shared__ f2 match32_sig[];                            // [chunk][MATCH_VOX]
    __shared__ MatchPartial match32_best[MATCH_WAVES][MATCH_VOX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = lane & 15, grp = lane >> 4;
    const int64_t m0 = (int64_t)(blockIdx.x % a.nvt) * MATCH_VOX;
    const int split = (int)(blockIdx.x / a.nvt);
    int64_t a0, a1;
    match_split(a.natoms, a.nsplit, split, &a0, &a1);

    double bq[MATCH_VT];
    float bcr[MATCH_VT], bci[MATCH_VT];
    int64_t ba[MATCH_VT];
#pragma unroll
    for (int v = 0; v < MATCH_VT; ++v) {
        bq[v] = -1.0;
        ba[v] = -1;
        bcr[v] = bci[v] = 0.0f;
    }

    const int64_t ntile = (a1 - a0 + MATCH_TILE - 1) / MATCH_TILE;
    const int64_t npass = (ntile + MATCH_WAVES - 1) / MATCH_WAVES;
    if (a.nchunk == 1 && npass > 0) {
        match32_stage(a, match32_sig, 0, m0);
        __syncthreads();
    }
    for (int64_t pass = 0; pass < npass; ++pass) {      // (the same trip count in every wavefront: the barriers below)
        const int64_t atom0 = a0 + (pass * MATCH_WAVES + wave) * MATCH_TILE;
        const bool active = atom0 < a1;                   // (wave-uniform)
        int64_t arow = atom0 + col;
        arow = arow < a1 ? arow : a1 - 1;                 // rows beyond the split read its last atom and are not compared
        const f2 *dcol = a.dict + arow;

        v4f cr[MATCH_VT], ci[MATCH_VT];
#pragma unroll
        for (int v = 0; v < MATCH_VT; ++v) cr[v] = ci[v] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

        for (int c = 0; c < a.nchunk; ++c) {
            if (a.nchunk > 1) {
                __syncthreads();
                match32_stage(a, match32_sig, c, m0);
                __syncthreads();
            }
            if (!active) continue;
            const int t0 = c * a.chunk;
            const int t1 = t0 + a.chunk < a.nrec ? t0 + a.chunk : a.nrec;
            for (int t = t0; t < t1; t += MATCH_STEP) {
                const int tt = t + grp;
                f2 d = dcol[(int64_t)(tt < a.nrec ? tt : a.nrec - 1) * a.dict_stride];
                if (tt >= a.nrec) d = f2{0.0f, 0.0f};
                const float dr = d.x, di = d.y, ndi = -d.y;
                const f2 *srow = match32_sig + (t - t0 + grp) * MATCH_VOX + col;
                f2 s[MATCH_VT];
#pragma unroll
                for (int v = 0; v < MATCH_VT; ++v) s[v] = srow[v * MATCH_TILE];
#pragma unroll
                for (int v = 0; v < MATCH_VT; ++v) {
                    cr[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(dr, s[v].x, cr[v], 0, 0, 0);
                    ci[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(dr, s[v].y, ci[v], 0, 0, 0);
                }
#pragma unroll
                for (int v = 0; v < MATCH_VT; ++v) {
                    cr[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(di, s[v].y, cr[v], 0, 0, 0);
                    ci[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(ndi, s[v].x, ci[v], 0, 0, 0);
                }
            }
        }
        if (!active) continue;

        // register r of this lane: atom atom0 + 4 grp + r against voxel m0 + 16 v + col
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t atom = atom0 + 4 * grp + r;
            const double n = a.norms[atom < a1 ? atom : a1 - 1];
            const bool valid = atom < a1 && n > 0.0 && __builtin_isfinite(n);
            const double inv = 1.0 / n;
#pragma unroll
            for (int v = 0; v < MATCH_VT; ++v) {
                const double xr = cr[v][r], xi = ci[v][r];
                const double q = fma(xr, xr, xi * xi) * inv;
                if (valid && match32_better(q, atom, bq[v], ba[v])) {
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
            const double oq = __shfl_xor(bq[v], off);
            const float ocr = __shfl_xor(bcr[v], off), oci = __shfl_xor(bci[v], off);
            const int64_t oa = __shfl_xor((long long)ba[v], off);
            if (oa >= 0 && (ba[v] < 0 || match32_better(oq, oa, bq[v], ba[v]))) {
                bq[v] = oq;
                ba[v] = oa;
                bcr[v] = ocr;
                bci[v] = oci;
            }
        }
        if (grp == 0) match32_best[wave][v * MATCH_TILE + col] = MatchPartial{bq[v], ba[v], (double)bcr[v], (double)bci[v]};
    }
    __syncthreads();
    if (threadIdx.x < MATCH_VOX && m0 + threadIdx.x < a.nmeas) {
        const MatchPartial *mine = &match32_best[0][threadIdx.x];
        double q = mine->q, cr = mine->cr, ci = mine->ci;
        int64_t at = mine->a;
#pragma unroll
        for (int w = 1; w < MATCH_WAVES; ++w) {
            const MatchPartial *o = &match32_best[w][threadIdx.x];
            const double oq = o->q, ocr = o->cr, oci = o->ci;
            const int64_t oa = o->a;
            if (oa >= 0 && (at < 0 || match32_better(oq, oa, q, at))) {
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

// match_merge_kernel with the energy read from complex64 signals (summed in fp64, record order)
__global__ void __launch_bounds__(256) match32_merge_kernel(const Match32MergeArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.nmeas) return;
    MatchPartial best = a.part[m];
    for (int s = 1; s < a.nsplit; ++s) {
        const MatchPartial o = a.part[(int64_t)s * a.nmeas + m];
        if (o.a >= 0 && (best.a < 0 || match32_better(o.q, o.a, best.q, best.a))) best = o;
    }
    double energy = 0.0;
    const f2 *col = a.sig + m;
    for (int t = 0; t < a.nrec; ++t) {
        const f2 x = col[(int64_t)t * a.sig_stride];
        const double xr = x.x, xi = x.y;
        energy = fma(xr, xr, energy);
        energy = fma(xi, xi, energy);
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

hipError_t epgx_launch_norms32(hipStream_t stream, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, double *out) {
    const int64_t blocks = (natoms + 255) / 256;
    hipLaunchKernelGGL(epgx::norms32_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const epgx::f2 *)dict, row_stride, nrec, natoms, out);
    return hipGetLastError();
}

hipError_t epgx_launch_match32(hipStream_t stream, const epgx::Match32Args &a) {
    const size_t lds = sizeof(epgx::f2) * (size_t)a.chunk * epgx::MATCH_VOX;      // <= 32 KiB, next to 8 KiB of match32_best
    hipLaunchKernelGGL(epgx::match32_kernel, dim3((unsigned)(a.nvt * a.nsplit)), dim3(epgx::MATCH_WAVES * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t epgx_launch_match32_merge(hipStream_t stream, const epgx::Match32MergeArgs &a) {
    const int64_t blocks = (a.nmeas + 255) / 256;
    hipLaunchKernelGGL(epgx::match32_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

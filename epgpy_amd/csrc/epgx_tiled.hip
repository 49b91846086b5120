// epgx_tiled.hip -- state matrices of any length (the reference's unbounded growth, epgpy/shift.py:86,98): temporal tiling
// with overlapping halos.
//   tiled_kernel<M, H, NSP>   the state lives in HBM as [nvox][3][Kbuf] (two buffers that alternate between blocks of
//       records).  One wavefront owns one (voxel, tile): it loads a WINDOW of 64 M consecutive orders (M per lane, the
//       contiguous layout of run_contig_kernel) = the tile's interior of W = 64 M - 2 H orders plus a halo of H orders on
//       either side (tile 0: the window starts at k = 0, where the k = 0 fold takes the place of the lower halo), runs the
//       block in registers with the record bodies of the per-timestep kernels, and writes the interior back.  Every operator
//       but the shift acts on each order by itself, and a shift by one spoils at most one order at each edge of the window
//       (the upper edge receives a zero, the lower edge of a tile other than 0 the fold of an order it does not hold), so
//       after a block whose shifts add up to at most H the interior is exact.  Only tile 0 holds k = 0: the probes, the
//       recovery / equilibrium terms and the fold are its own (Tile::k0).
//   tiled_shift_kernel   a shift by |n| > H as a launch of its own: an HBM-bound copy with the k = 0 fold.
//   tiled_equilibrium_kernel   Z_0 = density of every voxel.
//   tiled_deriv_kernel<M, H, NSP, V>   the same for a first-order derivative plan: the state and V derivative states of a
//       voxel live in HBM as [nvox][1 + V][3][Kbuf]; a wavefront keeps the 1 + V windows of its (voxel, tile) in registers and
//       walks the records with deriv_kernel's flag-tested body (deriv_record, epgx_deriv_record.hip.h) under the Tile policy.
//       A derivative state never populates an order the state does not, and a shift spoils the same edge orders of all
//       1 + V windows: the schedule (blocks, halos, tiles) is the plain one.  At an ADC tile 0 stores 1 + V rows.
// Shifts by 2 .. H inside a block are |n| records of S(+-1) (the host expands them: the same moves as shift_lds).
#include <algorithm>

#include "epgx_deriv_record.hip.h"
#include "epgx_launch_tiled.h"

using namespace epgx;

namespace epgx {

// a window of orders [base, base + 64 M) of a voxel; k0: the window holds k = 0 (tile 0)
struct Tile {
    static constexpr bool on = false;       // no hand-over between wavefronts: the edges of the window are simply spoiled
    static constexpr bool contig = true;    // order base + M lane + m
    int base = 0;
    bool k0 = true;
};
// (found by argument-dependent lookup from the record bodies: truncation compares orders, k = 0 terms need tile 0)
__device__ __forceinline__ int order_base(const Tile &sx) { return sx.base; }
__device__ __forceinline__ bool holds_k0(const Tile &sx) { return sx.k0; }

template <int M, int H, int NSP>
__global__ void __launch_bounds__(256, (M == 16 ? 1 : 2)) tiled_kernel(const TiledArgs a) {
    constexpr int L = 64 * M, W = L - 2 * H;
    static_assert(W > 0 && H % M == 0 && W % M == 0, "the halo and the interior are whole lanes");
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t v = (int64_t)blockIdx.x * 4 + wib;
    if (v >= a.nvox) return;
    const int t = (int)blockIdx.y;
    Tile sx;
    sx.k0 = t == 0;
    sx.base = t == 0 ? 0 : t * W - H;
    const int Kbuf = a.Kbuf;
    const int k_lane = sx.base + M * lane;
    const bool inb = k_lane < Kbuf;             // (base and Kbuf are multiples of M: a lane's orders are all inside or all above)
    const d2 *src = a.in + (size_t)v * 3 * Kbuf + (inb ? k_lane : 0);
    State<M> s;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        d2 x = {0.0, 0.0}, y = {0.0, 0.0}, z = {0.0, 0.0};
        if (inb) {
            x = src[m];
            y = src[Kbuf + m];
            z = src[2 * Kbuf + m];
        }
        s.Ar[m] = x.x; s.Ai[m] = x.y;
        s.Br[m] = y.x; s.Bi[m] = y.y;
        s.Zr[m] = z.x; s.Zi[m] = z.y;
    }
    const const_rec_t recs = (const_rec_t)(uintptr_t)a.recs;
    const const_f64_t pool = (const_f64_t)(uintptr_t)a.coef;
    const const_i32_t vidx = (const_i32_t)(uintptr_t)a.t.vidx;
    const uint32_t gv = (uint32_t)(a.t.vox0 + v);
    uint32_t p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;
    if (NSP > 0) p0 = (a.t.dense_spaces & 1u) ? gv : (uint32_t)vidx[v];
    if (NSP > 1) p1 = (a.t.dense_spaces & 2u) ? gv : (uint32_t)vidx[a.t.vidx_ld + v];
    if (NSP > 2) p2 = (a.t.dense_spaces & 4u) ? gv : (uint32_t)vidx[2 * a.t.vidx_ld + v];
    if (NSP > 2) p3 = (a.t.dense_spaces & 8u) ? gv : (uint32_t)vidx[3 * a.t.vidx_ld + v];
    double dens = sx.k0 ? a.dens[v] : 0.0;      // (tile 0 alone reads and writes the density: the k = 0 terms are its own)
    const bool l0 = lane == 0 && sx.k0;
    const double oh0 = l0 ? 1.0 : 0.0;          // the k = 0 fold of a shift: tile 0 only
    const uint32_t voff0 = l0 ? 0u : 16u;       // only the k = 0 lane of tile 0 stores a probe
    double eqv = l0 ? dens : 0.0;
    SigCursor sig;
    sig.base = a.signal + v;
    sig.ld = a.signal_ld;
    sig.seq = false;                            // (records carry their row)
    sig.next = sig.base;
    Rec ra = load_rec(recs, a.rec0);
    for (int i = a.rec0; i < a.rec1; i += 2) {
        const Rec rb = load_rec(recs, i + 1);
        dispatch_record<M, NSP, Tile>(s, ra, pool, p0, p1, p2, p3, dens, eqv, oh0, lane, voff0, sig, nullptr, a.coef, sx);
        ra = load_rec(recs, i + 2);
        if (i + 1 < a.rec1) dispatch_record<M, NSP, Tile>(s, rb, pool, p0, p1, p2, p3, dens, eqv, oh0, lane, voff0, sig, nullptr, a.coef, sx);
    }
    // the interior: orders [t W, (t + 1) W) = window offsets [lo, lo + W)
    const int lo = t == 0 ? 0 : H;
    if (inb && M * lane >= lo && M * lane < lo + W) {
        d2 *dst = a.out + (size_t)v * 3 * Kbuf + k_lane;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            d2 x, y, z;
            x.x = s.Ar[m]; x.y = s.Ai[m];
            y.x = s.Br[m]; y.y = s.Bi[m];
            z.x = s.Zr[m]; z.y = s.Zi[m];
            dst[m] = x;
            dst[Kbuf + m] = y;
            dst[2 * Kbuf + m] = z;
        }
    }
    if (l0) a.dens[v] = dens;
}

// one window of [3][Kbuf] complex <-> registers (a lane's M consecutive orders; lanes above Kbuf hold zeros)
template <int M>
__device__ __forceinline__ void load_window(State<M> &s, const d2 *src, int Kbuf, bool inb) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        d2 x = {0.0, 0.0}, y = {0.0, 0.0}, z = {0.0, 0.0};
        if (inb) {
            x = src[m];
            y = src[Kbuf + m];
            z = src[2 * Kbuf + m];
        }
        s.Ar[m] = x.x; s.Ai[m] = x.y;
        s.Br[m] = y.x; s.Bi[m] = y.y;
        s.Zr[m] = z.x; s.Zi[m] = z.y;
    }
}

template <int M>
__device__ __forceinline__ void store_window(const State<M> &s, d2 *dst, int Kbuf) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        d2 x, y, z;
        x.x = s.Ar[m]; x.y = s.Ai[m];
        y.x = s.Br[m]; y.y = s.Bi[m];
        z.x = s.Zr[m]; z.y = s.Zi[m];
        dst[m] = x;
        dst[Kbuf + m] = y;
        dst[2 * Kbuf + m] = z;
    }
}

template <int M, int H, int NSP, int V>
__global__ void __launch_bounds__(256) tiled_deriv_kernel(const TiledDerivArgs da) {
    constexpr int L = 64 * M, W = L - 2 * H;
    static_assert(W > 0 && H % M == 0 && W % M == 0, "the halo and the interior are whole lanes");
    const TiledArgs &a = da.a;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t v = (int64_t)blockIdx.x * 4 + wib;
    if (v >= a.nvox) return;
    const int t = (int)blockIdx.y;
    Tile sx;
    sx.k0 = t == 0;
    sx.base = t == 0 ? 0 : t * W - H;
    const int Kbuf = a.Kbuf;
    const int k_lane = sx.base + M * lane;
    const bool inb = k_lane < Kbuf;             // (base and Kbuf are multiples of M: a lane's orders are all inside or all above)
    const size_t win = (size_t)3 * Kbuf;        // one state window of a voxel; a voxel holds 1 + V of them
    const size_t at = (size_t)v * (1 + V) * win + (inb ? k_lane : 0);
    State<M> s;
    State<M> ds[V];
    load_window<M>(s, a.in + at, Kbuf, inb);
#pragma unroll
    for (int j = 0; j < V; ++j) load_window<M>(ds[j], a.in + at + (size_t)(1 + j) * win, Kbuf, inb);
    const const_rec_t recs = (const_rec_t)(uintptr_t)a.recs;
    const EPGX_CONSTANT u32x8 *drecs = (const EPGX_CONSTANT u32x8 *)(uintptr_t)da.drecs;
    const const_f64_t pool = (const_f64_t)(uintptr_t)a.coef;
    const const_i32_t vidx = (const_i32_t)(uintptr_t)a.t.vidx;
    const uint32_t gv = (uint32_t)(a.t.vox0 + v);
    uint32_t p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;
    if (NSP > 0) p0 = (a.t.dense_spaces & 1u) ? gv : (uint32_t)vidx[v];
    if (NSP > 1) p1 = (a.t.dense_spaces & 2u) ? gv : (uint32_t)vidx[a.t.vidx_ld + v];
    if (NSP > 2) p2 = (a.t.dense_spaces & 4u) ? gv : (uint32_t)vidx[2 * a.t.vidx_ld + v];
    if (NSP > 2) p3 = (a.t.dense_spaces & 8u) ? gv : (uint32_t)vidx[3 * a.t.vidx_ld + v];
    double dens = sx.k0 ? a.dens[v] : 0.0;      // (tile 0 alone reads and writes the density: the k = 0 terms are its own)
    const bool l0 = lane == 0 && sx.k0;
    const double oh0 = l0 ? 1.0 : 0.0;          // the k = 0 fold of a shift: tile 0 only
    const uint32_t voff0 = l0 ? 0u : 16u;       // only the k = 0 lane of tile 0 stores a probe
    double eqv = l0 ? dens : 0.0;
    d2 *sig_base = a.signal + v;
    for (int i = a.rec0; i < a.rec1; ++i)
        deriv_record<M, NSP, V, Tile>(s, ds, load_rec(recs, i), load_drec(drecs, i), pool, p0, p1, p2, p3, dens, eqv, oh0, lane, voff0, sig_base,
                                      a.signal_ld, da.through_plain, nullptr, a.coef, sx);
    // the interior: orders [t W, (t + 1) W) = window offsets [lo, lo + W)
    const int lo = t == 0 ? 0 : H;
    if (inb && M * lane >= lo && M * lane < lo + W) {
        d2 *dst = a.out + (size_t)v * (1 + V) * win + k_lane;
        store_window<M>(s, dst, Kbuf);
#pragma unroll
        for (int j = 0; j < V; ++j) store_window<M>(ds[j], dst + (size_t)(1 + j) * win, Kbuf);
    }
    if (l0) a.dens[v] = dens;
}

// X_k <- X_{k-n} (k >= n), X_k <- conj(Y_{n-k}) (k < n);  Y_k <- Y_{k+n} (k + n < Kbuf), else 0;  (X, Y) = (A, B) for n > 0,
// (B, A) for n < 0 -- shift_lds over the whole buffer; then the transverse orders above kmax are dropped
__global__ void __launch_bounds__(256) tiled_shift_kernel(const d2 *__restrict__ in, d2 *__restrict__ out, const int64_t nvox,
                                                          const int32_t Kbuf, const int32_t kcov, const int32_t n, const int32_t kmax) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= kcov) return;
    const int an = n > 0 ? n : -n;
    for (int64_t v = blockIdx.y; v < nvox; v += gridDim.y) {
        const d2 *A = in + (size_t)v * 3 * Kbuf, *B = A + Kbuf, *Z = A + 2 * Kbuf;
        const d2 *X = n > 0 ? A : B, *Y = n > 0 ? B : A;
        d2 x, y;
        if (k >= an) {
            x = X[k - an];
        } else {
            x = Y[an - k];
            x.y = -x.y;
        }
        if (k + an < Kbuf) y = Y[k + an];
        else y = d2{0.0, 0.0};
        if (k > kmax) x = y = d2{0.0, 0.0};
        d2 *oA = out + (size_t)v * 3 * Kbuf;
        oA[(n > 0 ? 0 : Kbuf) + k] = x;
        oA[(n > 0 ? Kbuf : 0) + k] = y;
        oA[2 * Kbuf + k] = Z[k];
    }
}

__global__ void __launch_bounds__(256) tiled_equilibrium_kernel(d2 *__restrict__ buf, double *__restrict__ dens,
                                                                const double *__restrict__ dens_in, const int64_t nvox, const int32_t Kbuf,
                                                                const int32_t windows) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    const double d = dens_in ? dens_in[v] : 1.0;
    buf[(size_t)v * windows * 3 * Kbuf + 2 * Kbuf] = d2{d, 0.0};   // (a voxel holds `windows` state windows: the first is S)
    dens[v] = d;
}

}  // namespace epgx

template <int M, int H, int NSP>
static hipError_t launch_tiled(hipStream_t stream, const TiledArgs &a) {
    hipLaunchKernelGGL((tiled_kernel<M, H, NSP>), dim3((unsigned)((a.nvox + 3) / 4), (unsigned)a.tiles), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <int M, int H>
static hipError_t launch_tiled_nsp(hipStream_t stream, const TiledArgs &a, int n_spaces) {
    switch (n_spaces) {
    case 0: return launch_tiled<M, H, 0>(stream, a);
    case 1: return launch_tiled<M, H, 1>(stream, a);
    case 2: return launch_tiled<M, H, 2>(stream, a);
    default: return launch_tiled<M, H, 4>(stream, a);
    }
}

hipError_t epgx_launch_tiled(hipStream_t stream, const TiledArgs &a, int M, int H, int n_spaces) {
    if (a.nvox <= 0 || a.tiles <= 0 || a.tiles > 65535 || (a.nvox + 3) / 4 > 0x7fffffff || a.Kbuf % 64 != 0) return hipErrorInvalidValue;
    if (M == 8 && H == 32) return launch_tiled_nsp<8, 32>(stream, a, n_spaces);
    if (M == 16 && H == 64) return launch_tiled_nsp<16, 64>(stream, a, n_spaces);
    return hipErrorInvalidValue;
}

template <int M, int H, int NSP>
static hipError_t launch_tiled_deriv_v(hipStream_t stream, const TiledDerivArgs &da, int n_vars) {
    const dim3 grid((unsigned)((da.a.nvox + 3) / 4), (unsigned)da.a.tiles);
    switch (n_vars) {
    case 1: hipLaunchKernelGGL((tiled_deriv_kernel<M, H, NSP, 1>), grid, dim3(256), 0, stream, da); break;
    case 2: hipLaunchKernelGGL((tiled_deriv_kernel<M, H, NSP, 2>), grid, dim3(256), 0, stream, da); break;
    default: return hipErrorInvalidValue;      // (three derivative windows spill: 136 bytes of scratch per lane at V = 3)
    }
    return hipGetLastError();
}

hipError_t epgx_launch_tiled_deriv(hipStream_t stream, const TiledDerivArgs &da, int M, int H, int n_spaces, int n_vars) {
    const TiledArgs &a = da.a;
    if (a.nvox <= 0 || a.tiles <= 0 || a.tiles > 65535 || (a.nvox + 3) / 4 > 0x7fffffff || a.Kbuf % 64 != 0 || !da.drecs)
        return hipErrorInvalidValue;
    if (M != 8 || H != 32) return hipErrorInvalidValue;      // (16 orders per lane: two windows alone are 384 VGPRs)
    switch (n_spaces) {
    case 0: return launch_tiled_deriv_v<8, 32, 0>(stream, da, n_vars);
    case 1: return launch_tiled_deriv_v<8, 32, 1>(stream, da, n_vars);
    case 2: return launch_tiled_deriv_v<8, 32, 2>(stream, da, n_vars);
    default: return launch_tiled_deriv_v<8, 32, 4>(stream, da, n_vars);
    }
}

hipError_t epgx_launch_tiled_shift(hipStream_t stream, const d2 *in, d2 *out, int64_t nvox, int32_t Kbuf, int32_t kcov, int32_t n,
                                   int32_t kmax) {
    if (nvox <= 0 || kcov <= 0 || kcov > Kbuf || n == 0 || (n > 0 ? n : -n) >= Kbuf) return hipErrorInvalidValue;
    const unsigned gy = (unsigned)std::min<int64_t>(nvox, 65535);
    hipLaunchKernelGGL(tiled_shift_kernel, dim3((unsigned)((kcov + 255) / 256), gy), dim3(256), 0, stream, in, out, nvox, Kbuf, kcov, n, kmax);
    return hipGetLastError();
}

hipError_t epgx_launch_tiled_equilibrium(hipStream_t stream, d2 *buf, double *dens, const double *dens_in, int64_t nvox, int32_t Kbuf,
                                         int32_t windows) {
    if (nvox <= 0 || windows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tiled_equilibrium_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, stream, buf, dens, dens_in, nvox, Kbuf,
                       windows);
    return hipGetLastError();
}

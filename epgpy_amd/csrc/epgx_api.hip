// epgx_api.hip -- host side of libepgx.so: the C ABI declared in include/epgx.h.
//
// Every entry point validates its operands against what the kernels and their grids assume
// BEFORE anything is launched (shapes, opcode range, coefficient-table bounds, shift range,
// signal slots), returns a negative status instead of throwing, and records a thread-local
// message for epgx_last_error().  There is no CPU execution path in this library.  (The entry points that read a signal, a
// dictionary or a Jacobian left in HBM -- crlb, match, refine, nnls, gram, project -- are epgx_signal.hip.)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: librccl.so.1 is loaded on first use (rccl_api)
#include <dlfcn.h>
#include <sched.h>
#include <pthread.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <string>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "epgx_ctx.h"
#include "epgx_kernels.hip.h"
#include "epgx_small_kernels.hip.h"
#include "epgx_exchange_kernels.hip.h"
#include "epgx_xrun_kernels.hip.h"
#include "epgx_dxrun_kernels.hip.h"
#include "epgx_deriv_kernels.hip.h"
#include "epgx_launch.h"
#include "epgx_launch_hess.h"
#include "epgx_planner.h"
#include "epgx_plan_check.h"
#include "epgx_run_check.h"
#include "epgx_chain.h"
#include "epgx_dft.h"
#include "epgx_merge.h"
#include "epgx_prune.h"
#include "epgx_launch_grow.h"
#include "epgx_launch_tiled.h"

using namespace epgx;

// ------------------------------------------------------------------------------ errors
// (fail and the thread-local message behind epgx_last_error: epgx_error.h; HIP_TRY: epgx_ctx.h)

// Measurement knobs of the selection (Knobs, epgx_planner.h), read from the environment ONCE per process, here and nowhere else.
namespace {
int env_int(const char *name, int fallback) {
    const char *v = getenv(name);
    return v ? atoi(v) : fallback;
}
const Knobs &knobs() {
    static const Knobs k = {env_int("EPGX_ROWS", 1) != 0,   env_int("EPGX_ROWS_DERIV", 1) != 0, env_int("EPGX_ROWS_DERIV2", 1) != 0,
                            env_int("EPGX_DRUN", 1) != 0,   env_int("EPGX_RUNS", 1) != 0,       env_int("EPGX_GROW", 1) != 0,
                            env_int("EPGX_CONTIG", 1) != 0, env_int("EPGX_SPLIT", 1) != 0,      env_int("EPGX_PREFETCH", 1) != 0,
                            env_int("EPGX_GROW_MIN", 1),    env_int("EPGX_FOLD", 1) != 0,
                            getenv("EPGX_GROW_SHARE") ? atof(getenv("EPGX_GROW_SHARE")) : 0.1, env_int("EPGX_LEAD_FORWARD", 1) != 0,
                            env_int("EPGX_SLAB_VOXELS", 0), env_int("EPGX_SPLIT_GROW", 1) != 0, env_int("EPGX_XRUN", 1) != 0,
                            env_int("EPGX_REACH", 1) != 0,  env_int("EPGX_CGROW", 1),           env_int("EPGX_LANES", 1),
                            env_int("EPGX_LANES_BODY", 1),  env_int("EPGX_LANES_TRAIN", 1),
                            env_int("EPGX_LANES_ODD", 1)};
    return k;
}

}  // namespace

// ------------------------------------------------------------------------------ objects
// (struct epgx_ctx: epgx_ctx.h, with the declarations of dev_alloc, dev_free and set_device for epgx_signal.hip)
static void dev_release_cache_locked(epgx_ctx *ctx) {
    if (ctx->cache.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &b : ctx->cache) (void)hipFree(b.first);
    ctx->cache.clear();
    ctx->cached_bytes = 0;
}

static void dev_release_cache(epgx_ctx *ctx) {
    std::lock_guard<std::mutex> guard(ctx->mem);
    dev_release_cache_locked(ctx);
}

hipError_t epgx::dev_alloc(epgx_ctx *ctx, void **out, size_t bytes) {
    std::lock_guard<std::mutex> guard(ctx->mem);
    bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
    int best = -1;
    for (int i = 0; i < (int)ctx->cache.size(); ++i) {
        const size_t n = ctx->cache[i].second;
        if (n >= bytes && n <= bytes + std::max<size_t>(bytes / 4, (size_t)1 << 20) &&
            (best < 0 || n < ctx->cache[best].second))
            best = i;
    }
    if (best >= 0) {
        *out = ctx->cache[best].first;
        ctx->live[*out] = ctx->cache[best].second;
        ctx->cached_bytes -= ctx->cache[best].second;
        ctx->cache.erase(ctx->cache.begin() + best);
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory) {   // give the cached blocks back and try once more
        (void)hipGetLastError();
        dev_release_cache_locked(ctx);
        e = hipMalloc(out, bytes);
    }
    if (e == hipSuccess) ctx->live[*out] = bytes;
    return e;
}

void epgx::dev_free(epgx_ctx *ctx, void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> guard(ctx->mem);
    auto it = ctx->live.find(p);
    if (it == ctx->live.end()) {   // not ours (should not happen): plain free
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
        return;
    }
    const size_t n = it->second;
    ctx->live.erase(it);
    ctx->cache.emplace_back(p, n);
    ctx->cached_bytes += n;
    // Keep at most half of the HBM (evict the largest block first) and 96 blocks.  Over the count: the OLDEST blocks below 1 GiB
    // go, in one batch down to 64 blocks behind ONE stream synchronisation -- a small block is cheap to allocate again, the
    // block that was just freed (the likeliest to be asked for next) stays, and the hot path pays one synchronisation per 32
    // frees instead of one per free.  Multi-GB blocks are never evicted on the count rule: giving one back to HIP has a
    // lasting price on this platform -- after one hipFree of 16 GB every later copy into page-locked host memory ran at 28.6
    // instead of 54 GB/s for the rest of the process (tools/release_probe.py; round 3's bench showed it: seven short PGSE calls
    // pushed the count past the cap, the 16 GB signal of the MRF leg went, and the end-to-end leg after it fell from 6.9 to
    // 20.7 ms).
    const size_t limit = (size_t)ctx->prop.totalGlobalMem / 2;
    bool synced = false;
    auto evict = [&](size_t victim) {
        if (!synced) (void)hipStreamSynchronize(ctx->stream);
        synced = true;
        (void)hipFree(ctx->cache[victim].first);
        ctx->cached_bytes -= ctx->cache[victim].second;
        ctx->cache.erase(ctx->cache.begin() + (std::ptrdiff_t)victim);
    };
    while (!ctx->cache.empty() && ctx->cached_bytes > limit) {
        size_t victim = 0;
        for (size_t i = 1; i < ctx->cache.size(); ++i)
            if (ctx->cache[i].second > ctx->cache[victim].second) victim = i;
        evict(victim);
    }
    if (ctx->cache.size() > 96) {
        for (size_t i = 0; i < ctx->cache.size() && ctx->cache.size() > 64;) {      // (the vector is in order of freeing: oldest first)
            if (ctx->cache[i].second < ((size_t)1 << 30)) evict(i);
            else ++i;
        }
    }
}

// one operator range [begin, end) packed into fused records for capacity K (epgx_planner.h), resident on the device
enum { DEV_RECS, DEV_DRECS, DEV_DRUNS, DEV_DDRUNS, DEV_BDRUNS, DEV_RUNS, DEV_GROW, DEV_COUNT };
struct PackedRange {
    RangeLists lists;
    void *dev[DEV_COUNT] = {};   // the list of that name with its padding records, or null (upload_range)
    const Rec *recs(int which) const { return (const Rec *)dev[which]; }
};

static void free_range(epgx_ctx *ctx, PackedRange &pr) {
    for (void *&p : pr.dev) {
        dev_free(ctx, p);
        p = nullptr;
    }
}

struct epgx_plan : PlanGeometry {   // ndim, shape, strides, nvox_total, dense_spaces, x_span, x_ncomp (epgx_plan_check.h)
    epgx_ctx *ctx = nullptr;
    PlanHost host;            // the host-only part: the primitive stream and what planning reads of it (epgx_planner.h)
    int32_t deriv_flags = 0;
    std::vector<PackedRange> packed;
    double *d_coef = nullptr;
    int64_t n_coef = 0;
    int32_t n_adc = 0;
    epgx_op *d_ops = nullptr;   // device copy of `ops` (xrun_kernel walks the primitive list), made on first use
    epgx_dop *d_dops = nullptr; // device copy of `dops` (dxrun_kernel), made on first use
    // `cache_lock` guards `packed` and the vidx cache (two host threads running ranges of one plan)
    std::mutex cache_lock;
    // cached table indices for one voxel range
    int32_t *d_vidx = nullptr;
    int64_t vidx_vox0 = -1, vidx_nvox = 0, vidx_cap = 0;
};

struct epgx_state {
    epgx_ctx *ctx = nullptr;
    int64_t nvox = 0;
    int32_t K = 0;
    d2 *data = nullptr;
    double *dens = nullptr;
};

struct epgx_coords {   // per-voxel coordinates next to a state of 64 stored orders (epgx_prune.hip)
    epgx_ctx *ctx = nullptr;
    int64_t nvox = 0;
    int32_t kdim = 0;
    double *k = nullptr;        // [nvox][kdim][64]
    int32_t *nlive = nullptr;   // [nvox]
};

int epgx::set_device(const epgx_ctx *ctx) {
    HIP_TRY(hipSetDevice(ctx->device));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ library
extern "C" int epgx_abi_version(void) { return EPGX_ABI_VERSION; }

extern "C" const char *epgx_last_error(void) { return g_err; }

extern "C" int epgx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int epgx_ctx_create(int device, epgx_ctx **out) {
    if (!out) return fail(EPGX_ERR_INVALID, "epgx_ctx_create: out is NULL");
    *out = nullptr;
    int n = epgx_device_count();
    if (n <= 0)
        return fail(EPGX_ERR_NODEVICE,
                    "epgx_ctx_create: no HIP device visible (libepgx has no CPU fallback)");
    if (device < 0 || device >= n)
        return fail(EPGX_ERR_INVALID, "epgx_ctx_create: device %d out of range [0,%d)", device, n);
    epgx_ctx *ctx = new (std::nothrow) epgx_ctx();
    if (!ctx) return fail(EPGX_ERR_NOMEM, "epgx_ctx_create: host allocation failed");
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&ctx->prop, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e != hipSuccess) {
        delete ctx;
        return fail(EPGX_ERR_HIP, "epgx_ctx_create: %s", hipGetErrorString(e));
    }
    if (ctx->prop.warpSize != 64) {
        int w = ctx->prop.warpSize;
        epgx_ctx_destroy(ctx);
        return fail(EPGX_ERR_NODEVICE, "epgx_ctx_create: device wavefront size %d, need 64 (CDNA)", w);
    }
    ctx->stream = ctx->own;
    ctx->own_stream = true;
    *out = ctx;
    return EPGX_OK;
}

extern "C" int epgx_ctx_destroy(epgx_ctx *ctx) {
    if (!ctx) return EPGX_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->own) (void)hipStreamSynchronize(ctx->own);
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    for (hipEvent_t ev : ctx->slab_events) (void)hipEventDestroy(ev);
    for (auto &st : ctx->stages) {
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.host) (void)hipHostFree(st.host);
    }
    for (auto &b : ctx->host_cache) (void)hipHostFree(b.first);
    dev_release_cache(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->own) (void)hipStreamDestroy(ctx->own);
    delete ctx;
    return EPGX_OK;
}

extern "C" int epgx_ctx_set_stream(epgx_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_ctx_set_stream: ctx is NULL");
    if (int rc = set_device(ctx)) return rc;
    // recycled device blocks rely on stream order: drain the old stream before switching
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
        ctx->own_stream = false;
    } else {
        ctx->stream = ctx->own;
        ctx->own_stream = true;
    }
    return EPGX_OK;
}

extern "C" int epgx_ctx_synchronize(epgx_ctx *ctx) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_ctx_synchronize: ctx is NULL");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return EPGX_OK;
}

extern "C" int epgx_ctx_info(epgx_ctx *ctx, epgx_device_info *out) {
    if (!ctx || !out) return fail(EPGX_ERR_INVALID, "epgx_ctx_info: NULL argument");
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", ctx->prop.name);
    snprintf(out->arch, sizeof(out->arch), "%s", ctx->prop.gcnArchName);
    out->compute_units = ctx->prop.multiProcessorCount;
    out->wavefront_size = ctx->prop.warpSize;
    out->clock_khz = ctx->prop.clockRate;
    out->hbm_bytes = (int64_t)ctx->prop.totalGlobalMem;
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ memory
extern "C" int epgx_malloc(epgx_ctx *ctx, int64_t bytes, void **dptr) {
    if (!ctx || !dptr || bytes < 0) return fail(EPGX_ERR_INVALID, "epgx_malloc: bad argument");
    *dptr = nullptr;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(dev_alloc(ctx, dptr, (size_t)std::max<int64_t>(bytes, 16)));
    return EPGX_OK;
}

extern "C" int epgx_ctx_release_cache(epgx_ctx *ctx) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_ctx_release_cache: ctx is NULL");
    if (int rc = set_device(ctx)) return rc;
    dev_release_cache(ctx);
    return EPGX_OK;
}

extern "C" int epgx_free(epgx_ctx *ctx, void *dptr) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_free: ctx is NULL");
    if (!dptr) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    dev_free(ctx, dptr);
    return EPGX_OK;
}

extern "C" int epgx_memset(epgx_ctx *ctx, void *dptr, int value, int64_t bytes) {
    if (!ctx || (!dptr && bytes) || bytes < 0) return fail(EPGX_ERR_INVALID, "epgx_memset: bad argument");
    if (int rc = set_device(ctx)) return rc;
    if (bytes) HIP_TRY(hipMemsetAsync(dptr, value, (size_t)bytes, ctx->stream));
    return EPGX_OK;
}

extern "C" int epgx_memcpy_h2d(epgx_ctx *ctx, void *dptr, const void *host, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes && (!dptr || !host)))
        return fail(EPGX_ERR_INVALID, "epgx_memcpy_h2d: bad argument");
    if (int rc = set_device(ctx)) return rc;
    if (bytes) {
        HIP_TRY(hipMemcpyAsync(dptr, host, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return EPGX_OK;
}

extern "C" int epgx_memcpy_d2h(epgx_ctx *ctx, void *host, const void *dptr, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes && (!dptr || !host)))
        return fail(EPGX_ERR_INVALID, "epgx_memcpy_d2h: bad argument");
    if (int rc = set_device(ctx)) return rc;
    if (bytes) {
        HIP_TRY(hipMemcpyAsync(host, dptr, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return EPGX_OK;
}

extern "C" int epgx_memcpy_d2d(epgx_ctx *ctx, void *dst, const void *src, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes && (!dst || !src)))
        return fail(EPGX_ERR_INVALID, "epgx_memcpy_d2d: bad argument");
    if (int rc = set_device(ctx)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ page-locked host memory
extern "C" int epgx_host_alloc(epgx_ctx *ctx, int64_t bytes, int32_t cached_only, void **hptr) {
    if (!ctx || !hptr || bytes < 0) return fail(EPGX_ERR_INVALID, "epgx_host_alloc: bad argument");
    *hptr = nullptr;
    if (int rc = set_device(ctx)) return rc;
    size_t n = std::max<size_t>(((size_t)bytes + 4095) & ~(size_t)4095, 4096);
    {
        std::lock_guard<std::mutex> guard(ctx->mem);
        int best = -1;
        for (int i = 0; i < (int)ctx->host_cache.size(); ++i) {
            const size_t have = ctx->host_cache[i].second;
            if (have >= n && have <= n + n / 4 && (best < 0 || have < ctx->host_cache[best].second)) best = i;
        }
        if (best >= 0) {
            *hptr = ctx->host_cache[best].first;
            ctx->host_live[*hptr] = ctx->host_cache[best].second;
            ctx->host_cached_bytes -= ctx->host_cache[best].second;
            ctx->host_cache.erase(ctx->host_cache.begin() + best);
            return EPGX_OK;
        }
    }
    if (cached_only) return EPGX_OK;   // nothing to recycle: the caller takes its pageable path
    HIP_TRY(hipHostMalloc(hptr, n, hipHostMallocDefault));
    std::lock_guard<std::mutex> guard(ctx->mem);
    ctx->host_live[*hptr] = n;
    return EPGX_OK;
}

extern "C" int epgx_host_free(epgx_ctx *ctx, void *hptr) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_host_free: ctx is NULL");
    if (!hptr) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    std::vector<void *> victims;
    {
        std::lock_guard<std::mutex> guard(ctx->mem);
        auto it = ctx->host_live.find(hptr);
        if (it == ctx->host_live.end()) return fail(EPGX_ERR_INVALID, "epgx_host_free: not a block of this context");
        ctx->host_cache.emplace_back(hptr, it->second);
        ctx->host_cached_bytes += it->second;
        ctx->host_live.erase(it);
        // keep at most EPGX_PINNED_CACHE_MB (4 GiB) / 16 blocks of pinned memory around (oldest first out)
        static const size_t budget = (size_t)(getenv("EPGX_PINNED_CACHE_MB") ? std::max(0, atoi(getenv("EPGX_PINNED_CACHE_MB"))) : 4096) << 20;
        while (!ctx->host_cache.empty() && (ctx->host_cached_bytes > budget || ctx->host_cache.size() > 16)) {
            victims.push_back(ctx->host_cache.front().first);
            ctx->host_cached_bytes -= ctx->host_cache.front().second;
            ctx->host_cache.erase(ctx->host_cache.begin());
        }
    }
    for (void *v : victims) (void)hipHostFree(v);
    return EPGX_OK;
}

extern "C" int epgx_host_register(epgx_ctx *ctx, void *hptr, int64_t bytes) {
    if (!ctx || !hptr || bytes <= 0) return fail(EPGX_ERR_INVALID, "epgx_host_register: bad argument");
    if (int rc = set_device(ctx)) return rc;
    const hipError_t e = hipHostRegister(hptr, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP, "epgx_host_register: %s", hipGetErrorString(e));
    }
    return EPGX_OK;
}

extern "C" int epgx_host_unregister(epgx_ctx *ctx, void *hptr) {
    if (!ctx || !hptr) return fail(EPGX_ERR_INVALID, "epgx_host_unregister: NULL argument");
    if (int rc = set_device(ctx)) return rc;
    // (copies into the block may still be in flight on the context's streams)
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    const hipError_t e = hipHostUnregister(hptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(EPGX_ERR_HIP, "epgx_host_unregister: %s", hipGetErrorString(e));
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ timing
extern "C" int epgx_timer_start(epgx_ctx *ctx) {
    if (!ctx) return fail(EPGX_ERR_INVALID, "epgx_timer_start: ctx is NULL");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return EPGX_OK;
}

extern "C" int epgx_timer_stop(epgx_ctx *ctx, float *elapsed_ms) {
    if (!ctx || !elapsed_ms) return fail(EPGX_ERR_INVALID, "epgx_timer_stop: NULL argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ plan
static int plan_create(epgx_ctx *ctx, const epgx_plan_desc *d, const epgx_plan_ext *ext, epgx_plan **out);

extern "C" int epgx_plan_create(epgx_ctx *ctx, const epgx_plan_desc *d, epgx_plan **out) { return plan_create(ctx, d, nullptr, out); }

extern "C" int epgx_plan_create_ext(epgx_ctx *ctx, const epgx_plan_desc *d, const epgx_plan_ext *ext, epgx_plan **out) {
    if (out) *out = nullptr;
    if (ext && ext->struct_size != sizeof(epgx_plan_ext))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create_ext: struct_size = %u, but epgx_plan_ext has %zu bytes in this library (ABI %d)",
                    ext->struct_size, sizeof(epgx_plan_ext), EPGX_ABI_VERSION);
    if (ext && (ext->n_chain < 0 || (ext->n_chain && !ext->chain)))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create_ext: n_chain = %d without a list", ext->n_chain);
    return plan_create(ctx, d, ext, out);
}

// The device half of plan creation.  Each step queues its work on ctx->stream and returns the first HIP error; plan_create
// synchronises once behind the last.

// the pool with its padding and the room of the log tables behind it; the host part uploaded, its rounding residues cleared
static hipError_t upload_pool(epgx_ctx *ctx, epgx_plan *pl, const epgx_plan_desc *d, const std::vector<Snap> &snaps) {
    // pool padded so that the fixed-width scalar loads of the last entry stay in bounds
    const int64_t n_pool = pl->host.n_pool, n_log = pl->host.n_log;
    hipError_t e = dev_alloc(ctx, (void **)&pl->d_coef, sizeof(double) * (size_t)(n_pool + 32 + n_log + (n_log ? 32 : 0)));
    if (e == hipSuccess && n_log)
        e = hipMemsetAsync(pl->d_coef + n_pool + 32 + n_log, 0, sizeof(double) * 32, ctx->stream);
    if (e == hipSuccess)   // (the generated part is written entry by entry: only the padding needs zeros)
        e = hipMemsetAsync(pl->d_coef + n_pool, 0, sizeof(double) * 32, ctx->stream);
    static const double identity_relaxation[4] = {1.0, 0.0, 1.0, 0.0};   // e, Im e, e2, r: what a missing E_a / E_b of a folded record reads
    if (e == hipSuccess)
        e = hipMemcpyAsync(pl->d_coef + n_pool, identity_relaxation, sizeof(identity_relaxation), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && d->n_coef)
        e = hipMemcpyAsync(pl->d_coef, d->coef, sizeof(double) * (size_t)d->n_coef,
                           hipMemcpyHostToDevice, ctx->stream);
    for (size_t i = 0; i < snaps.size() && e == hipSuccess; ++i) {   // clear the rounding residues (analyse_plan)
        const Snap &sn = snaps[i];
        hipLaunchKernelGGL(snap_kernel, dim3((unsigned)((sn.entries + 255) / 256)), dim3(256), 0, ctx->stream,
                           pl->d_coef + sn.off, sn.entries, sn.nc, sn.mask);
        e = hipGetLastError();
    }
    return e;
}

// tables assembled from per-axis columns (epgx_assemble): one launch for all recipes
static hipError_t generate_assembled(epgx_ctx *ctx, epgx_plan *pl, const epgx_plan_desc *d) {
    if (d->n_assemble <= 0) return hipSuccess;
    std::vector<AsmArgs> recipes((size_t)d->n_assemble);
    int64_t most = 1;
    for (int i = 0; i < d->n_assemble; ++i) {
        const epgx_assemble &as = d->assemble[i];
        AsmArgs &aa = recipes[(size_t)i];
        memset(&aa, 0, sizeof(aa));
        aa.dst_off = as.dst_off;
        aa.n_entries = pl->entries(as.dst_space);
        aa.ndim = pl->ndim;
        aa.ncoef = as.ncoef;
        aa.n_src = as.n_src;
        pl->fill(aa.shape, aa.dst_str, as.dst_space);
        for (int k = 0; k < as.n_src; ++k) {
            aa.src_off[k] = as.src[k].off;
            aa.src_ncol[k] = as.src[k].ncol;
            for (int dd = 0; dd < pl->ndim; ++dd) aa.src_str[k][dd] = as.src[k].strides[dd];
        }
        memcpy(aa.col_src, as.col_src, sizeof(aa.col_src));
        memcpy(aa.col_idx, as.col_idx, sizeof(aa.col_idx));
        most = std::max(most, aa.n_entries);
    }
    AsmArgs *d_recipes = nullptr;
    hipError_t e = dev_alloc(ctx, (void **)&d_recipes, sizeof(AsmArgs) * recipes.size());
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_recipes, recipes.data(), sizeof(AsmArgs) * recipes.size(), hipMemcpyHostToDevice, ctx->stream);
    const unsigned bx = (unsigned)std::min<int64_t>((most + 255) / 256, 4096);
    for (int first = 0; first < d->n_assemble && e == hipSuccess; first += 32768) {
        const unsigned by = (unsigned)std::min(d->n_assemble - first, 32768);
        hipLaunchKernelGGL(assemble_kernel, dim3(bx, by), dim3(256), 0, ctx->stream, pl->d_coef, (const AsmArgs *)(d_recipes + first));
        e = hipGetLastError();
    }
    // (`recipes` is a local: the copy must have left the host before it goes; the plan's final synchronise is in plan_create,
    // so wait here only for the upload)
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, d_recipes);
    return e;
}

// collapsed tables (epgx_chain): the steps of all chains in one upload, one launch per chain
static hipError_t generate_chains(epgx_ctx *ctx, epgx_plan *pl, const epgx_plan_ext *ext) {
    const int n_chain = ext ? ext->n_chain : 0;
    if (n_chain <= 0) return hipSuccess;
    std::vector<epgx_chain_step> steps;
    for (int i = 0; i < n_chain; ++i) steps.insert(steps.end(), ext->chain[i].steps, ext->chain[i].steps + ext->chain[i].n_steps);
    epgx_chain_step *d_steps = nullptr;
    hipError_t e = dev_alloc(ctx, (void **)&d_steps, sizeof(epgx_chain_step) * steps.size());
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_steps, steps.data(), sizeof(epgx_chain_step) * steps.size(), hipMemcpyHostToDevice, ctx->stream);
    size_t at = 0;
    for (int i = 0; i < n_chain && e == hipSuccess; ++i) {
        const epgx_chain &ch = ext->chain[i];
        ChainArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.pool = pl->d_coef;
        ca.steps = d_steps + at;
        ca.dst_off = ch.dst_off;
        ca.n_entries = pl->entries(ch.dst_space);
        ca.n_steps = ch.n_steps;
        ca.ndim = pl->ndim;
        pl->fill(ca.shape, ca.dst_str, ch.dst_space);
        for (int sp = 0; sp < pl->host.n_spaces; ++sp)
            for (int dd = 0; dd < pl->ndim; ++dd) ca.sp_str[sp][dd] = pl->strides[sp][dd];
        e = epgx_launch_chain(ctx->stream, ca);
        at += (size_t)ch.n_steps;
    }
    // (`steps` is a local: its upload must have left the host before it goes; the kernels have read d_steps by then too)
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, d_steps);
    return e;
}

// fused tables (epgx_fuse), then their partials (epgx_fuse_partial): one launch per recipe, in list order
static hipError_t generate_fused(epgx_ctx *ctx, epgx_plan *pl, const epgx_plan_desc *d) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < d->n_fuse && e == hipSuccess; ++i) {
        const epgx_fuse &fu = d->fuse[i];
        FuseArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.pool = pl->d_coef;
        fa.dst_off = fu.dst_off;
        fa.src_off = fu.src_off;
        fa.e_off = fu.e_off;
        fa.n_entries = pl->entries(fu.dst_space);
        fa.ndim = pl->ndim;
        fa.src_ncoef = fu.src_ncoef;
        fa.after = fu.after;
        pl->fill(fa.shape, fa.dst_str, fu.dst_space);
        pl->fill(fa.shape, fa.src_str, fu.src_space);
        pl->fill(fa.shape, fa.e_str, fu.e_space);
        hipLaunchKernelGGL(fuse_kernel, dim3((unsigned)((fa.n_entries + 255) / 256)), dim3(256), 0, ctx->stream, fa);
        e = hipGetLastError();
    }
    for (int i = 0; i < d->n_fuse_partial && e == hipSuccess; ++i) {
        const epgx_fuse_partial &fp = d->fuse_partial[i];
        FusePartialArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.pool = pl->d_coef;
        fa.dst_off = fp.dst_off;
        fa.src_off = fp.src_off;
        fa.dsrc_off = fp.dsrc_off < 0 ? -1 : fp.dsrc_off;
        fa.e_off = fp.e_off;
        fa.de_off = fp.de_off < 0 ? -1 : fp.de_off;
        fa.n_entries = pl->entries(fp.dst_space);
        fa.ndim = pl->ndim;
        fa.src_ncoef = fp.src_ncoef;
        fa.dsrc_ncoef = fp.dsrc_ncoef;
        fa.after = fp.after;
        pl->fill(fa.shape, fa.dst_str, fp.dst_space);
        pl->fill(fa.shape, fa.src_str, fp.src_space);
        pl->fill(fa.shape, fa.dsrc_str, fp.dsrc_off < 0 ? -1 : fp.dsrc_space);
        pl->fill(fa.shape, fa.e_str, fp.e_space);
        pl->fill(fa.shape, fa.de_str, fp.de_off < 0 ? -1 : fp.de_space);
        hipLaunchKernelGGL(fuse_partial_kernel, dim3((unsigned)((fa.n_entries + 255) / 256)), dim3(256), 0, ctx->stream, fa);
        e = hipGetLastError();
    }
    return e;
}

// tables of logarithmic partials (logtab_kernel) and the copy of their flags into `logflags`, which is complete once the stream
// has been synchronised; *d_logflags is the caller's to free
static hipError_t generate_log_tables(epgx_ctx *ctx, epgx_plan *pl, const std::vector<LogJob> &log_jobs, uint32_t **d_logflags,
                                      std::vector<uint32_t> &logflags) {
    if (log_jobs.empty()) return hipSuccess;
    hipError_t e = dev_alloc(ctx, (void **)d_logflags, sizeof(uint32_t) * log_jobs.size());
    if (e == hipSuccess) e = hipMemsetAsync(*d_logflags, 0, sizeof(uint32_t) * log_jobs.size(), ctx->stream);
    for (size_t j = 0; j < log_jobs.size() && e == hipSuccess; ++j) {
        LogTabArgs la;
        memset(&la, 0, sizeof(la));
        la.pool = pl->d_coef;
        la.e_off = log_jobs[j].e_off;
        la.de_off = log_jobs[j].de_off;
        la.dst_off = pl->host.logtabs[j].off;
        la.n_entries = log_jobs[j].entries;
        la.flags = *d_logflags;
        la.slot = (int32_t)j;
        hipLaunchKernelGGL(logtab_kernel, dim3((unsigned)((la.n_entries + 255) / 256)), dim3(256), 0, ctx->stream, la);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(logflags.data(), *d_logflags, sizeof(uint32_t) * log_jobs.size(), hipMemcpyDeviceToHost, ctx->stream);
    return e;
}

// what logtab_kernel found out about every log table, and the two EPGX_TRACE lines on them
static void read_log_flags(epgx_plan *pl, const std::vector<LogJob> &log_jobs, const std::vector<uint32_t> &logflags, bool trace) {
    for (size_t j = 0; j < log_jobs.size(); ++j) {
        pl->host.logtabs[j].any = logflags[j] & 3u;
        if (logflags[j] & 4u) pl->host.logtabs[j].off = -1;   // not of the logarithmic form: records that need it do not fold
        if (trace && (j < 8 || (logflags[j] & 4u)))
            fprintf(stderr, "[epgx] plan_create log table %zu: value table at %lld, partial at %lld, %lld entries: wT %s, wL %s%s\n", j,
                    (long long)log_jobs[j].e_off, (long long)log_jobs[j].de_off, (long long)log_jobs[j].entries,
                    (logflags[j] & 1u) ? "nonzero" : "zero", (logflags[j] & 2u) ? "nonzero" : "zero",
                    (logflags[j] & 4u) ? " -- NOT of the logarithmic form" : "");
    }
    if (trace && !pl->host.t0_logd.empty()) {
        int routed = 0, generated = 0;
        for (size_t i = 0; i < pl->host.ops.size(); ++i)
            for (int v = 0; v < pl->host.n_vars; ++v)
                if (pl->host.ops[i].opcode == EPGX_OP_T0 && pl->host.dops[i].coef_off[v] >= 0) (pl->host.t0_logd[i * EPGX_MAX_VARS + v] ? routed : generated)++;
        fprintf(stderr, "[epgx] plan_create fused-echo partials: %d relaxation-only (logarithmic route), %d with a rotation partial\n", routed, generated);
    }
}

static int plan_create(epgx_ctx *ctx, const epgx_plan_desc *d, const epgx_plan_ext *ext, epgx_plan **out) {
    if (!ctx || !d || !out) return fail(EPGX_ERR_INVALID, "epgx_plan_create: NULL argument");
    *out = nullptr;
    // (the first member: readable whatever the caller's idea of the struct is)
    if (d->struct_size != sizeof(epgx_plan_desc))
        return fail(EPGX_ERR_INVALID, "epgx_plan_create: struct_size = %u, but epgx_plan_desc has %zu bytes in this library (ABI %d): "
                    "set struct_size = sizeof(epgx_plan_desc) and rebuild the caller against include/epgx.h", d->struct_size,
                    sizeof(epgx_plan_desc), EPGX_ABI_VERSION);
    const Lap lap;
    PlanAnalysis an;   // everything decided on host data alone, every refusal among it (epgx_plan_check.h)
    if (int rc = analyse_plan(d, ext, knobs(), &an)) return rc;
    if (int rc = set_device(ctx)) return rc;
    lap("host done");
    // (epgx_plan_destroy copes with a half-built plan: an early return gives back whatever the plan holds by then)
    std::unique_ptr<epgx_plan, decltype(&epgx_plan_destroy)> pl(new (std::nothrow) epgx_plan(), epgx_plan_destroy);
    if (!pl) return fail(EPGX_ERR_NOMEM, "epgx_plan_create: host allocation failed");
    pl->ctx = ctx;
    static_cast<PlanGeometry &>(*pl) = an.geo;
    pl->host = std::move(an.host);
    pl->deriv_flags = d->deriv_flags;
    pl->n_adc = d->n_adc;
    pl->n_coef = d->n_coef;
    uint32_t *d_logflags = nullptr;
    std::vector<uint32_t> logflags(an.log_jobs.size(), 0u);
    hipError_t e = upload_pool(ctx, pl.get(), d, an.snaps);
    if (e == hipSuccess) e = generate_assembled(ctx, pl.get(), d);
    if (e == hipSuccess) e = generate_chains(ctx, pl.get(), ext);
    if (e == hipSuccess) e = generate_fused(ctx, pl.get(), d);
    if (e == hipSuccess) e = generate_log_tables(ctx, pl.get(), an.log_jobs, &d_logflags, logflags);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, d_logflags);
    read_log_flags(pl.get(), an.log_jobs, logflags, lap.on);
    lap("uploaded");
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP, "epgx_plan_create: %s",
                    hipGetErrorString(e));
    *out = pl.release();
    return EPGX_OK;
}

extern "C" int epgx_plan_destroy(epgx_plan *pl) {
    if (!pl) return EPGX_OK;
    (void)hipSetDevice(pl->ctx->device);
    for (auto &pr : pl->packed) free_range(pl->ctx, pr);
    dev_free(pl->ctx, pl->d_coef);
    dev_free(pl->ctx, pl->d_vidx);
    dev_free(pl->ctx, pl->d_ops);
    dev_free(pl->ctx, pl->d_dops);
    delete pl;
    return EPGX_OK;
}

// make sure the plan's cached table-index array covers [vox0, vox0+nvox)
static int ensure_vidx(epgx_plan *pl, int64_t vox0, int64_t nvox) {
    if (pl->host.n_spaces == 0) return EPGX_OK;
    if (pl->d_vidx && pl->vidx_vox0 == vox0 && pl->vidx_nvox == nvox) return EPGX_OK;
    epgx_ctx *ctx = pl->ctx;
    if (!pl->d_vidx || pl->vidx_cap < nvox) {
        dev_free(ctx, pl->d_vidx);
        pl->d_vidx = nullptr;
        // the 4-space kernel variant reads four rows: always allocate (and zero) that many
        const int rows = pl->host.n_spaces > 2 ? 4 : pl->host.n_spaces;
        HIP_TRY(dev_alloc(ctx, (void **)&pl->d_vidx, sizeof(int32_t) * (size_t)nvox * rows));
        HIP_TRY(hipMemsetAsync(pl->d_vidx, 0, sizeof(int32_t) * (size_t)nvox * rows, ctx->stream));
        pl->vidx_cap = nvox;
    }
    IndexArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.vidx = pl->d_vidx;
    ia.ld = nvox;
    ia.vox0 = vox0;
    ia.nvox = nvox;
    ia.n_spaces = pl->host.n_spaces;
    ia.ndim = pl->ndim;
    for (int i = 0; i < EPGX_MAX_DIMS; ++i) ia.shape[i] = pl->shape[i];
    memcpy(ia.strides, pl->strides, sizeof(ia.strides));
    const unsigned blocks = (unsigned)((nvox + 255) / 256);
    hipLaunchKernelGGL(index_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ia);
    HIP_TRY(hipGetLastError());
    pl->vidx_vox0 = vox0;
    pl->vidx_nvox = nvox;
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ signal reduction
extern "C" int epgx_signal_reduce(epgx_ctx *ctx, const void *signal, int64_t signal_ld, int32_t row0, int32_t row_step,
                                  int32_t n_rows, int32_t ndim, const int64_t *grid_shape, const uint8_t *reduce_axis,
                                  const void *weights, const int64_t *weight_strides, void *out, int64_t vox0, int64_t nvox_held) {
    if (!ctx || !signal || !grid_shape || !reduce_axis || !out || (weights && !weight_strides))
        return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: NULL argument");
    if (ndim < 1 || ndim > EPGX_MAX_DIMS) return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: ndim %d not in [1,%d]", ndim, EPGX_MAX_DIMS);
    if (n_rows < 0 || row0 < 0 || row_step < 1) return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: bad row range");
    ReduceArgs a;
    memset(&a, 0, sizeof(a));
    int64_t nvox = 1, acc[EPGX_MAX_DIMS];
    for (int d = ndim - 1; d >= 0; --d) {
        if (grid_shape[d] < 1) return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: grid_shape[%d] < 1", d);
        acc[d] = nvox;
        nvox *= grid_shape[d];
    }
    if (vox0 < 0 || nvox_held < 0 || vox0 + nvox_held > nvox)
        return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: slab [%lld,%lld) outside the grid (%lld voxels)", (long long)vox0,
                    (long long)(vox0 + nvox_held), (long long)nvox);
    if (nvox_held > signal_ld) return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: slab of %lld voxels exceeds signal_ld=%lld", (long long)nvox_held, (long long)signal_ld);
    a.n_out = a.n_red_total = 1;
    for (int d = 0; d < ndim; ++d) {
        const int64_t ws = weights ? weight_strides[d] : 0;
        if (ws < 0) return fail(EPGX_ERR_INVALID, "epgx_signal_reduce: negative weight stride");
        if (reduce_axis[d]) {
            a.red_size[a.n_red] = grid_shape[d];
            a.red_stride[a.n_red] = acc[d];
            a.red_wstride[a.n_red++] = ws;
            a.n_red_total *= grid_shape[d];
        } else {
            a.keep_size[a.n_keep] = grid_shape[d];
            a.keep_stride[a.n_keep] = acc[d];
            a.keep_wstride[a.n_keep++] = ws;
            a.n_out *= grid_shape[d];
        }
    }
    if (n_rows == 0) return EPGX_OK;
    if (n_rows > 65535) return fail(EPGX_ERR_UNSUPPORTED, "epgx_signal_reduce: more than 65535 rows per call");
    if (int rc = set_device(ctx)) return rc;
    a.signal = (const d2 *)signal;
    a.ld = signal_ld;
    a.row0 = row0;
    a.row_step = row_step;
    a.n_rows = n_rows;
    a.weights = (const d2 *)weights;
    a.out = (d2 *)out;
    a.vox0 = vox0;
    a.nheld = nvox_held;
    if (reduce_axis[ndim - 1])
        hipLaunchKernelGGL(reduce_wave_kernel, dim3((unsigned)((a.n_out + 3) / 4), (unsigned)n_rows), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(reduce_thread_kernel, dim3((unsigned)((a.n_out + 255) / 256), (unsigned)n_rows), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ records complex128 -> complex64
static int launch_narrow(epgx_ctx *ctx, const void *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols) {
    if (!rows || !cols) return EPGX_OK;
    const unsigned bx = (unsigned)std::min<int64_t>((cols + 1023) / 1024, 4096), by = (unsigned)std::min<int64_t>(rows, 65535);
    hipLaunchKernelGGL(narrow_kernel, dim3(bx, by), dim3(256), 0, ctx->stream, (const d2 *)src, src_ld, (float2 *)dst, dst_ld, rows, cols);
    HIP_TRY(hipGetLastError());
    return EPGX_OK;
}

extern "C" int epgx_signal_narrow(epgx_ctx *ctx, const void *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols) {
    if (!ctx || rows < 0 || cols < 0 || src_ld < cols || dst_ld < cols || (rows && cols && (!src || !dst)))
        return fail(EPGX_ERR_INVALID, "epgx_signal_narrow: bad argument");
    if (int rc = set_device(ctx)) return rc;
    return launch_narrow(ctx, src, src_ld, dst, dst_ld, rows, cols);
}

// ------------------------------------------------------------------------------ state
extern "C" int epgx_state_create(epgx_ctx *ctx, int64_t nvox, int32_t K, epgx_state **out) {
    if (!ctx || !out) return fail(EPGX_ERR_INVALID, "epgx_state_create: NULL argument");
    *out = nullptr;
    if (nvox < 1) return fail(EPGX_ERR_INVALID, "epgx_state_create: nvox < 1");
    if (!supported_K(K))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_create: K=%d, supported capacities are 64,128,256,512,1024", K);
    if (int rc = set_device(ctx)) return rc;
    epgx_state *st = new (std::nothrow) epgx_state();
    if (!st) return fail(EPGX_ERR_NOMEM, "epgx_state_create: host allocation failed");
    st->ctx = ctx;
    st->nvox = nvox;
    st->K = K;
    hipError_t e = dev_alloc(ctx, (void **)&st->data, sizeof(d2) * (size_t)nvox * 3 * K);
    if (e == hipSuccess) e = dev_alloc(ctx, (void **)&st->dens, sizeof(double) * (size_t)nvox);
    if (e != hipSuccess) {
        epgx_state_destroy(st);
        return fail(e == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP, "epgx_state_create: %s",
                    hipGetErrorString(e));
    }
    const int64_t total = nvox * 3 * K;
    hipLaunchKernelGGL(state_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       st->data, (int)K, st->dens, nvox);
    e = hipGetLastError();
    if (e != hipSuccess) {
        epgx_state_destroy(st);
        return fail(EPGX_ERR_HIP, "epgx_state_create: %s", hipGetErrorString(e));
    }
    *out = st;
    return EPGX_OK;
}

extern "C" int epgx_state_destroy(epgx_state *st) {
    if (!st) return EPGX_OK;
    (void)hipSetDevice(st->ctx->device);
    dev_free(st->ctx, st->data);
    dev_free(st->ctx, st->dens);
    delete st;
    return EPGX_OK;
}

extern "C" int epgx_state_upload(epgx_state *st, const double *half, const double *density) {
    if (!st || !half) return fail(EPGX_ERR_INVALID, "epgx_state_upload: NULL argument");
    if (int rc = epgx_memcpy_h2d(st->ctx, st->data, half, (int64_t)sizeof(d2) * st->nvox * 3 * st->K)) return rc;
    if (density) return epgx_memcpy_h2d(st->ctx, st->dens, density, (int64_t)sizeof(double) * st->nvox);
    return EPGX_OK;
}

extern "C" int epgx_state_download(const epgx_state *st, double *half, double *density) {
    if (!st || !half) return fail(EPGX_ERR_INVALID, "epgx_state_download: NULL argument");
    if (int rc = epgx_memcpy_d2h(st->ctx, half, st->data, (int64_t)sizeof(d2) * st->nvox * 3 * st->K)) return rc;
    if (density) return epgx_memcpy_d2h(st->ctx, density, st->dens, (int64_t)sizeof(double) * st->nvox);
    return EPGX_OK;
}

static int launch_copy(epgx_state *dst, const epgx_state *src, const int32_t *d_map) {
    epgx_ctx *ctx = dst->ctx;
    if (int rc = set_device(ctx)) return rc;
    const int64_t total = dst->nvox * 3 * dst->K;
    hipLaunchKernelGGL(state_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream,
                       dst->data, (int)dst->K, (const d2 *)src->data, (int)src->K, d_map, dst->dens,
                       (const double *)src->dens, dst->nvox);
    HIP_TRY(hipGetLastError());
    return EPGX_OK;
}

extern "C" int epgx_state_copy(epgx_state *dst, const epgx_state *src) {
    if (!dst || !src) return fail(EPGX_ERR_INVALID, "epgx_state_copy: NULL argument");
    if (dst == src) return EPGX_OK;
    if (dst->ctx != src->ctx) return fail(EPGX_ERR_INVALID, "epgx_state_copy: states belong to different contexts");
    if (dst->nvox != src->nvox)
        return fail(EPGX_ERR_INVALID, "epgx_state_copy: nvox mismatch (%lld vs %lld)", (long long)dst->nvox,
                    (long long)src->nvox);
    return launch_copy(dst, src, nullptr);
}

extern "C" int epgx_state_broadcast(epgx_state *dst, const epgx_state *src, const int32_t *src_index) {
    if (!dst || !src || !src_index) return fail(EPGX_ERR_INVALID, "epgx_state_broadcast: NULL argument");
    if (dst == src) return fail(EPGX_ERR_INVALID, "epgx_state_broadcast: dst and src must differ");
    if (dst->ctx != src->ctx) return fail(EPGX_ERR_INVALID, "epgx_state_broadcast: different contexts");
    for (int64_t j = 0; j < dst->nvox; ++j)
        if (src_index[j] < 0 || src_index[j] >= src->nvox)
            return fail(EPGX_ERR_INVALID, "epgx_state_broadcast: src_index[%lld]=%d out of range", (long long)j,
                        src_index[j]);
    epgx_ctx *ctx = dst->ctx;
    if (int rc = set_device(ctx)) return rc;
    int32_t *d_map = nullptr;
    HIP_TRY(dev_alloc(ctx, (void **)&d_map, sizeof(int32_t) * (size_t)dst->nvox));
    hipError_t e = hipMemcpyAsync(d_map, src_index, sizeof(int32_t) * (size_t)dst->nvox, hipMemcpyHostToDevice,
                                  ctx->stream);
    int rc = EPGX_OK;
    if (e != hipSuccess) rc = fail(EPGX_ERR_HIP, "epgx_state_broadcast: %s", hipGetErrorString(e));
    if (!rc) rc = launch_copy(dst, src, d_map);
    (void)hipStreamSynchronize(ctx->stream);   // `src_index` is the caller's
    dev_free(ctx, d_map);
    return rc;
}

extern "C" int epgx_state_axpy(epgx_state *dst, const epgx_state *src, double alpha, int32_t zero_density) {
    if (!dst || !src) return fail(EPGX_ERR_INVALID, "epgx_state_axpy: NULL argument");
    if (dst->ctx != src->ctx) return fail(EPGX_ERR_INVALID, "epgx_state_axpy: states of different contexts");
    if (dst->nvox != src->nvox || dst->K != src->K)
        return fail(EPGX_ERR_INVALID, "epgx_state_axpy: shapes differ (%lld x %d vs %lld x %d)", (long long)dst->nvox, dst->K,
                    (long long)src->nvox, src->K);
    epgx_ctx *ctx = dst->ctx;
    if (int rc = set_device(ctx)) return rc;
    const int64_t n = dst->nvox * 3 * dst->K;
    hipLaunchKernelGGL(state_axpy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dst->data,
                       (const d2 *)src->data, alpha, n);
    HIP_TRY(hipGetLastError());
    if (zero_density) HIP_TRY(hipMemsetAsync(dst->dens, 0, sizeof(double) * (size_t)dst->nvox, ctx->stream));
    return EPGX_OK;
}

extern "C" int epgx_state_info(const epgx_state *st, int64_t *nvox, int32_t *K, void **data, void **density) {
    if (!st) return fail(EPGX_ERR_INVALID, "epgx_state_info: NULL argument");
    if (nvox) *nvox = st->nvox;
    if (K) *K = st->K;
    if (data) *data = st->data;
    if (density) *density = st->dens;
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ spatial read-out (epgx_dft.hip)
extern "C" int epgx_state_dft(epgx_ctx *ctx, const epgx_state *st, int64_t vox0, int64_t nvox, int32_t nrow, const double *k,
                              const double *w, int32_t d, const double *pos, int64_t npos, double phase_re, double phase_im,
                              void *out) {
    if (!ctx || !st || !k || !w || !pos || !out) return fail(EPGX_ERR_INVALID, "epgx_state_dft: NULL argument");
    if (st->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_state_dft: the state belongs to another context");
    if (nrow < 1 || nrow > st->K)
        return fail(EPGX_ERR_INVALID, "epgx_state_dft: nrow = %d not in [1, K = %d]", nrow, st->K);
    if (d < 1 || d > 3) return fail(EPGX_ERR_INVALID, "epgx_state_dft: d = %d position columns, expected 1 .. 3", d);
    if (vox0 < 0 || nvox < 1 || vox0 + nvox > st->nvox)
        return fail(EPGX_ERR_INVALID, "epgx_state_dft: voxels [%lld, %lld) outside the state (%lld voxels)", (long long)vox0,
                    (long long)(vox0 + nvox), (long long)st->nvox);
    if (npos < 1) return fail(EPGX_ERR_INVALID, "epgx_state_dft: npos = %lld < 1", (long long)npos);
    const int64_t tiles_v = (nvox + DFT_TV - 1) / DFT_TV, tiles_p = (npos + DFT_TP - 1) / DFT_TP;
    const size_t table_bytes = sizeof(double) * 4 * (size_t)dft_table_voxels(nvox) * (size_t)nrow;
    if (tiles_v > 65535 || tiles_p > 0x7fffffff || table_bytes > ((size_t)8 << 30))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_dft: %lld voxels x %d orders x %lld positions in one call: hand over a smaller "
                    "voxel range (the coefficient table is limited to 8 GiB, the launch to %d voxels)", (long long)nvox, nrow,
                    (long long)npos, 65535 * DFT_TV);
    if (int rc = set_device(ctx)) return rc;
    // k and pos padded to three columns (zero columns add nothing to the phase), w: one upload behind the table
    std::vector<double> host((size_t)4 * nrow + (size_t)3 * npos, 0.0);
    double *hk = host.data(), *hw = hk + (size_t)3 * nrow, *hp = hw + nrow;
    for (int32_t j = 0; j < nrow; ++j) {
        for (int c = 0; c < d; ++c) hk[3 * j + c] = k[(size_t)j * d + c];
        hw[j] = w[j];
    }
    for (int64_t p = 0; p < npos; ++p)
        for (int c = 0; c < d; ++c) hp[3 * p + c] = pos[p * d + c];
    char *block = nullptr;
    HIP_TRY(dev_alloc(ctx, (void **)&block, table_bytes + sizeof(double) * host.size()));
    double *d_small = (double *)(block + table_bytes);
    hipError_t e = hipMemcpyAsync(d_small, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (`host` is pageable and dies with this call)
    if (e == hipSuccess) {
        DftArgs a;
        a.state = st->data;
        a.K = st->K;
        a.nrow = nrow;
        a.vox0 = vox0;
        a.nvox = nvox;
        a.k = d_small;
        a.w = d_small + (size_t)3 * nrow;
        a.pos = d_small + (size_t)4 * nrow;
        a.npos = npos;
        a.table = (double *)block;
        a.phase_re = phase_re;
        a.phase_im = phase_im;
        a.out = (d2 *)out;
        e = epgx_launch_dft(ctx->stream, a);
    }
    dev_free(ctx, block);   // (recycled in stream order, behind the kernels that read it)
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_state_dft: %s", hipGetErrorString(e));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ float-wavenumber shift (epgx_merge.hip)
extern "C" int epgx_state_row_stats(epgx_ctx *ctx, const epgx_state *st, int32_t nrow, double *sums, double *maxabs) {
    if (!ctx || !st || !sums || !maxabs) return fail(EPGX_ERR_INVALID, "epgx_state_row_stats: NULL argument");
    if (st->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_state_row_stats: the state belongs to another context");
    if (nrow < 1 || nrow > st->K) return fail(EPGX_ERR_INVALID, "epgx_state_row_stats: nrow = %d not in [1, K = %d]", nrow, st->K);
    if (st->nvox < 1 || (st->K & 63)) return fail(EPGX_ERR_INVALID, "epgx_state_row_stats: a state of %lld voxels x %d orders", (long long)st->nvox, st->K);
    if (int rc = set_device(ctx)) return rc;
    RowStatsArgs a;
    a.state = st->data;
    a.K = st->K;
    a.nvox = st->nvox;
    a.slab = stats_slab(st->nvox);
    a.nblocks = (int32_t)stats_blocks(st->nvox);
    const size_t n_out = (size_t)4 * st->K;
    double *block = nullptr;
    HIP_TRY(dev_alloc(ctx, (void **)&block, sizeof(double) * n_out * ((size_t)a.nblocks + 1)));
    a.partial = block + n_out;
    a.out = block;
    std::vector<double> host(n_out);
    hipError_t e = epgx_launch_row_stats(ctx->stream, a);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), a.out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, block);
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_state_row_stats: %s", hipGetErrorString(e));
    for (int q = 0; q < 3; ++q) memcpy(sums + (size_t)q * nrow, host.data() + (size_t)q * st->K, sizeof(double) * (size_t)nrow);
    memcpy(maxabs, host.data() + (size_t)3 * st->K, sizeof(double) * (size_t)nrow);
    return EPGX_OK;
}

extern "C" int epgx_state_merge(epgx_ctx *ctx, epgx_state *dst, const epgx_state *src, int32_t nrow_dst, const int32_t *offsets,
                                const int32_t *sources) {
    if (!ctx || !dst || !src || !offsets || !sources) return fail(EPGX_ERR_INVALID, "epgx_state_merge: NULL argument");
    if (nrow_dst > MERGE_MAX_ROWS)
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_merge: %d stored orders in the destination, at most %d are supported", nrow_dst,
                    MERGE_MAX_ROWS);
    if (dst->ctx != ctx || src->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_state_merge: a state belongs to another context");
    if (dst == src || dst->data == src->data) return fail(EPGX_ERR_INVALID, "epgx_state_merge: dst and src must differ");
    if (dst->nvox != src->nvox)
        return fail(EPGX_ERR_INVALID, "epgx_state_merge: nvox mismatch (%lld vs %lld)", (long long)dst->nvox, (long long)src->nvox);
    if (nrow_dst < 1 || nrow_dst > dst->K)
        return fail(EPGX_ERR_INVALID, "epgx_state_merge: nrow_dst = %d not in [1, K = %d] of the destination", nrow_dst, dst->K);
    const size_t n_off = (size_t)3 * ((size_t)nrow_dst + 1);
    if (offsets[0] != 0) return fail(EPGX_ERR_INVALID, "epgx_state_merge: offsets[0][0] = %d, expected 0", offsets[0]);
    for (size_t i = 1; i < n_off; ++i) {
        const bool seam = i % ((size_t)nrow_dst + 1) == 0;      // (the first entry of a component repeats the last of the one before)
        if (seam ? offsets[i] != offsets[i - 1] : offsets[i] < offsets[i - 1])
            return fail(EPGX_ERR_INVALID, "epgx_state_merge: offsets[%zu] = %d after %d: the table is not in CSR form", i, offsets[i],
                        offsets[i - 1]);
    }
    const int32_t n_src = offsets[n_off - 1];
    for (int32_t s = 0; s < n_src; ++s) {
        const int32_t ent = sources[s], order = ent & MERGE_ORDER_MASK, comp = (ent >> MERGE_COMP_SHIFT) & 0x3fff;
        if (ent < 0 || comp > 2 || order >= src->K)
            return fail(EPGX_ERR_INVALID, "epgx_state_merge: sources[%d] = 0x%x: component %d, order %d (the source has %d orders)", s,
                        ent, comp, order, src->K);
    }
    if (int rc = set_device(ctx)) return rc;
    std::vector<int32_t> host(n_off + (size_t)std::max(n_src, 1));
    memcpy(host.data(), offsets, sizeof(int32_t) * n_off);
    if (n_src) memcpy(host.data() + n_off, sources, sizeof(int32_t) * (size_t)n_src);
    int32_t *d_tab = nullptr;
    HIP_TRY(dev_alloc(ctx, (void **)&d_tab, sizeof(int32_t) * host.size()));
    hipError_t e = hipMemcpyAsync(d_tab, host.data(), sizeof(int32_t) * host.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (`host` is pageable and dies with this call)
    if (e == hipSuccess) {
        MergeArgs a;
        a.dst = dst->data;
        a.src = src->data;
        a.Kd = dst->K;
        a.Ks = src->K;
        a.nrow = nrow_dst;
        a.nvox = dst->nvox;
        a.offsets = d_tab;
        a.sources = d_tab + n_off;
        e = epgx_launch_merge(ctx->stream, a);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dst->dens, src->dens, sizeof(double) * (size_t)dst->nvox, hipMemcpyDeviceToDevice, ctx->stream);
    }
    dev_free(ctx, d_tab);   // (recycled in stream order, behind the kernel that reads it)
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_state_merge: %s", hipGetErrorString(e));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ per-voxel float shift (epgx_prune.hip)
extern "C" int epgx_coords_create(epgx_ctx *ctx, int64_t nvox, int32_t kdim, epgx_coords **out) {
    if (!ctx || !out) return fail(EPGX_ERR_INVALID, "epgx_coords_create: NULL argument");
    *out = nullptr;
    if (nvox < 1) return fail(EPGX_ERR_INVALID, "epgx_coords_create: nvox < 1");
    if (kdim < 1 || kdim > 4) return fail(EPGX_ERR_INVALID, "epgx_coords_create: kdim = %d, expected 1 .. 4", kdim);
    if (int rc = set_device(ctx)) return rc;
    epgx_coords *c = new (std::nothrow) epgx_coords();
    if (!c) return fail(EPGX_ERR_NOMEM, "epgx_coords_create: host allocation failed");
    c->ctx = ctx;
    c->nvox = nvox;
    c->kdim = kdim;
    const size_t kbytes = sizeof(double) * (size_t)nvox * (size_t)kdim * PRUNE_K;
    hipError_t e = dev_alloc(ctx, (void **)&c->k, kbytes);
    if (e == hipSuccess) e = dev_alloc(ctx, (void **)&c->nlive, sizeof(int32_t) * (size_t)nvox);
    if (e == hipSuccess) e = hipMemsetAsync(c->k, 0, kbytes, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->nlive, 0, sizeof(int32_t) * (size_t)nvox, ctx->stream);
    if (e != hipSuccess) {
        epgx_coords_destroy(c);
        return fail(e == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP, "epgx_coords_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return EPGX_OK;
}

extern "C" int epgx_coords_destroy(epgx_coords *c) {
    if (!c) return EPGX_OK;
    (void)hipSetDevice(c->ctx->device);
    dev_free(c->ctx, c->k);
    dev_free(c->ctx, c->nlive);
    delete c;
    return EPGX_OK;
}

extern "C" int epgx_coords_info(const epgx_coords *c, int64_t *nvox, int32_t *kdim) {
    if (!c) return fail(EPGX_ERR_INVALID, "epgx_coords_info: NULL argument");
    if (nvox) *nvox = c->nvox;
    if (kdim) *kdim = c->kdim;
    return EPGX_OK;
}

static int coords_widen(epgx_coords *dst, const double *d_k, const int32_t *d_n, int32_t ks, int broadcast) {
    CoordsWidenArgs a;
    a.dst = dst->k;
    a.src = d_k;
    a.ndst = dst->nlive;
    a.nsrc_rows = d_n;
    a.nvox = dst->nvox;
    a.kd = dst->kdim;
    a.ks = ks;
    a.broadcast = broadcast;
    HIP_TRY(epgx_launch_coords_widen(dst->ctx->stream, a));
    return EPGX_OK;
}

extern "C" int epgx_coords_upload(epgx_coords *c, const double *k, const int32_t *nlive, int64_t nsrc) {
    if (!c || !k || !nlive) return fail(EPGX_ERR_INVALID, "epgx_coords_upload: NULL argument");
    if (nsrc != 1 && nsrc != c->nvox)
        return fail(EPGX_ERR_INVALID, "epgx_coords_upload: %lld coordinate sets for %lld voxels (one for all, or one each)", (long long)nsrc,
                    (long long)c->nvox);
    for (int64_t v = 0; v < nsrc; ++v)
        if (nlive[v] < 1 || nlive[v] > PRUNE_K)
            return fail(EPGX_ERR_INVALID, "epgx_coords_upload: nlive[%lld] = %d not in [1, %d]", (long long)v, nlive[v], PRUNE_K);
    epgx_ctx *ctx = c->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t kbytes = sizeof(double) * (size_t)nsrc * (size_t)c->kdim * PRUNE_K, nbytes = sizeof(int32_t) * (size_t)nsrc;
    if (nsrc == c->nvox) {
        if (int rc = epgx_memcpy_h2d(ctx, c->k, k, (int64_t)kbytes)) return rc;
        return epgx_memcpy_h2d(ctx, c->nlive, nlive, (int64_t)nbytes);
    }
    char *block = nullptr;      // one set for all voxels: uploaded once, repeated on the device
    HIP_TRY(dev_alloc(ctx, (void **)&block, kbytes + nbytes));
    int rc = epgx_memcpy_h2d(ctx, block, k, (int64_t)kbytes);
    if (!rc) rc = epgx_memcpy_h2d(ctx, block + kbytes, nlive, (int64_t)nbytes);
    if (!rc) rc = coords_widen(c, (const double *)block, (const int32_t *)(block + kbytes), c->kdim, 1);
    dev_free(ctx, block);   // (recycled in stream order, behind the kernel that reads it)
    return rc;
}

extern "C" int epgx_coords_download(const epgx_coords *c, double *k, int32_t *nlive) {
    if (!c || !k || !nlive) return fail(EPGX_ERR_INVALID, "epgx_coords_download: NULL argument");
    if (int rc = epgx_memcpy_d2h(c->ctx, k, c->k, (int64_t)(sizeof(double) * (size_t)c->nvox * (size_t)c->kdim * PRUNE_K))) return rc;
    return epgx_memcpy_d2h(c->ctx, nlive, c->nlive, (int64_t)(sizeof(int32_t) * (size_t)c->nvox));
}

extern "C" int epgx_coords_widen(epgx_coords *dst, const epgx_coords *src) {
    if (!dst || !src) return fail(EPGX_ERR_INVALID, "epgx_coords_widen: NULL argument");
    if (dst == src || dst->k == src->k) return fail(EPGX_ERR_INVALID, "epgx_coords_widen: dst and src must differ");
    if (dst->ctx != src->ctx) return fail(EPGX_ERR_INVALID, "epgx_coords_widen: different contexts");
    if (dst->nvox != src->nvox || dst->kdim < src->kdim)
        return fail(EPGX_ERR_INVALID, "epgx_coords_widen: %lld voxels x %d columns into %lld x %d", (long long)src->nvox, src->kdim,
                    (long long)dst->nvox, dst->kdim);
    if (int rc = set_device(dst->ctx)) return rc;
    return coords_widen(dst, src->k, src->nlive, src->kdim, 0);
}

extern "C" int epgx_state_prune_shift(epgx_ctx *ctx, epgx_state *dst, epgx_coords *cdst, const epgx_state *src, const epgx_coords *csrc,
                                      const double *table, int64_t ntable, int32_t ndim, const int64_t *shape, const int64_t *sstride,
                                      const double *ktvalue, const double *grid, int32_t nmax, int32_t prune, double tol,
                                      int32_t *max_live) {
    if (!ctx || !dst || !cdst || !src || !csrc || !table || !shape || !sstride || !ktvalue || !grid || !max_live)
        return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: NULL argument");
    if (dst->ctx != ctx || src->ctx != ctx || cdst->ctx != ctx || csrc->ctx != ctx)
        return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: a state or a coordinate buffer belongs to another context");
    if (dst == src || dst->data == src->data || cdst == csrc || cdst->k == csrc->k)
        return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: dst and src must differ");
    const int64_t nvox = src->nvox;
    if (dst->nvox != nvox || cdst->nvox != nvox || csrc->nvox != nvox)
        return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: nvox mismatch (%lld, %lld, %lld, %lld)", (long long)dst->nvox,
                    (long long)cdst->nvox, (long long)src->nvox, (long long)csrc->nvox);
    const int32_t kdim = csrc->kdim;
    if (kdim < 1 || kdim > 4 || cdst->kdim != kdim)
        return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: kdim = %d / %d, expected equal and 1 .. 4", csrc->kdim, cdst->kdim);
    if (dst->K != PRUNE_K || src->K != PRUNE_K)
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_prune_shift: states of %d / %d stored orders, the per-voxel shift covers %d", src->K,
                    dst->K, PRUNE_K);
    if (ndim < 1 || ndim > PRUNE_MAX_DIMS) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: ndim = %d not in [1, %d]", ndim, PRUNE_MAX_DIMS);
    if (ntable < 1) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: ntable < 1");
    int64_t total = 1, last = 0;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] < 1 || sstride[d] < 0 || total > nvox)
            return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: grid axis %d: extent %lld, table stride %lld", d, (long long)shape[d],
                        (long long)sstride[d]);
        total *= shape[d];
        last += (shape[d] - 1) * sstride[d];
    }
    if (total != nvox) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: a grid of %lld voxels for states of %lld", (long long)total, (long long)nvox);
    if (last >= ntable) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: the grid reaches entry %lld of a table of %lld", (long long)last, (long long)ntable);
    for (int c = 0; c < kdim; ++c) {
        if (!(grid[c] > 0.0) || !std::isfinite(grid[c])) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: grid[%d] = %g, expected positive", c, grid[c]);
        if (ktvalue[c] == 0.0 || !std::isfinite(ktvalue[c])) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: ktvalue[%d] = %g", c, ktvalue[c]);
    }
    for (int64_t i = 0; i < ntable * kdim; ++i)
        if (!std::isfinite(table[i])) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: table[%lld] is not finite", (long long)i);
    if (!(tol >= 0.0)) return fail(EPGX_ERR_INVALID, "epgx_state_prune_shift: tol = %g", tol);
    if (int rc = set_device(ctx)) return rc;

    PruneArgs a;
    a.dst = dst->data;
    a.src = src->data;
    a.kdst = cdst->k;
    a.ksrc = csrc->k;
    a.ndst = cdst->nlive;
    a.nsrc = csrc->nlive;
    a.nvox = nvox;
    a.kdim = kdim;
    a.ndim = ndim;
    int64_t stride = nvox;
    for (int d = 0; d < PRUNE_MAX_DIMS; ++d) {
        a.shape[d] = d < ndim ? shape[d] : 1;
        stride /= a.shape[d];
        a.vstride[d] = d < ndim ? stride : 1;
        a.sstride[d] = d < ndim ? sstride[d] : 0;
    }
    for (int c = 0; c < 4; ++c) {
        a.scale_in[c] = a.scale_out[c] = c < kdim ? ktvalue[c] : 1.0;
        a.grid[c] = c < kdim ? grid[c] : 1.0;
    }
    a.nmax = nmax < 0 ? -1 : nmax;
    a.prune = prune ? 1 : 0;
    a.tol = tol;
    a.nblocks = (int32_t)(nvox < PRUNE_MAX_BLOCKS ? nvox : PRUNE_MAX_BLOCKS);
    const size_t tbytes = (sizeof(double) * (size_t)ntable * (size_t)kdim + 15) & ~(size_t)15;
    char *block = nullptr;
    HIP_TRY(dev_alloc(ctx, (void **)&block, tbytes + sizeof(int32_t) * (2 * (size_t)a.nblocks + 2)));
    a.table = (const double *)block;
    a.result = (int32_t *)(block + tbytes);
    a.partial = a.result + 2;
    int32_t result[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(block, table, sizeof(double) * (size_t)ntable * (size_t)kdim, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (`table` is the caller's)
    if (e == hipSuccess) e = epgx_launch_prune_shift(ctx->stream, a);
    if (e == hipSuccess) e = hipMemcpyAsync(dst->dens, src->dens, sizeof(double) * (size_t)nvox, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(result, a.result, sizeof(result), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    dev_free(ctx, block);
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_state_prune_shift: %s", hipGetErrorString(e));
    if (result[1])
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_prune_shift: a voxel keeps more than %d stored orders after trim and prune", PRUNE_K);
    *max_live = result[0];
    return EPGX_OK;
}

extern "C" int epgx_state_prune_read(epgx_ctx *ctx, const epgx_state *st, const epgx_coords *c, double tvalue, void *out) {
    if (!ctx || !st || !c || !out) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: NULL argument");
    if (st->ctx != ctx || c->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: the state or the coordinates belong to another context");
    if (st->nvox != c->nvox) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: nvox mismatch (%lld vs %lld)", (long long)st->nvox, (long long)c->nvox);
    if (c->kdim != 4) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: kdim = %d, the read-out weighs a time coordinate (kdim 4)", c->kdim);
    if (st->K != PRUNE_K) return fail(EPGX_ERR_UNSUPPORTED, "epgx_state_prune_read: a state of %d stored orders, expected %d", st->K, PRUNE_K);
    if (!std::isfinite(tvalue)) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: tvalue = %g", tvalue);
    if (((uintptr_t)out & 15) != 0) return fail(EPGX_ERR_INVALID, "epgx_state_prune_read: out is not aligned to 16 bytes");
    if (int rc = set_device(ctx)) return rc;
    PruneReadArgs a;
    a.state = st->data;
    a.k = c->k;
    a.nlive = c->nlive;
    a.nvox = st->nvox;
    a.tscale = tvalue;
    a.out = (d2 *)out;
    HIP_TRY(epgx_launch_prune_read(ctx->stream, a));
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ run
// the lists of one range on the device: build_range (epgx_planner.cpp) on a cache miss, uploaded once, kept with the plan
// every list of `pr.lists` that holds something, with its padding records (all zero) behind it: the kernels fetch up to three
// records past the end (rows_kernel may run the first as a no-op), rows_deriv_kernel as many DRecs; two past the folded lists
static hipError_t upload_range(epgx_ctx *ctx, PackedRange &pr) {
    const RangeLists &l = pr.lists;
    const struct { const void *host; size_t elem, count, pad; } table[DEV_COUNT] = {
        {l.recs.data(), sizeof(Rec), l.recs.size(), 3},      {l.drecs.data(), sizeof(DRec), l.drecs.size(), 3},
        {l.druns.data(), sizeof(Rec), l.druns.size(), 3},    {l.ddruns.data(), sizeof(DRec), l.ddruns.size(), 3},
        {l.bdruns.data(), sizeof(DRecB), l.bdruns.size(), 3}, {l.runs.data(), sizeof(Rec), l.runs.size(), 2},
        {l.grow.data(), sizeof(Rec), l.grow.size(), 2}};
    std::vector<char> staged[DEV_COUNT];
    hipError_t e = hipSuccess;
    for (int i = 0; i < DEV_COUNT && e == hipSuccess; ++i) {
        if (!table[i].count) continue;
        staged[i].assign((table[i].count + table[i].pad) * table[i].elem, 0);
        memcpy(staged[i].data(), table[i].host, table[i].count * table[i].elem);
        e = dev_alloc(ctx, &pr.dev[i], staged[i].size());
        if (e == hipSuccess) e = hipMemcpyAsync(pr.dev[i], staged[i].data(), staged[i].size(), hipMemcpyHostToDevice, ctx->stream);
    }
    // `staged` is local: nothing may still be reading it when this returns
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? es : e;
}

static int get_packed(epgx_plan *pl, int begin, int end, int K, const PackedRange **out) {
    for (const auto &pr : pl->packed)
        if (pr.lists.begin == begin && pr.lists.end == end && pr.lists.K == K) {
            *out = &pr;
            return EPGX_OK;
        }
    PackedRange pr;
    pr.lists = build_range(pl->host, begin, end, K, knobs());
    if (pr.lists.n_rec) {
        const hipError_t e = upload_range(pl->ctx, pr);
        if (e != hipSuccess) {
            free_range(pl->ctx, pr);
            return fail(EPGX_ERR_HIP, "epgx_run: uploading records failed: %s", hipGetErrorString(e));
        }
    }
    if (pl->packed.size() >= 4096) {  // bound the cache (streams of thousands of distinct ranges)
        for (auto &old : pl->packed) free_range(pl->ctx, old);
        pl->packed.clear();
    }
    pl->packed.push_back(std::move(pr));
    *out = &pl->packed.back();
    return EPGX_OK;
}

// one call of epgx_run / epgx_kernel_for: the request as run analysis reads it (epgx_run_check.h) and the handles behind it
struct RunCall {
    RunRequest rq;
    const epgx_state *in;
    epgx_state *out;
    void *signal;
    d2 *signal_col() const { return signal ? (d2 *)signal + rq.signal_col0 : nullptr; }
};

static StateFacts facts_of(const epgx_state *st, const epgx_ctx *ctx) {
    StateFacts f;
    if (st) f.present = true, f.K = st->K, f.nvox = st->nvox, f.foreign = st->ctx != ctx;
    return f;
}

static RunCall run_call(const epgx_ctx *ctx, int32_t op_begin, int32_t op_end, int64_t vox0, int64_t nvox, const epgx_state *in, epgx_state *out,
                        int32_t K, void *signal, int64_t signal_ld, int64_t signal_col0, bool naming) {
    RunCall call = {{}, in, out, signal};
    call.rq.op_begin = op_begin, call.rq.op_end = op_end, call.rq.vox0 = vox0, call.rq.nvox = nvox, call.rq.K = K;
    call.rq.in = facts_of(in, ctx), call.rq.out = facts_of(out, ctx);
    call.rq.has_signal = signal != nullptr, call.rq.signal_ld = signal_ld, call.rq.signal_col0 = signal_col0, call.rq.naming = naming;
    return call;
}

// what epgx_run and epgx_kernel_for do first, both through here: the handles, then everything that needs no record list
static int analyse_call(const epgx_ctx *ctx, const epgx_plan *pl, const RunCall &call, RunDecision *d) {
    if (!ctx || !pl) return fail(EPGX_ERR_INVALID, "epgx_run: NULL argument");
    if (pl->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_run: plan belongs to another context");
    return analyse_run(pl->host, *pl, call.rq, knobs(), d);
}

// xrun_kernel launchers (epgx_xrun.hip, one translation unit per number of compartments): M = K / 64
hipError_t epgx_launch_xrun_nc2(hipStream_t stream, const epgx::XRunArgs &a, int64_t ngroups, int M);
hipError_t epgx_launch_xrun_nc3(hipStream_t stream, const epgx::XRunArgs &a, int64_t ngroups, int M);
hipError_t epgx_launch_xrun_nc4(hipStream_t stream, const epgx::XRunArgs &a, int64_t ngroups, int M);
// dxrun_kernel launchers (epgx_dxrun.hip, likewise): V = derivative states
hipError_t epgx_launch_dxrun_nc2(hipStream_t stream, const epgx::DXRunArgs &a, int64_t ngroups, int M, int V);
hipError_t epgx_launch_dxrun_nc3(hipStream_t stream, const epgx::DXRunArgs &a, int64_t ngroups, int M, int V);
hipError_t epgx_launch_dxrun_nc4(hipStream_t stream, const epgx::DXRunArgs &a, int64_t ngroups, int M, int V);

// one EPGX_OP_X over the groups of voxels [vox0, vox0 + st->nvox) of the grid, state in place
static int launch_exchange(epgx_ctx *ctx, const epgx_plan *pl, const epgx_op &op, int64_t vox0, epgx_state *st) {
    XArgs a;
    memset(&a, 0, sizeof(a));
    a.state = st->data;
    a.dens = st->dens;
    a.tab = pl->d_coef + op.coef_off;
    a.ngroups = st->nvox / op.ia;
    a.stride = op.ib;
    a.vox0 = vox0;
    int log2K = 0;
    while ((1 << log2K) < st->K) ++log2K;
    a.log2K = log2K;
    a.ndim = pl->ndim;
    a.space = op.space;
    for (int d = 0; d < EPGX_MAX_DIMS; ++d) {
        a.shape[d] = pl->shape[d];
        a.strides[d] = op.space >= 0 ? pl->strides[op.space][d] : 0;
    }
    const int64_t lanes = a.ngroups << log2K;
    if ((lanes + 255) / 256 > 0x7fffffff) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: exchange over too many voxels in one launch");
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    switch (op.ia) {
    case 2: hipLaunchKernelGGL(exchange_kernel<2>, grid, block, 0, ctx->stream, a); break;
    case 3: hipLaunchKernelGGL(exchange_kernel<3>, grid, block, 0, ctx->stream, a); break;
    case 4: hipLaunchKernelGGL(exchange_kernel<4>, grid, block, 0, ctx->stream, a); break;
    case 5: hipLaunchKernelGGL(exchange_kernel<5>, grid, block, 0, ctx->stream, a); break;
    case 6: hipLaunchKernelGGL(exchange_kernel<6>, grid, block, 0, ctx->stream, a); break;
    case 7: hipLaunchKernelGGL(exchange_kernel<7>, grid, block, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL(exchange_kernel<8>, grid, block, 0, ctx->stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return EPGX_OK;
}

// the device copy of `ops` (and, for dxrun_kernel, of `dops`), made on first use
static int ensure_dev_ops(epgx_ctx *ctx, epgx_plan *pl, bool with_dops) {
    std::lock_guard<std::mutex> plan_guard(pl->cache_lock);
    if (!pl->d_ops) {
        HIP_TRY(dev_alloc(ctx, (void **)&pl->d_ops, sizeof(epgx_op) * pl->host.ops.size()));
        HIP_TRY(hipMemcpyAsync(pl->d_ops, pl->host.ops.data(), sizeof(epgx_op) * pl->host.ops.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    if (with_dops && !pl->d_dops) {
        HIP_TRY(dev_alloc(ctx, (void **)&pl->d_dops, sizeof(epgx_dop) * pl->host.dops.size()));
        HIP_TRY(hipMemcpyAsync(pl->d_dops, pl->host.dops.data(), sizeof(epgx_dop) * pl->host.dops.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    return EPGX_OK;
}

static void fill_xrun(XRunArgs &a, const epgx_plan *pl, const RunCall &call, int NC) {
    const epgx_state *in = call.in, *out = call.out;
    a.ops = pl->d_ops;
    a.op_begin = call.rq.op_begin;
    a.op_end = call.rq.op_end;
    a.coef = pl->d_coef;
    a.in = in ? in->data : nullptr;
    a.dens_in = in ? in->dens : nullptr;
    a.out = out ? out->data : nullptr;
    a.dens_out = out ? out->dens : nullptr;
    a.signal = call.signal_col();
    a.signal_ld = call.rq.signal_ld;
    a.vox0 = call.rq.vox0;
    a.stride = pl->x_span / NC;
    a.ndim = pl->ndim;
    a.n_spaces = pl->host.n_spaces;
    memcpy(a.shape, pl->shape, sizeof(a.shape));
    memcpy(a.strides, pl->strides, sizeof(a.strides));
}

// ROUTE_XRUN / ROUTE_DXRUN: ONE launch of xrun_kernel<NC, M, HAS_IN> or -- a plan with derivative states, from equilibrium --
// dxrun_kernel<NC, M, V>, the compartment groups (and derivative states) in registers
static int run_exchange_fused(epgx_ctx *ctx, epgx_plan *pl, const RunCall &call, const RunDecision &d) {
    const bool deriv = d.route == ROUTE_DXRUN;
    const int NC = d.NC, M = d.M, V = d.V;
    if (tracing())
        fprintf(stderr, "[epgx] run: %s -- compartment groups %sin registers\n", d.name, deriv ? "and derivative states " : "");
    if (int rc = ensure_dev_ops(ctx, pl, deriv)) return rc;
    DXRunArgs a;
    memset(&a, 0, sizeof(a));
    fill_xrun(a.x, pl, call, NC);
    a.dops = pl->d_dops;
    a.through_plain = (pl->deriv_flags & EPGX_DERIV_THROUGH_PLAIN_OPS) ? 1 : 0;
    const int64_t ngroups = call.rq.nvox / NC;
    if (ngroups > 0x7fffffff) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: more than 2^31 compartment groups in one launch");
    hipError_t e = hipErrorInvalidValue;
    if (deriv) switch (NC) {
        case 2: e = epgx_launch_dxrun_nc2(ctx->stream, a, ngroups, M, V); break;
        case 3: e = epgx_launch_dxrun_nc3(ctx->stream, a, ngroups, M, V); break;
        default: e = epgx_launch_dxrun_nc4(ctx->stream, a, ngroups, M, V); break;
        }
    else switch (NC) {
        case 2: e = epgx_launch_xrun_nc2(ctx->stream, a.x, ngroups, M); break;
        case 3: e = epgx_launch_xrun_nc3(ctx->stream, a.x, ngroups, M); break;
        default: e = epgx_launch_xrun_nc4(ctx->stream, a.x, ngroups, M); break;
        }
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_run: %s launch failed: %s", deriv ? "dxrun_kernel" : "xrun_kernel", hipGetErrorString(e));
    return EPGX_OK;
}

static int run_records(epgx_ctx *ctx, epgx_plan *pl, const RunCall &call, int K);

// ROUTE_XSPLIT: the records between two X run as pieces with the state in HBM (`out`, or a temporary state when out is NULL),
// each X on exchange_kernel in between.  (A piece is a part of a range run analysis has accepted: it goes to its records.)
static int run_exchange_split(epgx_ctx *ctx, epgx_plan *pl, const RunCall &call, int K) {
    const int32_t op_begin = call.rq.op_begin, op_end = call.rq.op_end;
    const int64_t vox0 = call.rq.vox0, nvox = call.rq.nvox;
    const epgx_state *in = call.in;
    epgx_state *out = call.out;
    if (tracing()) fprintf(stderr, "[epgx] run: split<exchange_kernel> -- records between exchanges on the per-timestep kernels\n");
    epgx_state *tmp = nullptr;
    epgx_state *work = out;
    if (!work) {
        if (int rc = epgx_state_create(ctx, nvox, K, &tmp)) return rc;
        work = tmp;
    }
    int rc = EPGX_OK;
    const epgx_state *src = in;   // the state the next piece starts from (NULL: equilibrium)
    int begin = op_begin;
    for (int i = op_begin; i <= op_end && !rc; ++i) {
        if (i < op_end && pl->host.ops[i].opcode != EPGX_OP_X) continue;
        if (i > begin) {
            RunCall piece = call;
            piece.rq.op_begin = begin, piece.rq.op_end = i;
            piece.in = src, piece.out = work;
            rc = run_records(ctx, pl, piece, K);
            src = work;
        }
        if (rc || i == op_end) break;
        if (src != work) {   // the exchange acts in place: bring the start state into `work`
            if (src) rc = epgx_state_copy(work, src);
            else {
                const int64_t total = nvox * 3 * K;
                hipLaunchKernelGGL(state_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, work->data, (int)K,
                                   work->dens, nvox);
                if (hipGetLastError() != hipSuccess) rc = fail(EPGX_ERR_HIP, "epgx_run: state init failed");
            }
            src = work;
        }
        if (!rc) rc = launch_exchange(ctx, pl, pl->host.ops[i], vox0, work);
        begin = i + 1;
    }
    if (!rc && out && src != out) rc = epgx_state_copy(out, src);   // (a range of X-free NOPs only: cannot happen, kept for safety)
    epgx_state_destroy(tmp);
    return rc;
}

// The kernel instantiations live in separate translation units (epgx_inst.hip compiled once per
// M, epgx_deriv.hip ...) so that they build in parallel; see epgx_launch.h.

// the records route of a derivative plan: DerivArgs and the launch of the family `c` names
static hipError_t launch_deriv(epgx_ctx *ctx, const epgx_plan *pl, const RunCall &call, int K, const PackedRange *pr, const Choice &c) {
    const RangeLists &rl = pr->lists;
    const epgx_state *in = call.in;
    hipError_t e = hipSuccess;
    DerivArgs da;
    memset(&da, 0, sizeof(da));
    da.nvox = call.rq.nvox;
    da.in = in ? in->data : nullptr;
    da.dens_in = in ? in->dens : nullptr;
    da.recs = pr->recs(DEV_RECS);
    da.drecs = (const DRec *)pr->dev[DEV_DRECS];
    da.coef = pl->d_coef;
    da.signal = call.signal_col();
    da.signal_ld = call.rq.signal_ld;
    da.t.vidx = pl->d_vidx;
    da.t.vidx_ld = pl->vidx_nvox;
    da.t.vox0 = call.rq.vox0;
    da.t.n_rec = rl.n_rec;
    da.t.dense_spaces = pl->dense_spaces;
    da.t.use_lds = c.lds_mode;
    da.through_plain = (pl->deriv_flags & EPGX_DERIV_THROUGH_PLAIN_OPS) ? 1 : 0;
    da.contig = c.contig ? 1 : 0;
    if (c.family == FAM_DRUN && knobs().grow) {   // (0, 0: four orders per lane throughout; EPGX_GROW=0, measurements)
        da.grow1 = rl.dgrow1;
        da.grow2 = rl.dgrow2;
    }
    if (c.family == FAM_PACKED_DFOLD || c.family == FAM_DRUN) {   // the records with run headers (and E_b's logarithmic partials)
        da.recs = pr->recs(DEV_DRUNS);
        da.drecs = (const DRec *)pr->dev[DEV_DDRUNS];
        da.drecs_b = (const DRecB *)pr->dev[DEV_BDRUNS];
        da.t.n_rec = rl.n_druns;
        // (these kernels exist for 1 and 4 index spaces: a space the plan does not have counts as dense -- no index row is read for it)
        da.t.dense_spaces |= 0xfu & ~((1u << pl->host.n_spaces) - 1u);
        if (tracing())
            fprintf(stderr, "[epgx] run: %d records with headers (%d unfolded); %d runs (%d of one repeated record) hold %d records; [0, %d) "
                            "with one order per lane, [%d, %d) with two\n",
                    rl.n_druns, rl.n_rec, rl.drun_headers, rl.drun_ident, rl.drun_inside, da.grow1, da.grow1, da.grow2);
    }
    switch (c.family) {
    case FAM_HESS: e = epgx_launch_hess(ctx->stream, da, K, pl->host.n_spaces, pl->host.n_vars == 2); break;
    case FAM_PACKED_DFOLD: e = epgx_launch_packed_dfold(ctx->stream, da, K, pl->host.n_vars); break;
    case FAM_DRUN:
        if (c.split3) {
            // three derivative states of folded runs: the last variable alone (rows shifted by two), then the first two over it
            DerivArgs last = da;
            last.signal = da.signal ? da.signal + 2 * da.signal_ld : nullptr;
            e = epgx_launch_drun(ctx->stream, last, K, pl->host.n_spaces, 1, rl.drun_code | (int)DRUN_LAST);
            if (e == hipSuccess) e = epgx_launch_drun(ctx->stream, da, K, pl->host.n_spaces, 2, rl.drun_code);
        } else
            e = epgx_launch_drun(ctx->stream, da, K, pl->host.n_spaces, pl->host.n_vars, rl.drun_code);
        break;
    case FAM_ROWS_DERIV:
        if (pl->host.n_vars == 2) {
            switch (pl->host.n_spaces) {
            case 0: e = epgx_launch_rows_deriv_v2_nsp0(ctx->stream, da, K); break;
            case 1: e = epgx_launch_rows_deriv_v2_nsp1(ctx->stream, da, K); break;
            case 2: e = epgx_launch_rows_deriv_v2_nsp2(ctx->stream, da, K); break;
            default: e = epgx_launch_rows_deriv_v2_nsp4(ctx->stream, da, K); break;
            }
        } else {
            switch (pl->host.n_spaces) {
            case 0: e = epgx_launch_rows_deriv_nsp0(ctx->stream, da, K); break;
            case 1: e = epgx_launch_rows_deriv_nsp1(ctx->stream, da, K); break;
            case 2: e = epgx_launch_rows_deriv_nsp2(ctx->stream, da, K); break;
            default: e = epgx_launch_rows_deriv_nsp4(ctx->stream, da, K); break;
            }
        }
        break;
    case FAM_PACKED_DERIV: e = epgx_launch_packed_deriv(ctx->stream, da, K, pl->host.n_spaces, pl->host.n_vars); break;
    default: e = epgx_launch_deriv(ctx->stream, da, K, pl->host.n_spaces, pl->host.n_vars); break;
    }
    return e;
}

// K = 2048 in two legs per slab of voxels: records [0, j1) on one wavefront per voxel at 512 orders (run_kernel<8, ..>: the growing
// kernel cannot hand its state on -- epgx_cgrow.hip), its state [3][512] + density through a scratch buffer (24 KiB per voxel:
// slabs of at most 8 GiB), then the records [j1, n_rec) on four wavefronts per voxel
static hipError_t launch_two_legs(epgx_ctx *ctx, const epgx_plan *pl, const RunArgs &a, const RangeLists &rl) {
    const int64_t nvox = a.nvox, vox0 = a.t.vox0;
    const int j1 = rl.cgrow[3], j2 = rl.cgrow[4], j3 = rl.cgrow[5];
    const int64_t per_voxel = (int64_t)3 * 512 * sizeof(d2) + sizeof(double);
    const int64_t slab = slab_voxels(nvox, per_voxel, knobs().slab_voxels, 0);
    void *scratch = nullptr;
    hipError_t e = dev_alloc(ctx, &scratch, (size_t)(slab * per_voxel));
    if (e != hipSuccess) return e;
    d2 *st = (d2 *)scratch;
    double *dn = (double *)((char *)scratch + slab * 3 * 512 * sizeof(d2));
    if (tracing())
        fprintf(stderr, "[epgx] run: %d records: [0, %d) on one wavefront per voxel, the rest on four (parts 2 and 3 join at %d and %d); slabs of "
                        "%lld voxels\n", rl.n_rec, j1, j2, j3, (long long)slab);
    for (int64_t c0 = 0; c0 < nvox && e == hipSuccess; c0 += slab) {
        RunArgs s = a;
        s.nvox = std::min(slab, nvox - c0);
        s.t.vox0 = vox0 + c0;
        if (s.t.vidx) s.t.vidx += c0;
        if (s.signal) s.signal += c0;
        if (s.dens_in) s.dens_in += c0;
        RunArgs leg = s;      // the first leg: the per-timestep kernel at 512 orders over the records [0, j1), its state to the scratch buffer
        leg.t.n_rec = j1;
        leg.t.prefetch = std::min(leg.t.prefetch, j1);
        leg.out = st;
        leg.t.dens_out = dn;
        leg.t.write_dens = 1;
        e = epgx_launch_run_m8(ctx->stream, leg, pl->host.n_spaces);
        if (e == hipSuccess && j1 < rl.n_rec)
            e = epgx_launch_run_split2048(ctx->stream, s, pl->host.n_spaces, st, dn, j1, j2, j3, rl.first_slot + rl.cgrow_adc3);
    }
    dev_free(ctx, scratch);
    return e;
}

// the records route of a plain plan: RunArgs and the launch of the family `c` names
static hipError_t launch_plain(epgx_ctx *ctx, const epgx_plan *pl, const RunCall &call, int K, const PackedRange *pr, const Choice &c) {
    const RangeLists &rl = pr->lists;
    const epgx_state *in = call.in, *out = call.out;
    const int64_t nvox = call.rq.nvox, vox0 = call.rq.vox0;
    hipError_t e = hipSuccess;
    RunArgs a;
    memset(&a, 0, sizeof(a));
    a.recs = pr->recs(DEV_RECS);
    a.t.n_rec = rl.n_rec;
    a.coef = pl->d_coef;
    a.t.vidx = pl->d_vidx;
    a.t.vidx_ld = pl->vidx_nvox;
    a.nvox = nvox;
    a.in = in ? in->data : nullptr;
    a.out = out ? out->data : nullptr;
    a.dens_in = in ? in->dens : nullptr;
    a.t.dens_out = out ? out->dens : nullptr;
    a.signal = call.signal_col();
    a.signal_ld = call.rq.signal_ld;
    a.t.use_lds = c.lds_mode;
    a.t.seq_slots = rl.seq_slots ? 1 : 0;
    a.t.first_slot = rl.first_slot;
    a.t.vox0 = vox0;
    a.t.dense_spaces = pl->dense_spaces;
    a.t.write_dens = (rl.has_pd || out != in) ? 1 : 0;
    // long record lists over per-voxel tables: prefetch (EPGX_PREFETCH=0 disables, for measurements)
    a.t.prefetch = (knobs().prefetch && !in && rl.n_rec >= 4) ? rl.pf_count : 0;
    // a wave of rows_kernel takes ONE voxel group (rounds 1 and 2 gave it four on big grids; with today's kernels one is faster on
    // every workload measured: MRF C3 44.5 / 45.8 ms, MRF with max_nstate = 10 at 16 orders 27.0 / 28.5 ms, spoiled gradient echo
    // 14.5 / 14.7 ms); a wave of rows_grow_kernel two (C2-L 0.672 -> 0.634 ms per launch; four: the same).  EPGX_GPW=n overrides
    a.groups_per_wave = c.family == FAM_ROWS_GROW ? 2 : 1;
    if (c.runs) {   // run-length folded records (get_packed)
        a.recs = pr->recs(DEV_RUNS);
        a.t.n_rec = rl.n_runs;
    }
    switch (c.family) {
    case FAM_ROWS_GROW:
        a.recs = pr->recs(DEV_GROW);
        a.t.n_rec = rl.n_grow;
        if (tracing())
            fprintf(stderr, "[epgx] run: %d records: [0, %d) at %d orders per voxel, [%d, %d) at %d, the rest at %d\n", rl.n_grow, rl.grow1,
                    rl.grow_cap[0], rl.grow1, rl.grow2, rl.grow_cap[1], rl.grow_cap[2]);
        // (rows layout or one voxel per lane: epgx_launch_grow.h)
        e = epgx_launch_rows_grow(ctx->stream, a, pl->host.n_spaces, rl.grow, rl.grow1, rl.grow2, rl.grow_cap, knobs());
        break;
    case FAM_ROWS:
        switch (K / 16) {
        case 1: e = epgx_launch_rows_r1(ctx->stream, a, pl->host.n_spaces, c.runs); break;
        case 2: e = epgx_launch_rows_r2(ctx->stream, a, pl->host.n_spaces, c.runs); break;
        case 4: e = epgx_launch_rows_r4(ctx->stream, a, pl->host.n_spaces, c.runs); break;
        default: e = epgx_launch_rows_r8(ctx->stream, a, pl->host.n_spaces, c.runs); break;
        }
        break;
    case FAM_RUN_SPLIT:
        if (c.split_grow) e = launch_two_legs(ctx, pl, a, rl);
        else e = epgx_launch_run_split2048(ctx->stream, a, pl->host.n_spaces, nullptr, nullptr, 0, 0, 0, 0);
        break;
    case FAM_RUN_CONTIG: e = epgx_launch_run_contig(ctx->stream, a, K, pl->host.n_spaces); break;
    case FAM_RUN_CONTIG_GROW:
        if (tracing())
            fprintf(stderr, "[epgx] run: %d records: [0, %d) at 64 orders per voxel, [%d, %d) at 128, [%d, %d) at 256, [%d, %d) at 512, the rest at %d\n",
                    rl.n_rec, rl.cgrow[0], rl.cgrow[0], rl.cgrow[1], rl.cgrow[1], rl.cgrow[2], rl.cgrow[2], rl.cgrow[3], K);
        {
            const int g4[4] = {rl.cgrow[0], rl.cgrow[1], rl.cgrow[2], rl.cgrow[3]};
            e = epgx_launch_run_contig_grow(ctx->stream, a, K, pl->host.n_spaces, g4);
        }
        break;
    default:
        switch (K / 64) {
        case 1: e = epgx_launch_run_m1(ctx->stream, a, pl->host.n_spaces); break;
        case 2: e = epgx_launch_run_m2(ctx->stream, a, pl->host.n_spaces); break;
        case 4: e = epgx_launch_run_m4(ctx->stream, a, pl->host.n_spaces); break;
        case 8: e = epgx_launch_run_m8(ctx->stream, a, pl->host.n_spaces); break;
        default: e = epgx_launch_run_m16(ctx->stream, a, pl->host.n_spaces); break;
        }
        break;
    }
    return e;
}

// ROUTE_RECORDS up to the decision, for epgx_run and epgx_kernel_for alike: the lists of the range (cached, or built and uploaded),
// room for its probes, the kernel.  The caller holds pl->cache_lock.  Nothing but NOPs: no records, and the name is "none"
static int plan_records(epgx_plan *pl, const RunCall &call, int K, const PackedRange **pr, Choice *c) {
    const RunRequest &rq = call.rq;
    if (int rc = get_packed(pl, rq.op_begin, rq.op_end, K, pr)) return rc;
    if ((*pr)->lists.has_adc)
        if (int rc = signal_room(rq, false)) return rc;
    if ((*pr)->lists.n_rec == 0) {
        snprintf(c->name, sizeof(c->name), "none");
        return EPGX_OK;
    }
    return choose_kernel(pl->host, (*pr)->lists, rq.op_begin, rq.op_end, K, call.in != nullptr, call.out != nullptr, knobs(), c);
}

// ROUTE_RECORDS, and every piece of the split path
static int run_records(epgx_ctx *ctx, epgx_plan *pl, const RunCall &call, int K) {
    if (int rc = set_device(ctx)) return rc;
    // from here to the launch the plan's caches (packed records, table indices of the voxel range) are read and
    // possibly rebuilt: one host thread at a time per plan (the launch itself is asynchronous)
    std::lock_guard<std::mutex> plan_guard(pl->cache_lock);
    const PackedRange *pr = nullptr;
    Choice c;
    if (int rc = plan_records(pl, call, K, &pr, &c)) return rc;
    if (pr->lists.n_rec == 0) {  // only a state copy may be needed
        if (call.out && call.in && call.out != call.in) return epgx_state_copy(call.out, call.in);
        return EPGX_OK;
    }
    if (tracing()) fprintf(stderr, "[epgx] run: %s -- %s\n", c.name, c.why);
    if (int rc = ensure_vidx(pl, call.rq.vox0, call.rq.nvox)) return rc;
    const hipError_t e = pl->host.n_vars > 0 ? launch_deriv(ctx, pl, call, K, pr, c) : launch_plain(ctx, pl, call, K, pr, c);
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "epgx_run: launch failed: %s", hipGetErrorString(e));
    return EPGX_OK;
}

extern "C" int epgx_run(epgx_ctx *ctx, const epgx_plan *plan, int32_t op_begin, int32_t op_end, int64_t vox0, int64_t nvox,
                        const epgx_state *in, epgx_state *out, int32_t K, void *signal, int64_t signal_ld, int64_t signal_col0) {
    const RunCall call = run_call(ctx, op_begin, op_end, vox0, nvox, in, out, K, signal, signal_ld, signal_col0, false);
    RunDecision d;
    if (int rc = analyse_call(ctx, plan, call, &d)) return rc;
    epgx_plan *pl = const_cast<epgx_plan *>(plan);
    switch (d.route) {
    case ROUTE_NONE: return EPGX_OK;
    case ROUTE_RECORDS: return run_records(ctx, pl, call, d.K);
    default: break;
    }
    if (int rc = set_device(ctx)) return rc;
    return d.route == ROUTE_XSPLIT ? run_exchange_split(ctx, pl, call, d.K) : run_exchange_fused(ctx, pl, call, d);
}

// the same two steps as epgx_run, then the name instead of the launch (the records route: through get_packed and choose_kernel)
extern "C" int epgx_kernel_for(epgx_ctx *ctx, const epgx_plan *plan, int32_t op_begin, int32_t op_end, int32_t K, const epgx_state *in,
                               epgx_state *out, char *name_out, int64_t name_bytes) {
    if (!name_out || name_bytes < 2) return fail(EPGX_ERR_INVALID, "epgx_kernel_for: no room for the name");
    if (!ctx || !plan) return fail(EPGX_ERR_INVALID, "epgx_kernel_for: NULL argument");
    const int64_t nvox = in ? in->nvox : (out ? out->nvox : plan->nvox_total);
    const RunCall call = run_call(ctx, op_begin, op_end, 0, nvox, in, out, K, nullptr, 0, 0, true);
    RunDecision d;
    if (int rc = analyse_call(ctx, plan, call, &d)) return rc;
    const char *name = d.name;
    Choice c;
    if (d.route == ROUTE_RECORDS) {
        epgx_plan *pl = const_cast<epgx_plan *>(plan);
        if (int rc = set_device(ctx)) return rc;
        std::lock_guard<std::mutex> plan_guard(pl->cache_lock);
        const PackedRange *pr = nullptr;
        if (int rc = plan_records(pl, call, d.K, &pr, &c)) return rc;
        name = c.name;
    }
    snprintf(name_out, (size_t)name_bytes, "%s", name);
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ tiled runs: state matrices of any length
// (epgx_tiled.hip; the schedule -- blocks and shift steps -- comes from tiled_schedule, epgx_planner.cpp)

// the handles, then analyse_tiled (epgx_run_check.h): `rq` for a run, NULL and `top0` for an info call
static int tiled_analysis(const char *who, bool deriv, const epgx_ctx *ctx, const epgx_plan *pl, int32_t Kbuf, const TiledRequest *rq, int32_t top0,
                          TiledShape *shape) {
    static const int tiled_m = env_int("EPGX_TILED_M", 8);   // 16: 16 orders per lane, halo 64 (measurements)
    if (!ctx || !pl) return fail(EPGX_ERR_INVALID, "%s: NULL argument", who);
    if (pl->ctx != ctx) return fail(EPGX_ERR_INVALID, "%s: plan belongs to another context", who);
    return analyse_tiled(who, deriv, pl->host, *pl, Kbuf, tiled_m, rq, top0, shape);
}

static int tiled_info(const char *who, bool deriv, epgx_ctx *ctx, const epgx_plan *plan, int32_t Kbuf, int32_t top0, int32_t *blocks,
                      int32_t *shifts, int64_t *tile_launches, int32_t *peak, char *names, int64_t name_bytes) {
    TiledShape shape;
    if (int rc = tiled_analysis(who, deriv, ctx, plan, Kbuf, nullptr, top0, &shape)) return rc;
    const int M = shape.M, H = shape.H;
    TiledSchedule ts;
    if (int rc = tiled_schedule(plan->host, Kbuf, top0, M, H, knobs(), ts)) return rc;
    const int nb = (int)ts.steps.size() - ts.n_shift;
    if (blocks) *blocks = nb;
    if (shifts) *shifts = ts.n_shift;
    if (tile_launches) *tile_launches = ts.tile_launches;
    if (peak) *peak = ts.peak;
    if (names && name_bytes > 1) {
        std::string n = nb ? std::string(deriv ? "tiled_deriv_kernel<" : "tiled_kernel<") + std::to_string(M) + ", " + std::to_string(H) +
                                 (deriv ? ", " + std::to_string(plan->host.n_vars) : std::string()) + ">"
                           : std::string();
        if (ts.n_shift) n += std::string(n.empty() ? "" : " + ") + "tiled_shift";
        snprintf(names, (size_t)name_bytes, "%s", n.empty() ? "none" : n.c_str());
    }
    return EPGX_OK;
}

extern "C" int epgx_tiled_info(epgx_ctx *ctx, const epgx_plan *plan, int32_t Kbuf, int32_t top0, int32_t *blocks, int32_t *shifts,
                               int64_t *tile_launches, int32_t *peak, char *names, int64_t name_bytes) {
    return tiled_info("epgx_tiled_info", false, ctx, plan, Kbuf, top0, blocks, shifts, tile_launches, peak, names, name_bytes);
}

extern "C" int epgx_tiled_deriv_info(epgx_ctx *ctx, const epgx_plan *plan, int32_t Kbuf, int32_t top0, int32_t *blocks, int32_t *shifts,
                                     int64_t *tile_launches, int32_t *peak, char *names, int64_t name_bytes) {
    return tiled_info("epgx_tiled_deriv_info", true, ctx, plan, Kbuf, top0, blocks, shifts, tile_launches, peak, names, name_bytes);
}

// both tiled entry points.  `deriv`: a voxel holds nw = 1 + n_vars state windows [3][Kbuf] per buffer (the state, then its
// derivative states, which start at zero) and the blocks run on tiled_deriv_kernel; a shift by more than H moves every window
static int run_tiled(const char *who, bool deriv, epgx_ctx *ctx, const epgx_plan *plan_c, int64_t vox0, int64_t nvox, const epgx_state *in,
                     int32_t Kbuf, void *signal, int64_t signal_ld, int64_t signal_col0, int64_t slab_voxels) {
    TiledRequest rq;
    rq.vox0 = vox0, rq.nvox = nvox, rq.slab_voxels = slab_voxels, rq.in = facts_of(in, ctx);
    TiledShape shape;
    if (int rc = tiled_analysis(who, deriv, ctx, plan_c, Kbuf, &rq, 0, &shape)) return rc;
    epgx_plan *pl = const_cast<epgx_plan *>(plan_c);
    const int nw = deriv ? 1 + pl->host.n_vars : 1;
    const int M = shape.M, H = shape.H;
    TiledSchedule ts;
    if (int rc = tiled_schedule(pl->host, Kbuf, shape.top0, M, H, knobs(), ts)) return rc;
    if (deriv && ts.drecs.size() != ts.recs.size()) return fail(EPGX_ERR_INVALID, "%s: %zu records, %zu derivative records", who, ts.recs.size(), ts.drecs.size());
    if (ts.has_adc) {
        if (!signal) return fail(EPGX_ERR_INVALID, "%s: the plan contains an ADC but signal is NULL", who);
        if (signal_col0 < 0 || signal_col0 + nvox > signal_ld)
            return fail(EPGX_ERR_INVALID, "%s: signal columns [%lld,%lld) exceed signal_ld=%lld", who, (long long)signal_col0,
                        (long long)(signal_col0 + nvox), (long long)signal_ld);
    }
    if (nvox == 0 || ts.steps.empty()) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    std::lock_guard<std::mutex> plan_guard(pl->cache_lock);
    if (int rc = ensure_vidx(pl, vox0, nvox)) return rc;
    // two buffers [slab][3][Kbuf] + the density: at most 8 GiB per slab (as the two legs at 2048 orders)
    const int64_t per_voxel = (int64_t)2 * nw * 3 * Kbuf * sizeof(d2) + sizeof(double);
    const int64_t slab = epgx::slab_voxels(nvox, per_voxel, knobs().slab_voxels, slab_voxels);
    const size_t buf_bytes = (size_t)slab * nw * 3 * Kbuf * sizeof(d2);
    void *mem = nullptr, *d_recs = nullptr, *d_drecs = nullptr;
    const size_t rec_bytes = (ts.recs.size() + 2) * sizeof(Rec);     // two padding records (the kernel fetches ahead)
    const size_t drec_bytes = (ts.recs.size() + 2) * sizeof(DRec);
    hipError_t e = dev_alloc(ctx, &d_recs, rec_bytes);
    if (e == hipSuccess && deriv) e = dev_alloc(ctx, &d_drecs, drec_bytes);
    if (e == hipSuccess) e = dev_alloc(ctx, &mem, 2 * buf_bytes + (size_t)slab * sizeof(double));
    if (e != hipSuccess) {
        dev_free(ctx, d_recs);
        dev_free(ctx, d_drecs);
        return fail(EPGX_ERR_NOMEM, "%s: %lld voxels x 2 x %d x %d orders: %s", who, (long long)slab, nw, Kbuf, hipGetErrorString(e));
    }
    ts.recs.resize(ts.recs.size() + 2);
    memset(&ts.recs[ts.recs.size() - 2], 0, 2 * sizeof(Rec));
    e = hipMemcpyAsync(d_recs, ts.recs.data(), rec_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (deriv) {
        ts.drecs.resize(ts.recs.size());
        memset(&ts.drecs[ts.drecs.size() - 2], 0, 2 * sizeof(DRec));
        if (e == hipSuccess) e = hipMemcpyAsync(d_drecs, ts.drecs.data(), drec_bytes, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // (the host vectors go away with this call)
    d2 *buf[2] = {(d2 *)mem, (d2 *)((char *)mem + buf_bytes)};
    double *dens = (double *)((char *)mem + 2 * buf_bytes);
    if (tracing())
        fprintf(stderr, "[epgx] %s: %d window(s) per voxel, %zu records, %zu steps (%d shifts by more than %d), %lld tile launches, peak order %d, Kbuf %d, "
                        "slabs of %lld voxels\n", who + 5, nw, ts.recs.size() - 2, ts.steps.size(), ts.n_shift, H, (long long)ts.tile_launches, ts.peak,
                Kbuf, (long long)slab);
    const int W = 64 * M - 2 * H;
    for (int64_t c0 = 0; c0 < nvox && e == hipSuccess; c0 += slab) {
        const int64_t nv = std::min(slab, nvox - c0);
        const size_t used = (size_t)nv * nw * 3 * Kbuf * sizeof(d2);
        e = hipMemsetAsync(buf[0], 0, used, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(buf[1], 0, used, ctx->stream);
        if (e == hipSuccess && in && !deriv)
            e = hipMemcpy2DAsync(buf[0], (size_t)Kbuf * sizeof(d2), in->data + (size_t)c0 * 3 * in->K, (size_t)in->K * sizeof(d2),
                                 (size_t)in->K * sizeof(d2), (size_t)nv * 3, hipMemcpyDeviceToDevice, ctx->stream);
        for (int comp = 0; comp < 3 && e == hipSuccess && in && deriv; ++comp)   // (the start state is window 0 of every voxel: one row per voxel and component)
            e = hipMemcpy2DAsync(buf[0] + (size_t)comp * Kbuf, (size_t)nw * 3 * Kbuf * sizeof(d2),
                                 in->data + (size_t)c0 * 3 * in->K + (size_t)comp * in->K, (size_t)3 * in->K * sizeof(d2),
                                 (size_t)in->K * sizeof(d2), (size_t)nv, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess && in) e = hipMemcpyAsync(dens, in->dens + c0, (size_t)nv * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess && !in) e = epgx_launch_tiled_equilibrium(ctx->stream, buf[0], dens, nullptr, nv, Kbuf, nw);
        for (size_t j = 0; j < ts.steps.size() && e == hipSuccess; ++j) {
            const TiledStep &st = ts.steps[j];
            const d2 *src = buf[j & 1];
            d2 *dst = buf[(j + 1) & 1];
            if (st.shift) {
                // (the windows of a voxel follow each other at the stride of a voxel of the plain layout: nv * nw "voxels")
                e = epgx_launch_tiled_shift(ctx->stream, src, dst, nv * nw, Kbuf, (int32_t)std::min<int64_t>(Kbuf, (int64_t)st.tiles * W), st.shift,
                                            st.kmax);
                continue;
            }
            TiledArgs a;
            memset(&a, 0, sizeof(a));
            a.in = src;
            a.out = dst;
            a.dens = dens;
            a.nvox = nv;
            a.recs = (const Rec *)d_recs;
            a.coef = pl->d_coef;
            a.signal = signal ? (d2 *)signal + signal_col0 + c0 : nullptr;
            a.signal_ld = signal_ld;
            a.rec0 = st.rec0;
            a.rec1 = st.rec1;
            a.Kbuf = Kbuf;
            a.tiles = st.tiles;
            a.t.vidx = pl->d_vidx ? pl->d_vidx + c0 : nullptr;
            a.t.vidx_ld = pl->vidx_nvox;
            a.t.vox0 = vox0 + c0;
            a.t.dense_spaces = pl->dense_spaces;
            if (!deriv) {
                e = epgx_launch_tiled(ctx->stream, a, M, H, pl->host.n_spaces);
                continue;
            }
            TiledDerivArgs da;
            memset(&da, 0, sizeof(da));
            da.a = a;
            da.drecs = (const DRec *)d_drecs;
            da.through_plain = (pl->deriv_flags & EPGX_DERIV_THROUGH_PLAIN_OPS) ? 1 : 0;
            e = epgx_launch_tiled_deriv(ctx->stream, da, M, H, pl->host.n_spaces, pl->host.n_vars);
        }
    }
    dev_free(ctx, mem);
    dev_free(ctx, d_recs);
    dev_free(ctx, d_drecs);
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return EPGX_OK;
}

extern "C" int epgx_run_tiled(epgx_ctx *ctx, const epgx_plan *plan, int64_t vox0, int64_t nvox, const epgx_state *in, int32_t Kbuf,
                              void *signal, int64_t signal_ld, int64_t signal_col0, int64_t slab_voxels) {
    return run_tiled("epgx_run_tiled", false, ctx, plan, vox0, nvox, in, Kbuf, signal, signal_ld, signal_col0, slab_voxels);
}

extern "C" int epgx_run_tiled_deriv(epgx_ctx *ctx, const epgx_plan *plan, int64_t vox0, int64_t nvox, const epgx_state *in, int32_t Kbuf,
                                    void *signal, int64_t signal_ld, int64_t signal_col0, int64_t slab_voxels) {
    return run_tiled("epgx_run_tiled_deriv", true, ctx, plan, vox0, nvox, in, Kbuf, signal, signal_ld, signal_col0, slab_voxels);
}

// ------------------------------------------------------------------------------ RCCL (loaded on first use)
// One gather of signal slabs is the only inter-GPU traffic of the path.  librccl.so.1 is half a
// gigabyte of device code: it is dlopen'ed when the first communicator is asked for, never at library load.
// (When the process has already loaded an RCCL of the same soname -- PyTorch's, say -- dlopen hands back that one.)
namespace {
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};
}  // namespace

static RcclApi *rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // RCCL must sit on the HIP runtime this library is bound to: a process may hold two ROCm stacks (PyTorch
        // wheels bundle their own libamdhip64 + librccl next to the system's, same sonames), and an RCCL of one on
        // the HIP runtime of the other fails in ncclCommInitRank.  So: the librccl that lives NEXT TO the loaded
        // libamdhip64 first, by full path (a bare soname would match whichever copy happens to be loaded already).
        std::vector<std::string> names;
        if (const char *env = getenv("EPGX_RCCL_LIBRARY")) names.emplace_back(env);
        Dl_info where;
        if (dladdr((const void *)&hipGetDeviceCount, &where) && where.dli_fname) {
            std::string dir(where.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash + 1);
                names.push_back(dir + "librccl.so.1");
                names.push_back(dir + "librccl.so");
            }
        }
        names.emplace_back("librccl.so.1");
        for (const std::string &name : names) {
            if (name.empty()) continue;
            api.handle = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            api.error = dlerror();
        }
        if (!api.handle) return;
        bool ok = true;
        auto sym = [&](const char *name) {
            void *p = dlsym(api.handle, name);
            if (!p) {
                ok = false;
                api.error = std::string("librccl lacks ") + name;
            }
            return p;
        };
        api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
        api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
        api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
        api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
        api.Send = (decltype(api.Send))sym("ncclSend");
        api.Recv = (decltype(api.Recv))sym("ncclRecv");
        api.Reduce = (decltype(api.Reduce))sym("ncclReduce");
        api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
        if (!ok) {
            dlclose(api.handle);
            api.handle = nullptr;
        }
    });
    return api.handle ? &api : nullptr;
}

#define RCCL_TRY(api, expr)                                                                                      \
    do {                                                                                                         \
        ncclResult_t r_ = (expr);                                                                                \
        if (r_ != ncclSuccess)                                                                                   \
            return fail(EPGX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, (api)->GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

struct epgx_comm {
    epgx_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    // every transfer runs on the communicator's own stream: behind `ev_in` (what the context's stream held when the
    // transfer was asked for), in front of `ev_out` (epgx_comm_join: the context's stream waits for it)
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
};

// every peer -> root, point to point, in ONE group: the transfers run concurrently, each over the peer's own xGMI
// link to the root (a ring or tree collective would be bound by a single link).  Rank r's `nbytes` land at
// gathered + r * stride; the root's own block is a device-to-device copy unless the slab was produced in place.
static int gather_blocks(RcclApi *api, ncclComm_t comm, hipStream_t stream, int rank, int world, const void *send,
                         void *gathered, int64_t nbytes, int64_t stride, int root) {
    const size_t count = (size_t)(nbytes / 8);
    if (rank == root) {
        char *mine = (char *)gathered + (size_t)rank * (size_t)stride;
        if (send != (const void *)mine && nbytes)
            HIP_TRY(hipMemcpyAsync(mine, send, (size_t)nbytes, hipMemcpyDeviceToDevice, stream));
        if (world > 1 && count) {
            RCCL_TRY(api, api->GroupStart());
            for (int peer = 0; peer < world; ++peer)
                if (peer != root)
                    RCCL_TRY(api, api->Recv((char *)gathered + (size_t)peer * (size_t)stride, count, ncclDouble, peer, comm, stream));
            RCCL_TRY(api, api->GroupEnd());
        }
    } else if (count) {
        RCCL_TRY(api, api->Send(send, count, ncclDouble, root, comm, stream));
    }
    return EPGX_OK;
}

extern "C" int epgx_comm_unique_id(void *id_out) {
    if (!id_out) return fail(EPGX_ERR_INVALID, "epgx_comm_unique_id: NULL argument");
    RcclApi *api = rccl_api();
    if (!api) return fail(EPGX_ERR_UNSUPPORTED, "epgx_comm_unique_id: cannot load librccl.so.1 (set EPGX_RCCL_LIBRARY)");
    static_assert(sizeof(ncclUniqueId) == EPGX_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    RCCL_TRY(api, api->GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return EPGX_OK;
}

extern "C" int epgx_comm_create(epgx_ctx *ctx, const void *id, int32_t rank, int32_t world_size, epgx_comm **out) {
    if (!ctx || !id || !out) return fail(EPGX_ERR_INVALID, "epgx_comm_create: NULL argument");
    *out = nullptr;
    if (world_size < 1 || rank < 0 || rank >= world_size)
        return fail(EPGX_ERR_INVALID, "epgx_comm_create: rank %d of %d", rank, world_size);
    RcclApi *api = rccl_api();
    if (!api) return fail(EPGX_ERR_UNSUPPORTED, "epgx_comm_create: cannot load librccl.so.1 (set EPGX_RCCL_LIBRARY)");
    if (int rc = set_device(ctx)) return rc;
    epgx_comm *cm = new (std::nothrow) epgx_comm();
    if (!cm) return fail(EPGX_ERR_NOMEM, "epgx_comm_create: host allocation failed");
    cm->ctx = ctx;
    cm->rank = rank;
    cm->world = world_size;
    hipError_t e = hipStreamCreateWithFlags(&cm->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&cm->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&cm->ev_out, hipEventDisableTiming);
    if (e != hipSuccess) {
        epgx_comm_destroy(cm);
        return fail(EPGX_ERR_HIP, "epgx_comm_create: %s", hipGetErrorString(e));
    }
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    const ncclResult_t r = api->CommInitRank(&cm->comm, world_size, uid, rank);
    if (r != ncclSuccess) {
        epgx_comm_destroy(cm);
        return fail(EPGX_ERR_HIP, "epgx_comm_create: ncclCommInitRank: %s", api->GetErrorString(r));
    }
    *out = cm;
    return EPGX_OK;
}

extern "C" int epgx_comm_destroy(epgx_comm *cm) {
    if (!cm) return EPGX_OK;
    RcclApi *api = rccl_api();
    (void)hipSetDevice(cm->ctx->device);
    if (cm->stream) (void)hipStreamSynchronize(cm->stream);
    (void)hipStreamSynchronize(cm->ctx->stream);
    if (api && cm->comm) (void)api->CommDestroy(cm->comm);
    if (cm->ev_in) (void)hipEventDestroy(cm->ev_in);
    if (cm->ev_out) (void)hipEventDestroy(cm->ev_out);
    if (cm->stream) (void)hipStreamDestroy(cm->stream);
    delete cm;
    return EPGX_OK;
}

extern "C" int epgx_comm_count(const epgx_comm *cm, int32_t *n_ranks) {
    if (!cm || !n_ranks) return fail(EPGX_ERR_INVALID, "epgx_comm_count: NULL argument");
    RcclApi *api = rccl_api();
    if (!api) return fail(EPGX_ERR_UNSUPPORTED, "epgx_comm_count: librccl is not loaded");
    int n = 0;
    RCCL_TRY(api, api->CommCount(cm->comm, &n));
    *n_ranks = n;
    return EPGX_OK;
}

// the communicator's stream takes over from the context's stream: everything enqueued there so far comes first
static int comm_enter(epgx_comm *cm) {
    HIP_TRY(hipEventRecord(cm->ev_in, cm->ctx->stream));
    HIP_TRY(hipStreamWaitEvent(cm->stream, cm->ev_in, 0));
    return EPGX_OK;
}

extern "C" int epgx_comm_join(epgx_comm *cm) {
    if (!cm) return fail(EPGX_ERR_INVALID, "epgx_comm_join: comm is NULL");
    if (int rc = set_device(cm->ctx)) return rc;
    HIP_TRY(hipEventRecord(cm->ev_out, cm->stream));
    HIP_TRY(hipStreamWaitEvent(cm->ctx->stream, cm->ev_out, 0));
    return EPGX_OK;
}

extern "C" int epgx_comm_gather_part(epgx_comm *cm, const void *send, void *gathered, int64_t nbytes, int64_t block_stride,
                                     int32_t root) {
    if (!cm) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: comm is NULL");
    if (nbytes < 0 || (nbytes & 7)) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: nbytes=%lld must be a non-negative multiple of 8", (long long)nbytes);
    if (block_stride < nbytes) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: block_stride=%lld < nbytes=%lld", (long long)block_stride, (long long)nbytes);
    if (root < 0 || root >= cm->world) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: root %d of %d ranks", root, cm->world);
    if (nbytes && !send) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: send is NULL");
    if (nbytes && cm->rank == root && !gathered) return fail(EPGX_ERR_INVALID, "epgx_comm_gather_part: the root needs a receive buffer");
    RcclApi *api = rccl_api();
    if (!api) return fail(EPGX_ERR_UNSUPPORTED, "epgx_comm_gather_part: librccl is not loaded");
    if (int rc = set_device(cm->ctx)) return rc;
    if (int rc = comm_enter(cm)) return rc;
    return gather_blocks(api, cm->comm, cm->stream, cm->rank, cm->world, send, gathered, nbytes, block_stride, root);
}

extern "C" int epgx_comm_gather(epgx_comm *cm, const void *send, void *gathered, int64_t nbytes, int32_t root) {
    if (int rc = epgx_comm_gather_part(cm, send, gathered, nbytes, nbytes, root)) return rc;
    return epgx_comm_join(cm);
}

extern "C" int epgx_comm_reduce(epgx_comm *cm, const void *send, void *recv, int64_t count, int32_t root) {
    if (!cm) return fail(EPGX_ERR_INVALID, "epgx_comm_reduce: comm is NULL");
    if (count < 0) return fail(EPGX_ERR_INVALID, "epgx_comm_reduce: count < 0");
    if (root < 0 || root >= cm->world) return fail(EPGX_ERR_INVALID, "epgx_comm_reduce: root %d of %d ranks", root, cm->world);
    if (count && !send) return fail(EPGX_ERR_INVALID, "epgx_comm_reduce: send is NULL");
    if (count && cm->rank == root && !recv) return fail(EPGX_ERR_INVALID, "epgx_comm_reduce: the root needs a receive buffer");
    RcclApi *api = rccl_api();
    if (!api) return fail(EPGX_ERR_UNSUPPORTED, "epgx_comm_reduce: librccl is not loaded");
    if (int rc = set_device(cm->ctx)) return rc;
    if (int rc = comm_enter(cm)) return rc;
    if (count)   // (non-root ranks may pass recv = NULL: ncclReduce only writes at the root)
        RCCL_TRY(api, api->Reduce(send, recv, (size_t)count, ncclDouble, ncclSum, root, cm->comm, cm->stream));
    return epgx_comm_join(cm);
}

extern "C" int epgx_memcpy_d2h_2d(epgx_ctx *ctx, void *host, int64_t host_pitch, const void *dptr, int64_t dev_pitch,
                                  int64_t width_bytes, int64_t rows) {
    if (!ctx || width_bytes < 0 || rows < 0 || host_pitch < width_bytes || dev_pitch < width_bytes ||
        (width_bytes && rows && (!host || !dptr)))
        return fail(EPGX_ERR_INVALID, "epgx_memcpy_d2h_2d: bad argument");
    if (int rc = set_device(ctx)) return rc;
    if (width_bytes && rows) {
        HIP_TRY(hipMemcpy2DAsync(host, (size_t)host_pitch, dptr, (size_t)dev_pitch, (size_t)width_bytes, (size_t)rows,
                                 hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return EPGX_OK;
}

// ------------------------------------------------------------------------------ host copy threads
// A few persistent host threads move staged blocks into pageable destinations (first touch of the pages included): one
// thread copies ~10 GB/s into fresh memory, the PCIe link brings 54.  Process-wide (the pipelines of several contexts
// share them), created on first use, never more than the cores this process may use.
namespace {
int usable_cpus() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2 CPU quota (a GPU box hands a job a share of its cores)
        char quota[32];
        long period = 0;
        if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
            n = std::min<long>(n, std::max<long>(1, (atol(quota) + period - 1) / period));
        fclose(f);
    }
    return std::max(1, n);
}

class CopyPool {
    struct Batch {
        std::mutex m;
        std::condition_variable cv;
        int left = 0;
    };
    struct Task {
        const std::function<void(int)> *fn;
        int index;
        Batch *batch;
    };
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Task> queue_;
    std::vector<std::thread> workers_;
    bool stop_ = false;

    static void finish(const Task &t) {
        (*t.fn)(t.index);
        std::lock_guard<std::mutex> g(t.batch->m);
        if (--t.batch->left == 0) t.batch->cv.notify_all();
    }
    void loop() {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || !queue_.empty(); });
                if (queue_.empty()) return;
                t = queue_.front();
                queue_.pop_front();
            }
            finish(t);
        }
    }

    cpu_set_t preferred_;
    bool has_preferred_ = false;

public:
    explicit CopyPool(int n) {
        CPU_ZERO(&preferred_);
        for (int i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &w : workers_) w.join();
    }
    int lanes() const { return std::max<int>(1, (int)workers_.size()); }
    // The workers keep to the CPUs of the NUMA node(s) that hold the staging blocks -- the node next to the GPU: a copy
    // thread on the other socket reads every staged byte across the socket link (measured: the same download 9 ms or 16 - 20 ms
    // from one process to the next, depending on where the scheduler had put the threads).  Union over all contexts.
    void prefer(const cpu_set_t &cpus) {
        std::lock_guard<std::mutex> g(m_);
        CPU_OR(&preferred_, &preferred_, &cpus);
        has_preferred_ = true;
        for (auto &w : workers_) (void)pthread_setaffinity_np(w.native_handle(), sizeof(preferred_), &preferred_);
    }
    // fn(0) .. fn(n - 1) on the workers (on the caller when there are none); returns when all are done
    void parallel(int n, const std::function<void(int)> &fn) {
        if (n <= 0) return;
        if (workers_.empty()) {
            for (int i = 0; i < n; ++i) fn(i);
            return;
        }
        Batch batch;
        batch.left = n;
        {
            std::lock_guard<std::mutex> g(m_);
            for (int i = 0; i < n; ++i) queue_.push_back({&fn, i, &batch});
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> g(batch.m);
        batch.cv.wait(g, [&] { return batch.left == 0; });
    }
    static CopyPool &get() {
        static CopyPool *pool = [] {
            const char *env = getenv("EPGX_COPY_THREADS");
            int n = env ? atoi(env) : std::min(12, usable_cpus() - 2);
            return new CopyPool(std::max(0, n));   // (leaked on purpose: no static-destruction order games at exit)
        }();
        return *pool;
    }
};

// NUMA node that holds the (resident) page at `p`, or -1
int node_of_page(void *p) {
    int status = -1;
    void *pages[1] = {p};
    const long rc = syscall(SYS_move_pages, 0, 1UL, pages, nullptr, &status, 0);
    return rc == 0 ? status : -1;
}

// CPUs of a NUMA node (/sys/devices/system/node/nodeN/cpulist: "0-63,128-191"), restricted to those this process may use
bool node_cpus(int node, cpu_set_t *out) {
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    char text[4096];
    const bool got = fgets(text, sizeof(text), f) != nullptr;
    fclose(f);
    if (!got) return false;
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
    CPU_ZERO(out);
    int n = 0;
    for (char *tok = strtok(text, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int a = 0, b = 0;
        const int k = sscanf(tok, "%d-%d", &a, &b);
        if (k < 1) continue;
        if (k == 1) b = a;
        for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &allowed)) {
                CPU_SET(c, out);
                ++n;
            }
    }
    return n > 0;
}

// rows x width bytes, staged contiguously at `src` (pitch = width), into dst (pitch dst_pitch): split by BYTES over the lanes
void scatter_rows(const char *src, char *dst, size_t dst_pitch, size_t width, int64_t rows) {
    CopyPool &pool = CopyPool::get();
    const size_t total = width * (size_t)rows;
    const int lanes = (int)std::min<size_t>((size_t)pool.lanes(), std::max<size_t>(1, total >> 20));   // at least 1 MiB per lane
    pool.parallel(lanes, [&](int t) {
        size_t at = total * (size_t)t / (size_t)lanes, end = total * (size_t)(t + 1) / (size_t)lanes;
        at &= ~(size_t)63;
        if (t + 1 < lanes) end &= ~(size_t)63;
        while (at < end) {
            const size_t r = at / width, c = at - r * width;
            const size_t n = std::min(width - c, end - at);
            memcpy(dst + r * dst_pitch + c, src + at, n);
            at += n;
        }
    });
}

bool host_is_pinned(const void *p, size_t span) {
    auto one = [](const void *q) {
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        if (hipPointerGetAttributes(&attr, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return attr.type == hipMemoryTypeHost;
    };
    return one(p) && (span <= 1 || one((const char *)p + span - 1));
}

// a [rows][width] byte region of device memory and where it goes on the host; `after`: event (on the context's
// stream) that marks the kernel whose output this is, or null
struct Region {
    const char *src;
    size_t src_pitch;
    char *dst;
    size_t dst_pitch, width;
    int64_t rows;
    hipEvent_t after;
};
}  // namespace

static int ensure_copy_stream(epgx_ctx *ctx, int n_events) {
    if (!ctx->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    while ((int)ctx->slab_events.size() < n_events) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->slab_events.push_back(ev);
    }
    return EPGX_OK;
}

static int ensure_stages(epgx_ctx *ctx) {
    if (!ctx->stages.empty()) return EPGX_OK;
    // 4 x 64 MiB: a block crosses PCIe in 1.2 ms; pinned once per context (~50 ms), EPGX_STAGE_MB / EPGX_STAGES to change
    const char *mb = getenv("EPGX_STAGE_MB"), *nst = getenv("EPGX_STAGES");
    const size_t bytes = (size_t)std::max(1, mb ? atoi(mb) : 64) << 20;
    const int n = std::max(2, nst ? atoi(nst) : 4);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        epgx_ctx::Stage st;
        e = hipHostMalloc(&st.host, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st.done, hipEventDisableTiming);
        if (e == hipSuccess) ctx->stages.push_back(st);
        else if (st.host) (void)hipHostFree(st.host);
    }
    if (e != hipSuccess) {   // all or nothing: a later call tries again
        for (auto &st : ctx->stages) {
            (void)hipEventDestroy(st.done);
            (void)hipHostFree(st.host);
        }
        ctx->stages.clear();
        return fail(e == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP, "staging blocks: %s", hipGetErrorString(e));
    }
    ctx->stage_bytes = bytes;
    {   // the copy threads move next to this memory (EPGX_COPY_AFFINITY=off: wherever the scheduler puts them)
        const char *aff = getenv("EPGX_COPY_AFFINITY");
        cpu_set_t cpus;
        const int node = (aff && strcmp(aff, "off") == 0) ? -1 : node_of_page(ctx->stages[0].host);
        if (node >= 0 && node_cpus(node, &cpus)) CopyPool::get().prefer(cpus);
        if (getenv("EPGX_TRACE")) fprintf(stderr, "[epgx] staging ring: %d x %zu MiB on NUMA node %d\n", n, bytes >> 20, node);
    }
    return EPGX_OK;
}

// The download engine (caller holds ctx->pipeline).  Page-locked destinations receive strided 2-D copies directly;
// pageable ones are filled through the staging ring: tile i + 1 .. i + ring - 1 cross PCIe while the host threads
// scatter tile i into place.  Enqueues on the copy stream; with `pinned` nothing has completed when this returns
// (the caller drains), otherwise everything has.
static int copy_regions(epgx_ctx *ctx, const std::vector<Region> &regions, bool pinned) {
    if (pinned) {
        for (const Region &r : regions) {
            if (!r.rows || !r.width) continue;
            if (r.after) HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, r.after, 0));
            HIP_TRY(hipMemcpy2DAsync(r.dst, r.dst_pitch, r.src, r.src_pitch, r.width, (size_t)r.rows, hipMemcpyDeviceToHost, ctx->copy_stream));
        }
        return EPGX_OK;
    }
    if (int rc = ensure_stages(ctx)) return rc;
    struct Tile { int region; int64_t row0, rows; size_t col0, width; };
    std::vector<Tile> tiles;
    const size_t cap = ctx->stage_bytes;
    for (int ri = 0; ri < (int)regions.size(); ++ri) {
        const Region &r = regions[(size_t)ri];
        if (!r.rows || !r.width) continue;
        if (r.width <= cap) {
            const int64_t per = std::max<int64_t>(1, (int64_t)(cap / r.width));
            for (int64_t r0 = 0; r0 < r.rows; r0 += per) tiles.push_back({ri, r0, std::min(per, r.rows - r0), 0, r.width});
        } else {
            for (int64_t r0 = 0; r0 < r.rows; ++r0)
                for (size_t c0 = 0; c0 < r.width; c0 += cap) tiles.push_back({ri, r0, 1, c0, std::min(cap, r.width - c0)});
        }
    }
    const int ring = (int)ctx->stages.size(), n = (int)tiles.size();
    int waited_region = -1;
    auto issue = [&](int i) -> hipError_t {
        const Tile &t = tiles[(size_t)i];
        const Region &r = regions[(size_t)t.region];
        hipError_t e = hipSuccess;
        if (r.after && t.region != waited_region) e = hipStreamWaitEvent(ctx->copy_stream, r.after, 0);
        waited_region = t.region;
        epgx_ctx::Stage &st = ctx->stages[(size_t)(i % ring)];
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(st.host, t.width, r.src + (size_t)t.row0 * r.src_pitch + t.col0, r.src_pitch, t.width, (size_t)t.rows,
                                 hipMemcpyDeviceToHost, ctx->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(st.done, ctx->copy_stream);
        return e;
    };
    hipError_t e = hipSuccess;
    int issued = 0;
    for (; issued < std::min(ring, n) && e == hipSuccess; ++issued) e = issue(issued);
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        epgx_ctx::Stage &st = ctx->stages[(size_t)(i % ring)];
        e = hipEventSynchronize(st.done);
        if (e != hipSuccess) break;
        const Tile &t = tiles[(size_t)i];
        const Region &r = regions[(size_t)t.region];
        scatter_rows((const char *)st.host, r.dst + (size_t)t.row0 * r.dst_pitch + t.col0, r.dst_pitch, t.width, t.rows);
        if (issued < n) e = issue(issued++);
    }
    if (e != hipSuccess) return fail(EPGX_ERR_HIP, "staged download: %s", hipGetErrorString(e));
    return EPGX_OK;
}

// both streams drain here whatever happened before: the caller may recycle the device scratch and the host block as
// soon as the entry point returns
static int drain_pipeline(epgx_ctx *ctx, int rc, const char *who) {
    const hipError_t e1 = ctx->copy_stream ? hipStreamSynchronize(ctx->copy_stream) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (!rc && (e1 != hipSuccess || e2 != hipSuccess))
        rc = fail(EPGX_ERR_HIP, "%s: %s", who, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return rc;
}

// ------------------------------------------------------------------------------ pipelined run to host memory
extern "C" int epgx_run_to_host(epgx_ctx *ctx, const epgx_plan *plan, int32_t K, int64_t vox0, int64_t nvox, void *signal_dev,
                                int64_t dev_ld, void *signal_host, int64_t host_ld, int64_t host_col0, int64_t slab, int32_t host_dtype) {
    if (!ctx || !plan) return fail(EPGX_ERR_INVALID, "epgx_run_to_host: NULL argument");
    if (host_dtype != EPGX_SIGNAL_C128 && host_dtype != EPGX_SIGNAL_C64)
        return fail(EPGX_ERR_INVALID, "epgx_run_to_host: host_dtype %d is no epgx_signal_dtype", host_dtype);
    const size_t rec = host_dtype == EPGX_SIGNAL_C64 ? sizeof(float2) : sizeof(d2);   // bytes per record on its way to the host
    if (plan->ctx != ctx) return fail(EPGX_ERR_INVALID, "epgx_run_to_host: plan belongs to another context");
    const int n_adc = plan->n_adc;
    if (vox0 < 0 || nvox < 0 || vox0 + nvox > plan->nvox_total)
        return fail(EPGX_ERR_INVALID, "epgx_run_to_host: voxel range [%lld,%lld) outside the grid (%lld voxels)", (long long)vox0,
                    (long long)(vox0 + nvox), (long long)plan->nvox_total);
    if (n_adc > 0 && nvox > 0 && (!signal_dev || !signal_host)) return fail(EPGX_ERR_INVALID, "epgx_run_to_host: signal buffers are NULL");
    if (dev_ld < nvox || host_col0 < 0 || host_ld < host_col0 + nvox)
        return fail(EPGX_ERR_INVALID, "epgx_run_to_host: %lld voxels do not fit rows of %lld (device) / columns [%lld, ..) of %lld (host)",
                    (long long)nvox, (long long)dev_ld, (long long)host_col0, (long long)host_ld);
    if (slab < 0) return fail(EPGX_ERR_INVALID, "epgx_run_to_host: slab < 0");
    if (nvox == 0) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    const auto tic = std::chrono::steady_clock::now();
    if (slab == 0) {   // ~8 slabs, at least 64 Ki voxels each (a launch should fill the chip), whole wavefront groups
        slab = std::max<int64_t>((nvox + 7) / 8, 65536);
        slab = (slab + 63) & ~(int64_t)63;
    }
    slab = std::max(slab, (nvox + 63) / 64);   // (one event per slab, 64 of them)
    if (plan->x_span) slab = (slab + plan->x_span - 1) / plan->x_span * plan->x_span;   // whole compartment groups
    const int n_slabs = (int)((nvox + slab - 1) / slab);
    std::lock_guard<std::mutex> one_at_a_time(ctx->pipeline);
    if (int rc = ensure_copy_stream(ctx, n_slabs)) return rc;
    const bool pinned = n_adc > 0 && host_is_pinned((const char *)signal_host + rec * (size_t)host_col0,
                                                    rec * ((size_t)(n_adc - 1) * (size_t)host_ld + (size_t)nvox));
    const int n_ops = (int)plan->host.ops.size();
    int rc = EPGX_OK;
    // complex64 destination: every slab is narrowed (behind its kernel, on the same stream) into scratch [n_adc][dev_ld] float2
    // of the context's block cache; the copies then move 8 bytes per record
    void *narrow = nullptr;
    if (host_dtype == EPGX_SIGNAL_C64 && n_adc > 0) {
        const hipError_t e = dev_alloc(ctx, &narrow, sizeof(float2) * (size_t)n_adc * (size_t)dev_ld);
        if (e != hipSuccess) return fail(EPGX_ERR_NOMEM, "epgx_run_to_host: scratch for complex64 records: %s", hipGetErrorString(e));
    }
    const char *src_base = narrow ? (const char *)narrow : (const char *)signal_dev;
    std::vector<Region> regions;
    for (int k = 0; k < n_slabs && !rc; ++k) {
        const int64_t j0 = (int64_t)k * slab, nv = std::min(slab, nvox - j0);
        rc = epgx_run(ctx, plan, 0, n_ops, vox0 + j0, nv, nullptr, nullptr, K, signal_dev, dev_ld, j0);
        if (rc || n_adc <= 0) continue;
        if (narrow) rc = launch_narrow(ctx, (const d2 *)signal_dev + j0, dev_ld, (float2 *)narrow + j0, dev_ld, n_adc, nv);
        if (rc) continue;
        hipEvent_t ev = ctx->slab_events[(size_t)k];
        const hipError_t e = hipEventRecord(ev, ctx->stream);
        if (e != hipSuccess) {
            rc = fail(EPGX_ERR_HIP, "epgx_run_to_host: %s", hipGetErrorString(e));
            break;
        }
        Region r = {src_base + rec * (size_t)j0, rec * (size_t)dev_ld,
                    (char *)signal_host + rec * (size_t)(host_col0 + j0), rec * (size_t)host_ld, rec * (size_t)nv,
                    n_adc, ev};
        if (pinned) {   // (straight away: the copy of slab k runs under the kernel of slab k + 1)
            std::vector<Region> single(1, r);
            rc = copy_regions(ctx, single, true);
        } else {
            regions.push_back(r);
        }
    }
    if (!rc && !regions.empty()) rc = copy_regions(ctx, regions, false);
    rc = drain_pipeline(ctx, rc, "epgx_run_to_host");
    if (narrow) dev_free(ctx, narrow);
    if (getenv("EPGX_TRACE"))
        fprintf(stderr, "[epgx] run_to_host %lld voxels x %d rows (%s), %d slabs, %s: %.3f ms\n", (long long)nvox, n_adc,
                narrow ? "complex64" : "complex128", n_slabs, pinned ? "page-locked destination" : "staged into pageable memory",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tic).count());
    return rc;
}

extern "C" int epgx_download_2d(epgx_ctx *ctx, void *host, int64_t host_pitch, const void *dptr, int64_t dev_pitch,
                                int64_t width_bytes, int64_t rows) {
    if (!ctx || width_bytes < 0 || rows < 0 || host_pitch < width_bytes || dev_pitch < width_bytes ||
        (width_bytes && rows && (!host || !dptr)))
        return fail(EPGX_ERR_INVALID, "epgx_download_2d: bad argument");
    if (!width_bytes || !rows) return EPGX_OK;
    if (int rc = set_device(ctx)) return rc;
    std::lock_guard<std::mutex> one_at_a_time(ctx->pipeline);
    if (int rc = ensure_copy_stream(ctx, 1)) return rc;
    hipEvent_t ev = ctx->slab_events[0];
    HIP_TRY(hipEventRecord(ev, ctx->stream));
    const bool pinned = host_is_pinned(host, (size_t)(rows - 1) * (size_t)host_pitch + (size_t)width_bytes);
    std::vector<Region> regions(1, Region{(const char *)dptr, (size_t)dev_pitch, (char *)host, (size_t)host_pitch, (size_t)width_bytes, rows, ev});
    const int rc = copy_regions(ctx, regions, pinned);
    return drain_pipeline(ctx, rc, "epgx_download_2d");
}

// ------------------------------------------------------------------------------ host-buffer convenience
extern "C" int epgx_simulate_f64(epgx_ctx *ctx, const epgx_plan_desc *desc, int32_t K, const double *init_half,
                                 const double *density, void *signal_out, double *state_out, int32_t signal_dtype) {
    if (!ctx || !desc) return fail(EPGX_ERR_INVALID, "epgx_simulate_f64: NULL argument");
    if (signal_dtype != EPGX_SIGNAL_C128 && signal_dtype != EPGX_SIGNAL_C64)
        return fail(EPGX_ERR_INVALID, "epgx_simulate_f64: signal_dtype %d is no epgx_signal_dtype", signal_dtype);
    if (desc->n_adc > 0 && !signal_out) return fail(EPGX_ERR_INVALID, "epgx_simulate_f64: signal_out is NULL");
    epgx_plan *pl = nullptr;
    int rc = epgx_plan_create(ctx, desc, &pl);
    if (rc) return rc;
    const int64_t nvox = pl->nvox_total;
    epgx_state *st = nullptr;
    void *d_sig = nullptr;
    const bool need_state = init_half || density || state_out;
    if (need_state) {
        rc = epgx_state_create(ctx, nvox, K, &st);
        if (!rc && init_half) rc = epgx_state_upload(st, init_half, density);
        else if (!rc && density) rc = epgx_memcpy_h2d(ctx, st->dens, density, (int64_t)sizeof(double) * nvox);
    }
    const int64_t sig_bytes = (int64_t)sizeof(d2) * desc->n_adc * nvox;
    if (!rc && desc->n_adc) rc = epgx_malloc(ctx, sig_bytes, &d_sig);
    if (!rc) {
        const bool from_eq = !init_half;
        // equilibrium start: `in` = NULL unless a custom density must be honoured
        const epgx_state *in = (from_eq && !density) ? nullptr : st;
        if (from_eq && density) {
            // rebuild the equilibrium state from the uploaded density with a RESET-only plan
            epgx_op r;
            memset(&r, 0, sizeof(r));
            r.opcode = EPGX_OP_RESET;
            r.space = -1;
            epgx_plan_desc d1 = *desc;
            d1.n_ops = 1;
            d1.ops = &r;
            d1.n_adc = 0;
            epgx_plan *p1 = nullptr;
            rc = epgx_plan_create(ctx, &d1, &p1);
            if (!rc) rc = epgx_run(ctx, p1, 0, 1, 0, nvox, st, st, K, nullptr, 0, 0);
            epgx_plan_destroy(p1);
        }
        // nothing but the signal to bring back: voxel slabs, each one's columns on their way to the host while the next computes
        const bool piped = !in && !state_out && desc->n_adc > 0 && sig_bytes >= ((int64_t)32 << 20);
        if (!rc && piped) {
            rc = epgx_run_to_host(ctx, pl, K, 0, nvox, d_sig, nvox, signal_out, nvox, 0, 0, signal_dtype);
            if (!rc) {   // done, signal included
                epgx_free(ctx, d_sig);
                epgx_state_destroy(st);
                epgx_plan_destroy(pl);
                return EPGX_OK;
            }
        }
        if (!rc && !piped) rc = epgx_run(ctx, pl, 0, desc->n_ops, 0, nvox, in, state_out ? st : nullptr, K, d_sig, nvox, 0);
    }
    if (!rc && desc->n_adc && signal_dtype == EPGX_SIGNAL_C64) {   // narrowed on the device, then half the bytes over PCIe
        void *small = nullptr;
        rc = epgx_malloc(ctx, sig_bytes / 2, &small);
        if (!rc) rc = launch_narrow(ctx, d_sig, nvox, small, nvox, desc->n_adc, nvox);
        if (!rc) rc = epgx_download_2d(ctx, signal_out, sig_bytes / 2, small, sig_bytes / 2, sig_bytes / 2, 1);
        if (small) epgx_free(ctx, small);
    } else if (!rc && desc->n_adc) {
        rc = epgx_download_2d(ctx, signal_out, sig_bytes, d_sig, sig_bytes, sig_bytes, 1);
    }
    if (!rc && state_out) rc = epgx_state_download(st, state_out, nullptr);
    if (d_sig) epgx_free(ctx, d_sig);
    epgx_state_destroy(st);
    epgx_plan_destroy(pl);
    return rc;
}

// the contexts of epgx_simulate_sharded_f64: one per device, created on first use and kept for the process (a context carries
// its block cache, its copy stream and -- for results in pageable memory -- a ring of page-locked staging blocks that costs
// ~50 ms to pin: per call that was most of a small simulate)
static int sharded_context(int device, epgx_ctx **out) {
    static std::mutex lock;
    static std::map<int, epgx_ctx *> kept;
    std::lock_guard<std::mutex> guard(lock);
    auto hit = kept.find(device);
    if (hit == kept.end()) {
        epgx_ctx *ctx = nullptr;
        if (int rc = epgx_ctx_create(device, &ctx)) return rc;
        hit = kept.emplace(device, ctx).first;
    }
    *out = hit->second;
    return EPGX_OK;
}

// communicator sets of the single-process gather (EPGX_SHARDED_GATHER=rccl): created once per `ngpu`, kept for the process
static int sharded_comms(RcclApi *api, int ngpu, ncclComm_t **out) {
    static std::mutex lock;
    static std::map<int, std::vector<ncclComm_t>> sets;
    std::lock_guard<std::mutex> guard(lock);
    auto hit = sets.find(ngpu);
    if (hit == sets.end()) {
        std::vector<ncclComm_t> comms((size_t)ngpu, nullptr);
        const ncclResult_t r = api->CommInitAll(comms.data(), ngpu, nullptr);
        if (r != ncclSuccess) return fail(EPGX_ERR_HIP, "epgx_simulate_sharded_f64: ncclCommInitAll: %s", api->GetErrorString(r));
        hit = sets.emplace(ngpu, std::move(comms)).first;
    }
    *out = hit->second.data();
    return EPGX_OK;
}

extern "C" int epgx_simulate_sharded_f64(const epgx_plan_desc *desc, int32_t K, int32_t ngpu,
                                         const double *density, void *signal_out, int32_t signal_dtype) {
    if (!desc || !signal_out) return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: NULL argument");
    if (signal_dtype != EPGX_SIGNAL_C128 && signal_dtype != EPGX_SIGNAL_C64)
        return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: signal_dtype %d is no epgx_signal_dtype", signal_dtype);
    const size_t rec = signal_dtype == EPGX_SIGNAL_C64 ? sizeof(float2) : sizeof(d2);
    if (desc->struct_size != sizeof(epgx_plan_desc))
        return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: struct_size = %u, epgx_plan_desc has %zu bytes (ABI %d)", desc->struct_size,
                    sizeof(epgx_plan_desc), EPGX_ABI_VERSION);
    if (desc->ndim < 1 || desc->ndim > EPGX_MAX_DIMS || !desc->grid_shape)
        return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: ndim %d not in [1,%d]", desc->ndim, EPGX_MAX_DIMS);
    if (desc->n_adc < 0) return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: n_adc < 0");
    const int ndev = epgx_device_count();
    if (ngpu < 1 || ngpu > ndev)
        return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: ngpu=%d, %d device(s) visible", ngpu, ndev);
    if (density) return fail(EPGX_ERR_UNSUPPORTED, "epgx_simulate_sharded_f64: custom density not supported");
    int64_t nvox = 1;
    for (int i = 0; i < desc->ndim; ++i) {
        if (desc->grid_shape[i] < 1) return fail(EPGX_ERR_INVALID, "epgx_simulate_sharded_f64: grid_shape[%d] < 1", i);
        nvox *= desc->grid_shape[i];
    }
    const int64_t slab = (nvox + ngpu - 1) / ngpu;
    const int64_t block = (int64_t)sizeof(d2) * desc->n_adc * slab;   // one rank's padded slab [n_adc][slab]
    // The result is a host array: by default every GPU downloads its own slab (ngpu PCIe links, no collective).
    // EPGX_SHARDED_GATHER=rccl gathers the slabs on GPU 0 first (the device-side route of epgx_comm_*, single-process form).
    const char *how = getenv("EPGX_SHARDED_GATHER");
    const bool use_rccl = how && strcmp(how, "rccl") == 0;
    RcclApi *api = use_rccl ? rccl_api() : nullptr;
    if (use_rccl && !api)
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_simulate_sharded_f64: cannot load librccl.so.1 (set EPGX_RCCL_LIBRARY)");
    std::vector<epgx_ctx *> ctxs(ngpu, nullptr);
    std::vector<epgx_plan *> plans(ngpu, nullptr);
    std::vector<void *> sig(ngpu, nullptr);
    std::vector<int64_t> v0(ngpu), nv(ngpu);
    void *gathered = nullptr;   // on device 0: [ngpu][n_adc][slab]
    int rc = EPGX_OK;
    for (int g = 0; g < ngpu && !rc; ++g) {
        v0[g] = std::min<int64_t>(nvox, g * slab);
        nv[g] = std::min<int64_t>(nvox, (g + 1) * slab) - v0[g];
        rc = sharded_context(g, &ctxs[g]);
        if (!rc) rc = epgx_plan_create(ctxs[g], desc, &plans[g]);
        if (!rc && g == 0 && use_rccl) rc = epgx_malloc(ctxs[0], std::max<int64_t>(block * ngpu, 16), &gathered);
        // (gather route: device 0 writes its slab straight into its block of the gathered buffer)
        if (!rc && !(g == 0 && use_rccl)) rc = epgx_malloc(ctxs[g], std::max<int64_t>(block, 16), &sig[g]);
    }
    if (!rc && !use_rccl) {
        // one host thread per device drives that device's slab pipeline (kernel slabs + their copies into the caller's array)
        std::vector<int> rcs(ngpu, EPGX_OK);
        std::vector<std::string> errs(ngpu);
        auto drive = [&](int g) {
            if (nv[g] <= 0) return;
            rcs[g] = epgx_run_to_host(ctxs[g], plans[g], K, v0[g], nv[g], sig[g], slab, signal_out, nvox, v0[g], 0, signal_dtype);
            if (rcs[g]) errs[g] = g_err;   // (thread-local message: carried back to the caller's thread below)
        };
        std::vector<std::thread> pool;
        for (int g = 1; g < ngpu; ++g) pool.emplace_back(drive, g);
        drive(0);
        for (auto &th : pool) th.join();
        for (int g = 0; g < ngpu && !rc; ++g)
            if (rcs[g]) rc = fail(rcs[g], "epgx_simulate_sharded_f64: device %d: %s", g, errs[g].c_str());
    }
    std::vector<void *> nar(ngpu, nullptr);   // complex64 route: the narrowed slabs (device g; on device 0 the gathered narrowed blocks)
    if (!rc && use_rccl) {
        // enqueue every slab first (async: the devices run concurrently), then ONE gather on the device side -- every GPU
        // sends its slab to GPU 0 over its own xGMI link -- and the download through GPU 0's PCIe link.  complex64 records
        // are narrowed where they were computed: half the bytes cross xGMI as well
        const bool c64 = signal_dtype == EPGX_SIGNAL_C64 && desc->n_adc > 0;
        const int64_t wire = c64 ? block / 2 : block;   // bytes of one rank's block on the wire
        for (int g = 0; g < ngpu && !rc; ++g) {
            void *dst = g == 0 ? gathered : sig[g];
            if (nv[g] < slab && desc->n_adc > 0) rc = epgx_memset(ctxs[g], dst, 0, block);   // (ragged / empty slab: defined padding)
            if (!rc && nv[g] > 0) rc = epgx_run(ctxs[g], plans[g], 0, desc->n_ops, v0[g], nv[g], nullptr, nullptr, K, dst, slab, 0);
            if (!rc && c64) rc = epgx_malloc(ctxs[g], std::max<int64_t>(g == 0 ? wire * ngpu : wire, 16), &nar[g]);
            if (!rc && c64) rc = launch_narrow(ctxs[g], dst, slab, nar[g], slab, desc->n_adc, slab);
        }
        void *root = c64 ? nar[0] : gathered;
        ncclComm_t *comms = nullptr;
        if (!rc && desc->n_adc > 0) rc = sharded_comms(api, ngpu, &comms);
        if (!rc && desc->n_adc > 0) {
            ncclResult_t r = api->GroupStart();
            for (int g = 0; g < ngpu && r == ncclSuccess; ++g) {
                if (hipSetDevice(g) != hipSuccess) { r = ncclUnhandledCudaError; break; }
                if (g == 0) {
                    for (int peer = 1; peer < ngpu && r == ncclSuccess; ++peer)
                        r = api->Recv((char *)root + (size_t)peer * (size_t)wire, (size_t)(wire / 8), ncclDouble, peer,
                                      comms[0], ctxs[0]->stream);
                } else {
                    r = api->Send(c64 ? nar[g] : sig[g], (size_t)(wire / 8), ncclDouble, 0, comms[g], ctxs[g]->stream);
                }
            }
            const ncclResult_t r2 = api->GroupEnd();
            if (r == ncclSuccess) r = r2;
            if (r != ncclSuccess) rc = fail(EPGX_ERR_HIP, "epgx_simulate_sharded_f64: RCCL gather: %s", api->GetErrorString(r));
        }
        // block g = [n_adc][slab] -> columns [v0, v0 + nv) of the caller's [n_adc][nvox] array
        for (int g = 0; g < ngpu && !rc; ++g) {
            if (nv[g] <= 0 || desc->n_adc <= 0) continue;
            if (!rc)   // (ordered behind the receives on GPU 0's stream)
                rc = epgx_download_2d(ctxs[0], (char *)signal_out + rec * v0[g], rec * nvox,
                                      (const char *)root + (size_t)g * (size_t)wire, rec * slab, rec * nv[g], desc->n_adc);
        }
    }
    for (int g = 0; g < ngpu; ++g) {
        if (!ctxs[g]) continue;
        int r2 = epgx_ctx_synchronize(ctxs[g]);
        if (!rc) rc = r2;
    }
    for (int g = 0; g < ngpu; ++g) {
        if (!ctxs[g]) continue;
        if (sig[g]) epgx_free(ctxs[g], sig[g]);
        if (nar[g]) epgx_free(ctxs[g], nar[g]);
        if (g == 0 && gathered) epgx_free(ctxs[0], gathered);
        epgx_plan_destroy(plans[g]);     // (the context stays: sharded_context)
    }
    return rc;
}

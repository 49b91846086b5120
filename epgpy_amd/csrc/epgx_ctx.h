// epgx_ctx.h -- the context object and the three helpers the entry points outside epgx_api.hip need of it (epgx_signal.hip): the
// seam between the two units that define the C ABI.  A HIP header, not part of the public ABI.  Plans, states, coordinates,
// communicators and the copy threads stay private to epgx_api.hip, which defines what is declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/epgx.h"
#include "epgx_error.h"

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? EPGX_ERR_NOMEM : EPGX_ERR_HIP,           \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,     \
                        __LINE__);                                                           \
    } while (0)

struct epgx_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t own = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop;
    // caching device allocator: freed blocks are kept and handed out again.  hipMalloc / hipFree
    // cost 1-25 ms each at the sizes of a plan (measured; hipFree also synchronises the device),
    // which dominated a repeated simulate() of the same shape.  Every use of a block is ordered on
    // ctx->stream, so a block can be recycled without waiting for the work that last touched it.
    // (`mem` guards the three containers: ctypes releases the GIL during calls, and one context may be
    // shared by several host threads -- their launches then interleave on the one stream, which is legal)
    std::mutex mem;
    // page-locked host blocks (epgx_host_alloc), recycled the same way; copy stream + events of epgx_run_to_host
    std::vector<std::pair<void *, size_t>> host_cache;
    std::unordered_map<void *, size_t> host_live;
    size_t host_cached_bytes = 0;
    hipStream_t copy_stream = nullptr;
    std::vector<hipEvent_t> slab_events;
    // one slab pipeline at a time per CONTEXT (copy stream, events and staging ring are shared by its host threads);
    // pipelines of different contexts / GPUs run side by side
    std::mutex pipeline;
    // ring of page-locked staging blocks for downloads into ordinary (pageable) host memory (epgx_run_to_host)
    struct Stage { void *host = nullptr; hipEvent_t done = nullptr; };
    std::vector<Stage> stages;
    size_t stage_bytes = 0;
    std::vector<std::pair<void *, size_t>> cache;
    std::unordered_map<void *, size_t> live;
    size_t cached_bytes = 0;
};

namespace epgx {

// a block of ctx's caching allocator; every use of it is ordered on ctx->stream, so dev_free may follow the last launch at once
hipError_t dev_alloc(epgx_ctx *ctx, void **out, size_t bytes);
void dev_free(epgx_ctx *ctx, void *p);
// hipSetDevice(ctx->device): EPGX_OK, or EPGX_ERR_HIP with the message left for epgx_last_error()
int set_device(const epgx_ctx *ctx);

}  // namespace epgx

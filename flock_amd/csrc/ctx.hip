// libflockgpu: context, error reporting, per-kernel HIP-event profiling.
#include <condition_variable>
#include <mutex>
#include <thread>

#include "common.hpp"

using namespace flockgpu;

// ---- the ctx's worker thread: runs the asynchronous calls (the reference's `tokio::spawn(collect(plan))`, context.rs:172-191)
namespace flockgpu {

struct AsyncWorker {
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> task;
    enum { Idle, Queued, Running, Done } state = Idle;
    int rc = FLOCKGPU_OK;
    bool quit = false;
    std::thread th;
    explicit AsyncWorker(int device) {
        th = std::thread([this, device] {
            (void)hipSetDevice(device);
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [this] { return quit || state == Queued; });
                if (quit) return;
                state = Running;
                std::function<int()> fn = std::move(task);
                lk.unlock();
                const int r = fn();
                lk.lock();
                rc = r;
                state = Done;
                cv.notify_all();
            }
        });
    }
    ~AsyncWorker() {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this] { return state == Idle || state == Done; });   // (a call in flight finishes first)
            quit = true;
        }
        cv.notify_all();
        th.join();
    }
};

int ctx_submit(flockgpu_ctx *ctx, std::function<int()> fn) {
    if (!ctx->worker) ctx->worker = new AsyncWorker(ctx->device);
    AsyncWorker *w = ctx->worker;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        if (w->state != AsyncWorker::Idle) return fail(ctx, FLOCKGPU_ERR_INVALID, "async: a call is already in flight on this ctx (flockgpu_ctx_wait first)");
        w->task = std::move(fn);
        w->state = AsyncWorker::Queued;
    }
    w->cv.notify_all();
    return FLOCKGPU_OK;
}

int ctx_wait(flockgpu_ctx *ctx) {
    AsyncWorker *w = ctx->worker;
    if (!w) return fail(ctx, FLOCKGPU_ERR_INVALID, "wait: no asynchronous call was submitted on this ctx");
    std::unique_lock<std::mutex> lk(w->mu);
    if (w->state == AsyncWorker::Idle) {
        lk.unlock();
        return fail(ctx, FLOCKGPU_ERR_INVALID, "wait: no asynchronous call was submitted on this ctx");
    }
    w->cv.wait(lk, [w] { return w->state == AsyncWorker::Done; });
    w->state = AsyncWorker::Idle;
    return w->rc;
}

}  // namespace flockgpu

extern "C" {

int flockgpu_abi_version(void) { return FLOCKGPU_ABI_VERSION; }

int flockgpu_ctx_create(int device, void *hip_stream, flockgpu_ctx **out) {
    if (!out) return FLOCKGPU_ERR_INVALID;
    *out = nullptr;
    flockgpu_ctx *ctx = new (std::nothrow) flockgpu_ctx();
    if (!ctx) return FLOCKGPU_ERR_OOM;
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        if (hip_stream) {
            ctx->stream = static_cast<hipStream_t>(hip_stream);
        } else {
            // a blocking stream: ordered against the legacy default stream, which is what a host that passes no
            // stream (e.g. torch on its default stream) allocates, fills and reads its buffers on
            e = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);
            ctx->owns_stream = (e == hipSuccess);
        }
    }
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    }
    if (e != hipSuccess) {
        // keep the ctx alive so the caller can read the message, but report the failure
        ctx->last_error = std::string("flockgpu_ctx_create: ") + hipGetErrorString(e);
        *out = ctx;
        return FLOCKGPU_ERR_HIP;
    }
    *out = ctx;
    return FLOCKGPU_OK;
}

void flockgpu_ctx_destroy(flockgpu_ctx *ctx) {
    if (!ctx) return;
    delete ctx->worker;   // (joins: a call still in flight finishes first)
    ctx->worker = nullptr;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    profile_drain(ctx);
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->sync_event) (void)hipEventDestroy(ctx->sync_event);
    for (auto &kv : ctx->arena)
        if (kv.second.ptr) dev_free(ctx, kv.second.ptr);
    for (auto &kv : ctx->guarded) {   // (the address ranges stay reserved: flockgpu_free_guarded)
        (void)hipMemUnmap(kv.second.base, kv.second.mapped);
        (void)hipMemRelease(kv.second.handle);
    }
    for (auto &kv : ctx->pinned)
        if (kv.second.ptr) (void)hipHostFree(kv.second.ptr);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *flockgpu_last_error(const flockgpu_ctx *ctx) { return ctx ? ctx->last_error.c_str() : "null ctx"; }

int flockgpu_ctx_synchronize(flockgpu_ctx *ctx) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLOCKGPU_OK;
}

int flockgpu_ctx_wait(flockgpu_ctx *ctx) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    // a plan's asynchronous execute parks its Arrow outputs in the plan: collecting its call from here would orphan them
    if (ctx->plan_in_flight) return fail(ctx, FLOCKGPU_ERR_INVALID, "ctx_wait: the call in flight is a plan's execute (flockgpu_plan_wait collects it)");
    return ctx_wait(ctx);
}

// The asynchronous twins of the batched-window entry points: the argument structs are copied (the host may build them on its
// stack), the arrays they point to are borrowed until flockgpu_ctx_wait returns.
int flockgpu_q3_join_async(flockgpu_ctx *ctx, const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                           const flockgpu_person_cols *person, const flockgpu_windows *person_win, int64_t category_lit,
                           const char *const *state_lits, int n_state_lits, flockgpu_q3_result *out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!auction || !auction_win || !person || !person_win || !out) return fail(ctx, FLOCKGPU_ERR_INVALID, "q3 async: null argument");
    const flockgpu_auction_cols a = *auction;
    const flockgpu_person_cols p = *person;
    const flockgpu_windows aw = *auction_win, pw = *person_win;
    return ctx_submit(ctx, [=] { return flockgpu_q3_join(ctx, &a, &aw, &p, &pw, category_lit, state_lits, n_state_lits, out); });
}

int flockgpu_q5_hot_items_async(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win, flockgpu_q5_result *out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!bid || !win || !out) return fail(ctx, FLOCKGPU_ERR_INVALID, "q5 async: null argument");
    const flockgpu_bid_cols b = *bid;
    const flockgpu_windows w = *win;
    return ctx_submit(ctx, [=] { return flockgpu_q5_hot_items(ctx, &b, &w, out); });
}

int flockgpu_q8_join_async(flockgpu_ctx *ctx, const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                           const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win, flockgpu_q8_result *out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!auction || !auction_win || !person || !person_win || !out) return fail(ctx, FLOCKGPU_ERR_INVALID, "q8 async: null argument");
    const flockgpu_auction_cols a = *auction;
    const flockgpu_person_cols p = *person;
    const flockgpu_windows aw = *auction_win, pw = *person_win;
    return ctx_submit(ctx, [=] { return flockgpu_q8_join(ctx, &p, &pw, &a, &aw, out); });
}

int flockgpu_malloc(flockgpu_ctx *ctx, size_t bytes, void **out_device_ptr) {
    if (!ctx || !out_device_ptr) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipSetDevice(ctx->device));
    *out_device_ptr = nullptr;
    hipError_t e = hipMalloc(out_device_ptr, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(ctx, FLOCKGPU_ERR_OOM, "flockgpu_malloc(%zu): %s", bytes, hipGetErrorString(e));
    return FLOCKGPU_OK;
}

int flockgpu_free(flockgpu_ctx *ctx, void *device_ptr) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!device_ptr) return FLOCKGPU_OK;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FG_HIP(ctx, hipFree(device_ptr));
    return FLOCKGPU_OK;
}

// Device memory that ENDS where mapped address space ends: `bytes` (rounded up to 16) at the tail of a physical allocation mapped into a
// reserved range one granule larger than itself, so the granule behind the buffer stays unmapped and a kernel that reads or writes past
// the end of a column faults instead of landing in a neighbouring allocation (how the unclamped predecessor loads of q3's build and q8's
// persons pass were found -- the second one only by accident, tests/test_gpu_guard.py).
int flockgpu_malloc_guarded(flockgpu_ctx *ctx, size_t bytes, void **out_device_ptr) {
    if (!ctx || !out_device_ptr) return FLOCKGPU_ERR_INVALID;
    *out_device_ptr = nullptr;
    FG_HIP(ctx, hipSetDevice(ctx->device));
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = ctx->device;
    size_t gran = 0;
    FG_HIP(ctx, hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
    if (gran == 0) return fail(ctx, FLOCKGPU_ERR_HIP, "flockgpu_malloc_guarded: zero allocation granularity");
    size_t want = ((bytes ? bytes : 16) + 15) & ~size_t(15);
    flockgpu::GuardedAlloc g;
    g.mapped = (want + gran - 1) / gran * gran;
    g.reserved = g.mapped + gran;
    FG_HIP(ctx, hipMemAddressReserve(&g.base, g.reserved, gran, nullptr, 0));
    hipError_t e = hipMemCreate(&g.handle, g.mapped, &prop, 0);
    if (e == hipSuccess) {
        e = hipMemMap(g.base, g.mapped, 0, g.handle, 0);
        if (e == hipSuccess) {
            hipMemAccessDesc acc{};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            e = hipMemSetAccess(g.base, g.mapped, &acc, 1);
            if (e != hipSuccess) (void)hipMemUnmap(g.base, g.mapped);
        }
        if (e != hipSuccess) (void)hipMemRelease(g.handle);
    }
    if (e != hipSuccess) {
        (void)hipMemAddressFree(g.base, g.reserved);
        return fail(ctx, FLOCKGPU_ERR_OOM, "flockgpu_malloc_guarded(%zu): %s", bytes, hipGetErrorString(e));
    }
    void *p = static_cast<uint8_t *>(g.base) + g.mapped - want;
    ctx->guarded[p] = g;
    *out_device_ptr = p;
    return FLOCKGPU_OK;
}

int flockgpu_free_guarded(flockgpu_ctx *ctx, void *device_ptr) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!device_ptr) return FLOCKGPU_OK;
    auto it = ctx->guarded.find(device_ptr);
    if (it == ctx->guarded.end()) return fail(ctx, FLOCKGPU_ERR_INVALID, "flockgpu_free_guarded: not a pointer of flockgpu_malloc_guarded");
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const flockgpu::GuardedAlloc g = it->second;
    ctx->guarded.erase(it);
    FG_HIP(ctx, hipMemUnmap(g.base, g.mapped));
    FG_HIP(ctx, hipMemRelease(g.handle));
    // The address range stays reserved for the life of the process -- on purpose.  A range that is freed, reserved again and mapped to
    // new physical memory gave kernels the OLD pages (ROCm 7.2, MI355X: the library's arena in guarded memory returned wrong results and
    // faulted as soon as an address came round a second time, and was exact -- 16 of 16 tests -- when no address was ever handed out
    // twice; ordinary hipFree / hipMalloc recycling with the same exact sizes: 16 of 16).  Address space is not what a test run is short of.
    return FLOCKGPU_OK;
}

int flockgpu_memcpy(flockgpu_ctx *ctx, void *dst, const void *src, size_t bytes, int kind) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (bytes == 0) return FLOCKGPU_OK;
    if (!dst || !src) return fail(ctx, FLOCKGPU_ERR_INVALID, "flockgpu_memcpy: null pointer");
    hipMemcpyKind k = kind == FLOCKGPU_H2D ? hipMemcpyHostToDevice
                      : kind == FLOCKGPU_D2H ? hipMemcpyDeviceToHost
                      : kind == FLOCKGPU_D2D ? hipMemcpyDeviceToDevice : hipMemcpyDefault;
    if (k == hipMemcpyDefault) return fail(ctx, FLOCKGPU_ERR_INVALID, "flockgpu_memcpy: bad kind %d", kind);
    FG_HIP(ctx, hipSetDevice(ctx->device));
    FG_HIP(ctx, hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLOCKGPU_OK;
}

int flockgpu_profile_enable(flockgpu_ctx *ctx, int on) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    profile_drain(ctx);
    ctx->profiling = on != 0;
    return FLOCKGPU_OK;
}

int flockgpu_profile_only(flockgpu_ctx *ctx, const char *kernel_name) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    profile_drain(ctx);
    ctx->profile_only = kernel_name ? kernel_name : "";
    return FLOCKGPU_OK;
}

int flockgpu_profile_reset(flockgpu_ctx *ctx) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    profile_drain(ctx);
    ctx->stats.clear();
    ctx->launch_ms.clear();
    return FLOCKGPU_OK;
}

int flockgpu_profile_read(flockgpu_ctx *ctx, flockgpu_kernel_stat *out, int cap, int *n) {
    if (!ctx || !n) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    profile_drain(ctx);
    int i = 0;
    for (auto &kv : ctx->stats) {
        if (out && i < cap) {
            std::memset(out[i].name, 0, sizeof out[i].name);
            std::strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
            out[i].launches = kv.second.launches;
            out[i].total_ms = kv.second.total_ms;
        }
        ++i;
    }
    *n = i;
    return FLOCKGPU_OK;
}

int flockgpu_profile_samples(flockgpu_ctx *ctx, const char *kernel_name, float *out_ms, int cap, int *n) {
    if (!ctx || !n || !kernel_name || cap < 0) return FLOCKGPU_ERR_INVALID;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    profile_drain(ctx);
    auto it = ctx->launch_ms.find(kernel_name);
    const int have = it == ctx->launch_ms.end() ? 0 : (int)it->second.size();
    for (int i = 0; out_ms && i < have && i < cap; ++i) out_ms[i] = it->second[i];
    *n = have;
    return FLOCKGPU_OK;
}

}  // extern "C"

// The process runtime behind every entry point (host side): the last-error text, the one-GPU-per-process binding, the lanes and
// the device scratch they own, the test aids that look at that scratch (include/mi355_nnunet.h, "Device scratch, for tests"), and
// DeviceAllocs, the owner of every other device allocation (common.h).
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "unet_internal.h"

namespace mi355 {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

static std::mutex g_mu;
static int g_bound_device = -1;
static bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

int bind_device() {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0) {
        set_error("no HIP device visible (%s); this library has no CPU fallback", e == hipSuccess ? "none current" : hipGetErrorString(e));
        return MI355_ERR_NO_DEVICE;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_bound_device < 0) {
        if (!is_gfx950(dev)) {
            set_error("HIP device %d is not gfx950 (MI355X); this library has no other code path", dev);
            return MI355_ERR_NO_DEVICE;
        }
        g_bound_device = dev;
    } else if (g_bound_device != dev) {
        set_error("this process is bound to HIP device %d but device %d is current: one process per GPU (weights, arena and "
                  "scratch live on the bound device)", g_bound_device, dev);
        return MI355_ERR_INVALID;
    }
    return MI355_OK;
}

// Lanes (round 5).  Scratch is per STREAM: the first MAX_LANES distinct streams the caller launches on get a lane of their own -
// activation arena, aggregation buffers, split-K partials, small reduction scratch - so that independent pieces of the work (the two
// ensemble members, or two halves of one member's (fold, tile) list: predictor.predict_folds(lanes = 2)) can be in flight on two
// streams at once: the HBM-bound kernels of one lane (norm passes, transposed convs, first layer, aggregation: a sixth of a
// config-3 step) then run beside the matrix-bound kernels of the other instead of in front of them.  Work on ONE stream is ordered
// by that stream, as before.  A stream beyond the table takes over the least recently used lane after a device synchronise.
// SCR_ZEROS / SCR_ZERO_BIAS are read-only once cleared and shared by all lanes.
constexpr int MAX_LANES = MI355_SCRATCH_LANES;
static struct { void *p; size_t bytes; } g_scratch[MAX_LANES][SCR_COUNT];
static struct { hipStream_t s; bool used; unsigned long tick; } g_lane[MAX_LANES];
static unsigned long g_lane_tick = 0;

static int lane_of_locked(hipStream_t s, int *lane) {
    int free_lane = -1, lru = 0;
    for (int i = 0; i < MAX_LANES; ++i) {
        if (g_lane[i].used && g_lane[i].s == s) { g_lane[i].tick = ++g_lane_tick; *lane = i; return MI355_OK; }
        if (!g_lane[i].used && free_lane < 0) free_lane = i;
        if (g_lane[i].used && g_lane[i].tick < g_lane[lru].tick) lru = i;
    }
    if (free_lane < 0) {
        MI355_HIP(hipDeviceSynchronize());  // whatever still runs on the evicted stream's scratch
        free_lane = lru;
    }
    g_lane[free_lane].s = s; g_lane[free_lane].used = true; g_lane[free_lane].tick = ++g_lane_tick;
    *lane = free_lane;
    return MI355_OK;
}

int device_scratch(int slot, hipStream_t stream, size_t bytes, void **out, bool zeroed) {
    MI355_REQUIRE(slot >= 0 && slot < SCR_COUNT && out, "bad scratch slot %d", slot);
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    int lane = 0;
    if (slot != SCR_ZEROS && slot != SCR_ZERO_BIAS) MI355_TRY(lane_of_locked(stream, &lane));
    auto &b = g_scratch[lane][slot];
    if (b.bytes < bytes) {
        if (b.p) {
            MI355_HIP(hipDeviceSynchronize());  // work in flight may still use the old buffer
            MI355_HIP(hipFree(b.p));
            b.p = nullptr; b.bytes = 0;
        }
        MI355_HIP(hipMalloc(&b.p, bytes));
        b.bytes = bytes;
        if (zeroed) MI355_HIP(hipMemset(b.p, 0, bytes));
    }
    *out = b.p;
    return MI355_OK;
}

// DeviceAllocs (common.h).  The counters are process-wide: the driver loads two models from two threads.
static std::atomic<int64_t> g_live_allocs{0}, g_live_bytes{0};

int DeviceAllocs::alloc(size_t bytes, void **dev) {
    *dev = nullptr;
    ptrs_.reserve(ptrs_.size() + 1);  // (so that recording the pointer cannot fail once the memory exists)
    MI355_HIP(hipMalloc(dev, bytes));
    ptrs_.push_back(*dev);
    bytes_ += bytes;
    g_live_allocs += 1; g_live_bytes += (int64_t)bytes;
    return MI355_OK;
}
int DeviceAllocs::upload(const void *host, size_t bytes, void **dev) {
    MI355_TRY(alloc(bytes, dev));
    MI355_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return MI355_OK;
}
int DeviceAllocs::upload_or_zero(const void *host_or_null, size_t bytes, void **dev) {
    if (host_or_null) return upload(host_or_null, bytes, dev);
    MI355_TRY(alloc(bytes, dev));
    MI355_HIP(hipMemset(*dev, 0, bytes));
    return MI355_OK;
}
void DeviceAllocs::release() {
    for (size_t i = ptrs_.size(); i-- > 0;) (void)hipFree(ptrs_[i]);
    g_live_allocs -= (int64_t)ptrs_.size(); g_live_bytes -= (int64_t)bytes_;
    ptrs_.clear(); bytes_ = 0;
}

extern "C" int mi355_live_allocations(int64_t *count, int64_t *bytes) {
    MI355_REQUIRE(count && bytes, "mi355_live_allocations: null output");
    *count = g_live_allocs.load(); *bytes = g_live_bytes.load();
    return MI355_OK;
}

// Test aids (mi355_nnunet.h, "Device scratch, for tests"): look at, overwrite and drop what device_scratch hands out.  Host code.
static bool scratch_slot_shared(int slot) { return slot == SCR_ZEROS || slot == SCR_ZERO_BIAS; }
static int lane_peek_locked(hipStream_t s) {  // the lane of a stream, or -1: claims nothing, touches no tick
    for (int i = 0; i < MAX_LANES; ++i)
        if (g_lane[i].used && g_lane[i].s == s) return i;
    return -1;
}

extern "C" int mi355_scratch_sizes(void *stream, int64_t *bytes, int n) {
    MI355_REQUIRE(n >= 0 && (bytes || n == 0), "mi355_scratch_sizes: bad arguments");
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    for (int slot = 0; slot < SCR_COUNT && slot < n; ++slot) {
        if (scratch_slot_shared(slot)) bytes[slot] = (int64_t)g_scratch[0][slot].bytes;
        else bytes[slot] = lane < 0 ? 0 : (int64_t)g_scratch[lane][slot].bytes;
    }
    return SCR_COUNT;
}

extern "C" int64_t mi355_scratch_fill(void *stream, int slot, uint32_t word) {
    MI355_REQUIRE(slot >= -1 && slot < SCR_COUNT, "mi355_scratch_fill: bad scratch slot %d", slot);
    MI355_REQUIRE(slot < 0 || !scratch_slot_shared(slot), "mi355_scratch_fill: slot %d is a shared zero page", slot);
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    if (lane < 0) return 0;
    int64_t filled = 0;
    for (int i = 0; i < SCR_COUNT; ++i) {
        if (scratch_slot_shared(i) || (slot >= 0 && i != slot)) continue;
        auto &b = g_scratch[lane][i];
        if (!b.p || b.bytes < 4) continue;
        MI355_HIP(hipMemsetD32Async((hipDeviceptr_t)b.p, (int)word, b.bytes / 4, (hipStream_t)stream));
        filled += (int64_t)(b.bytes / 4 * 4);
    }
    return filled;
}

extern "C" int mi355_scratch_release(void *stream) {
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    if (lane < 0) return MI355_OK;
    MI355_HIP(hipDeviceSynchronize());  // work in flight may still use the buffers
    for (int i = 0; i < SCR_COUNT; ++i) {
        if (scratch_slot_shared(i)) continue;  // (lane 0 also holds the zero pages of every lane)
        auto &b = g_scratch[lane][i];
        if (b.p) MI355_HIP(hipFree(b.p));
        b.p = nullptr; b.bytes = 0;
    }
    g_lane[lane].used = false; g_lane[lane].s = nullptr; g_lane[lane].tick = 0;
    return MI355_OK;
}

extern "C" int mi355_scratch_zero_pages(int64_t *nonzero_bytes) {
    MI355_REQUIRE(nonzero_bytes, "mi355_scratch_zero_pages: null output");
    const int slots[2] = {SCR_ZEROS, SCR_ZERO_BIAS};
    nonzero_bytes[0] = nonzero_bytes[1] = 0;
    std::lock_guard<std::mutex> lk(g_mu);
    for (int k = 0; k < 2; ++k) {
        auto &b = g_scratch[0][slots[k]];
        if (!b.p) continue;
        MI355_HIP(hipDeviceSynchronize());
        std::vector<unsigned char> host(b.bytes);
        MI355_HIP(hipMemcpy(host.data(), b.p, b.bytes, hipMemcpyDeviceToHost));
        for (unsigned char v : host) nonzero_bytes[k] += v != 0;
    }
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" const char *mi355_last_error(void) { return g_last_error.c_str(); }
extern "C" int mi355_version(void) { return 102; }
extern "C" int mi355_device_count(void) {
    int n = 0, good = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    for (int d = 0; d < n; ++d) good += is_gfx950(d) ? 1 : 0;
    return good;
}

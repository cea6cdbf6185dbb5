// Error reporting, per-device launch state and version for libthinktwice_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "tt_common.h"

namespace tt {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

namespace {
struct LdsGrant {
    size_t granted = 0;
    hipError_t refusal = hipSuccess;
};
struct LaunchState {
    void* zero_page = nullptr;
    std::unordered_map<const void*, LdsGrant> lds;     // per kernel
};
std::mutex g_launch_mutex;
LaunchState g_launch[kMaxDevices];

int current_device(const char* who) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        if (who) set_error("%s: no current device", who);
        return -1;
    }
    return dev;
}
}  // namespace

const void* zero_page(const char* who) {
    const int dev = current_device(who);
    if (dev < 0) return nullptr;
    std::lock_guard<std::mutex> lock(g_launch_mutex);
    void*& z = g_launch[dev].zero_page;
    if (!z) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, 256);
        if (e == hipSuccess && (e = hipMemset(p, 0, 256)) != hipSuccess) (void)hipFree(p);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: cannot allocate the zero page on device %d: %s", who, dev, hipGetErrorString(e));
            return nullptr;
        }
        z = p;
    }
    return z;
}

int lds_opt_in(const void* kernel, size_t bytes, const char* name) {
    const int dev = current_device(name);
    if (dev < 0) return -1;
    std::lock_guard<std::mutex> lock(g_launch_mutex);
    LdsGrant& g = g_launch[dev].lds[kernel];
    if (bytes <= g.granted) return 0;
    if (g.refusal == hipSuccess) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) {
            g.granted = bytes;
            return 0;
        }
        (void)hipGetLastError();     // a refusal must not surface later as a stale launch error
        g.refusal = e;
    }
    if (name)
        set_error("%s: device %d refuses %zu bytes of dynamic LDS: %s", name, dev, bytes, hipGetErrorString(g.refusal));
    return -1;
}
}  // namespace tt

extern "C" const char* tt_last_error(void) { return tt::g_err; }

// Which kernel the last tt_conv2d_fwd of this thread launched (measurement aid: bench.py groups its per-launch HIP-event
// times by kernel so that the dominant kernel's roofline can be set beside rocprofv3's per-kernel average).
namespace tt { thread_local char g_conv_kernel[96] = ""; }
extern "C" const char* tt_conv_last_kernel(void) { return tt::g_conv_kernel; }
// Measurement aid (tools/conv_trace.py): while set, every workgroup of the LDS-DMA conv kernel writes four wall-clock stamps (10 ns
// ticks: entry, first K tile landed, K loop done, epilogue done) at stamps[blockIdx.x * 4].  Null (the default) in the product.
namespace tt { long long* g_conv_trace = nullptr; }
extern "C" int tt_conv_set_trace(void* stamps_or_null) {
    tt::g_conv_trace = static_cast<long long*>(stamps_or_null);
    return 0;
}
extern "C" int tt_version(void) { return 100; }

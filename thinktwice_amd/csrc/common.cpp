// Error reporting, per-device launch state, the per-device fault word and version for libthinktwice_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
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

// ---- The fault word: one int in pinned, host-mapped memory per device (64 B apart).  A cross-workgroup wait that gives up
// (bounded_wait.h) sets it from the device with a system-scope store; the host reads it without a copy or a synchronisation of its
// own (tt_device_faults), and once it is set tt_mlp_chain_wide / tt_dec_gru / tt_encoder_fwd / tt_decoder_fwd / tt_plan_run refuse
// to run until tt_clear_device_faults().  Allocated under g_launch_mutex, which is taken last (tt_mlp_chain_wide comes here holding
// its pool's mutex; nothing under g_launch_mutex calls out of this file).
namespace {
int* g_fault_words = nullptr;
std::atomic<int> g_max_spin{kWaitMaxSpin};
}  // namespace

int* device_fault_word() {
    const int dev = current_device(nullptr);
    if (dev < 0) return nullptr;
    std::lock_guard<std::mutex> lock(g_launch_mutex);
    if (!g_fault_words) {
        void* p = nullptr;
        if (hipHostMalloc(&p, (size_t)kMaxDevices * 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        memset(p, 0, (size_t)kMaxDevices * 64);
        g_fault_words = static_cast<int*>(p);
    }
    return g_fault_words + (size_t)dev * 16;
}

int pair_wait_max_spin() { return g_max_spin.load(); }

// The check every forward entry point makes first: a wait's time-out is sticky (like a device fault), because whatever ran
// after it consumed poisoned data.
int refuse_after_fault(const char* what) {
    const int f = tt_device_faults();
    if (f > 0) {
        set_error("%s: refused -- an earlier tt_mlp_chain_wide launch on this device gave up waiting at its barrier (its "
                  "outputs are NaN); results since then are invalid.  tt_clear_device_faults() re-arms the device", what);
        return -3;
    }
    return 0;
}
}  // namespace tt

// Non-blocking: the fault word of the CURRENT device (0 = no wait has timed out since the last clear).  Meaningful for the
// work the caller has already synchronised with; any entry point that synchronises anyway (the D2H copy of tt_action_post's
// result, the end of a plan run in tools/plan_host.cpp) checks it there.
extern "C" int tt_device_faults(void) {
    const int dev = tt::current_device(nullptr);
    if (dev < 0) return -2;
    if (!tt::g_fault_words) return 0;
    return __atomic_load_n(tt::g_fault_words + (size_t)dev * 16, __ATOMIC_ACQUIRE);
}

extern "C" int tt_clear_device_faults(void) {
    const int dev = tt::current_device(nullptr);
    if (dev < 0) return -2;
    if (tt::g_fault_words) __atomic_store_n(tt::g_fault_words + (size_t)dev * 16, 0, __ATOMIC_RELEASE);
    return 0;
}

// Blocking form (tests): waits for the device, then reads the fault word.
extern "C" int tt_mlp_chain_wide_faults(void) {
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    return tt_device_faults();
}

// (named after the first kernel that waited; the bound is every bounded_wait's)
extern "C" int tt_mlp_chain_wide_set_max_spin(int polls) {
    tt::g_max_spin.store(polls < 0 ? tt::kWaitMaxSpin : polls);
    return 0;
}

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

// The lane convention of the cores that are written once and compiled twice (png_inflate.h, png_deflate.h, png_checksum.h,
// jpeg_core.h, file_slots.h): as device code by the .hip files, as host C++ by the checkers under tools/.
// Execution model.  The text is written for kLanes = 64 lanes.  `Lanes` names the lanes the caller runs: {l, l + 1} on the
// device, where every lane of the wave calls with its own l, and {0, 64} on the host, where one thread plays all 64 in turn.
// TT_ENC_LANES(l) { ... } is one phase of per-lane work; a value a lane keeps from one phase to the next is a PerLane<T> (a
// register on the device, an array of 64 on the host).  Everything outside a phase is the same in every lane.  Between two
// phases that touch the same shared state stands TT_PNG_SYNC().  So the host runs 64 lanes, not "lane 0 of 1", and the bytes
// are the device's.
// The names stay in the namespaces they were written in (tt_png, tt_pngenc) and the other cores reach them with
// using-declarations: `Lanes` is part of the mangled name of every function the compiler keeps out of line
// (tt_pngenc::plan_block is one), so a namespace of its own here would rename device symbols.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TT_HD __host__ __device__
#else
#define TT_HD
#endif
// TT_PNG_UNIFORM(x): a 32-bit value every lane holds alike, read from LDS or memory.  On the device it is taken from the
// first lane, which tells the compiler what the execution model guarantees: the reader state and every branch on it then
// live in scalar registers and scalar branches.  It changes no value.
#define TT_PNG_UNIFORM(x) ::tt_png::uniform(x)

#if defined(__HIP_DEVICE_COMPILE__)
#define TT_PNG_SYNC() __syncthreads()
#define TT_ENC_ADD(p, v) atomicAdd((p), (v))
#define TT_ENC_OR(p, v) atomicOr((p), (v))
#define TT_ENC_MAX(p, v) atomicMax((p), (v))
#else
#define TT_PNG_SYNC() ((void)0)
#define TT_ENC_ADD(p, v) (*(p) += (v))
#define TT_ENC_OR(p, v) (*(p) |= (v))
#define TT_ENC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif
#define TT_ENC_LANES(l) for (int l = L.lo; l < L.hi; ++l)

namespace tt_png {

template <typename T>
TT_HD inline T uniform(T x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (T)__builtin_amdgcn_readfirstlane((int)x);
#else
    return x;
#endif
}

}  // namespace tt_png

namespace tt_pngenc {

constexpr int kLanes = 64;

struct Lanes {
    int lo, hi;
};

template <typename T>
struct PerLane {
#if defined(__HIP_DEVICE_COMPILE__)
    T v;
    TT_HD T& operator[](int) { return v; }
#else
    T v[kLanes];
    TT_HD T& operator[](int l) { return v[l]; }
#endif
};

// pred != 0, lane by lane, as a mask
TT_HD inline uint64_t ballot(PerLane<int>& pred, Lanes L) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)L;
    return __ballot(pred.v != 0);
#else
    uint64_t m = 0;
    TT_ENC_LANES(l) m |= (uint64_t)(pred[l] != 0) << l;
    return m;
#endif
}

// v[l] becomes the sum of the lanes below l; returns the sum of all
TT_HD inline uint32_t exclusive_scan(PerLane<uint32_t>& v, Lanes L) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t own = v.v;
    uint32_t inc = own;
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, kLanes);
        if (L.lo >= o) inc += t;
    }
    v.v = inc - own;
    return __shfl(inc, kLanes - 1, kLanes);
#else
    uint32_t run = 0;
    TT_ENC_LANES(l) {
        const uint32_t t = v[l];
        v[l] = run;
        run += t;
    }
    return run;
#endif
}

TT_HD inline int popcount64(uint64_t x) { return __builtin_popcountll(x); }
TT_HD inline uint64_t bits_below(int b) { return b >= 64 ? ~0ull : ((1ull << b) - 1); }      // b >= 0

}  // namespace tt_pngenc

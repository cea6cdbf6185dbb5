// The one cross-workgroup wait of the library (the ticket barrier of tt_mlp_chain_wide, the flag hand-over of tt_dec_gru): ONE thread
// polls an agent-scope word until it reaches `target`, bounded by max_spin polls (tt::pair_wait_max_spin(), common.cpp).
//
// A wait that gives up -- the partner workgroups were not all running within max_spin polls: the chip was oversubscribed beyond
// what the host-side occupancy check allows for, or a count is wrong -- is made LOUD, never silent: the device's host-mapped fault
// word (tt::device_fault_word()) is set with a system-scope store and *gave_up (workgroup-shared) is set, on which the caller
// poisons every value the workgroup writes from there on with NaN, so the launch's outputs cannot be mistaken for results.  The
// workgroup still goes on to every later wait, so counters reach their totals and reset themselves.
#pragma once
#include "tt_common.h"

namespace tt {

__device__ __forceinline__ void bounded_wait(const unsigned* word, unsigned target, int* fault, int max_spin, int* gave_up) {
    int spin = 0;
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        if (++spin > max_spin) {
            __hip_atomic_store(fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            *gave_up = 1;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // one cache invalidate after the wait, not one per poll
}

}  // namespace tt

// Device log windows (thinktwice_amd/logvars.py): the logged values of a training job from the loss terms to the closed window
// without the host.  Three tiny kernels; the contract is stated in include/thinktwice_hip.h.
//   tt_logvars_pack        EncoderDecoder._parse_losses (encoder_decoder_framework.py:409-439): log_vars = mean of every entry (a
//                          list: the sum of its means), loss = sum of the entries whose name contains 'loss' -- one launch for the
//                          ~70 one-element torch launches of the Python expression, same bits
//   tt_logvars_accumulate  custom_multi_gpu_test's `results[k] += v * batch_size` (eval_tool.py:96-109) and mmcv's
//                          LogBuffer.update, on the device, gated by the step's gradient norm
//   tt_logvars_flush       mmcv LogBuffer.average + clear_output: hand the closed window over and start the next one
#include "tt_common.h"

namespace tt {

// The table is the kernel argument (640 bytes of the kernarg segment): no upload, no device copy of it to keep alive.
__global__ __launch_bounds__(64) void logvars_pack_kernel(const tt_logvars_terms tab, int n_terms, int n_slots,
                                                          float* __restrict__ packed) {
    __shared__ float val[TT_LOGVARS_MAX_TERMS];
    __shared__ float slot_val[TT_LOGVARS_MAX_TERMS];
    const int t = threadIdx.x;
    if (t < n_terms) val[t] = *tab.term[t];            // the loads go out together; the sums below are one thread's
    __syncthreads();
    if (t != 0) return;
    int i = 0;
    for (int s = 0; s < n_slots; ++s) {
        float v = 0.0f;                                // torch's reduction and Python's sum() both start from +0: 0 + v0 + v1 + ...
        for (; i < n_terms && tab.slot[i] == s; ++i) v = v + val[i];
        slot_val[s] = v;
        packed[s] = v;
    }
    float total = 0.0f;
    for (int s = 0; s < n_slots; ++s)
        if (tab.in_loss[s]) total = total + slot_val[s];
    packed[n_slots] = total;
}

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// v is an f32 and weight an integer below 2^29, so (double)v * weight is exact in f64 (24 + 29 significant bits): the fused and
// the unfused multiply-add round the same sum once, and whichever the compiler picks gives the same bits.
__global__ __launch_bounds__(64) void logvars_accumulate_kernel(const float* __restrict__ packed, int n,
                                                                const float* __restrict__ tail, int n_tail, int weight,
                                                                const float* __restrict__ gate, double* __restrict__ window) {
    const int n_all = n + n_tail;
    if (gate != nullptr && !finite_f32(gate[0])) {      // block-uniform
        if (threadIdx.x == 0) window[n_all + 2] += 1.0;
        return;
    }
    const double w = (double)weight;
    for (int i = threadIdx.x; i < n_all; i += blockDim.x) {
        const float v = i < n ? packed[i] : tail[i - n];
        window[i] += (double)v * w;
    }
    if (threadIdx.x == 0) {
        window[n_all] += w;
        window[n_all + 1] += 1.0;
    }
}

__global__ __launch_bounds__(64) void logvars_flush_kernel(double* __restrict__ window, int n_all, double* __restrict__ out) {
    for (int i = threadIdx.x; i < n_all; i += blockDim.x) {
        out[i] = window[i];
        window[i] = 0.0;
    }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_logvars_pack(const tt_logvars_terms* terms, int n_terms, int n_slots, float* packed, void* stream) {
    TT_REQUIRE(terms && packed, "tt_logvars_pack: null");
    TT_REQUIRE(n_slots >= 1 && n_slots <= n_terms && n_terms <= TT_LOGVARS_MAX_TERMS,
               "tt_logvars_pack: need 1 <= n_slots (%d) <= n_terms (%d) <= %d", n_slots, n_terms, TT_LOGVARS_MAX_TERMS);
    // the slots must walk 0..n_slots-1 in order: the kernel's one pass relies on it
    for (int i = 0; i < n_terms; ++i) {
        TT_REQUIRE(terms->term[i], "tt_logvars_pack: term %d is null", i);
        const int s = terms->slot[i], prev = i ? terms->slot[i - 1] : 0;
        TT_REQUIRE(i ? (s == prev || s == prev + 1) : s == 0, "tt_logvars_pack: slot of term %d is %d after %d", i, s, prev);
    }
    TT_REQUIRE(terms->slot[n_terms - 1] == n_slots - 1, "tt_logvars_pack: the last term's slot is %d, n_slots %d",
               (int)terms->slot[n_terms - 1], n_slots);
    hipLaunchKernelGGL(logvars_pack_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *terms, n_terms, n_slots, packed);
    return check_launch("tt_logvars_pack");
}

extern "C" int tt_logvars_accumulate(const float* packed, int n, const float* tail, int n_tail, int weight, const float* gate,
                                     double* window, void* stream) {
    TT_REQUIRE(packed && window, "tt_logvars_accumulate: null");
    TT_REQUIRE(n >= 1 && n_tail >= 0 && n + n_tail <= 1024 && (n_tail == 0 || tail),
               "tt_logvars_accumulate: bad sizes n %d, n_tail %d", n, n_tail);
    TT_REQUIRE(weight > 0 && weight < (1 << 29), "tt_logvars_accumulate: weight %d outside (0, 2^29)", weight);
    hipLaunchKernelGGL(logvars_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, packed, n, tail, n_tail, weight,
                       gate, window);
    return check_launch("tt_logvars_accumulate");
}

extern "C" int tt_logvars_flush(double* window, int n_all, double* out, void* stream) {
    TT_REQUIRE(window && out, "tt_logvars_flush: null");
    TT_REQUIRE(n_all >= 1 && n_all <= 1027, "tt_logvars_flush: n_all %d outside 1..1027", n_all);
    TT_REQUIRE(out + n_all <= window || window + n_all <= out, "tt_logvars_flush: out overlaps window");
    hipLaunchKernelGGL(logvars_flush_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, window, n_all, out);
    return check_launch("tt_logvars_flush");
}

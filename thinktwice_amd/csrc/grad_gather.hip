// Gradient gather of the torch-autograd training route (thinktwice_amd/autograd_route.py): the reverse sweep of the tape
// (thinktwice_amd/autodiff.py) leaves one separately allocated f32 tensor per parameter (~880, from a few elements to 2.36 M,
// 128 M floats in all); `loss.backward()` has to hand them to autograd scaled by grad_output.  One launch moves all of them into
// ONE flat buffer in flat-parameter order:
//     flat[dst_off[i] .. + count[i])  (=|+=)  scale * src[i][0 .. count[i])
// A pure HBM stream (4 B read + 4 B written per element, + 4 B read when accumulating).  The work is cut BY BYTES, not by
// tensor: the covered element range [first dst_off, last dst_off + count) is cut into pieces of kPiece elements on absolute
// multiples of kPiece, a workgroup takes pieces grid-stride and finds the segment(s) under its piece by binary search in the
// table -- a 2.36 M-element weight is spread over 576 pieces, a run of 64-element biases shares one.  Elements of `flat` that
// no segment covers are never written.
#include "tt_common.h"

namespace tt {

constexpr int kGatherThreads = 256;
constexpr long long kPiece = 4096;          // elements of `flat` per piece (16 KiB): 4 x 16 B per thread
constexpr int kGatherBlocks = kNumCU * 8;   // 8 workgroups of 4 waves fill a CU's 32 wave slots; pieces beyond that grid-stride

template <bool kAcc, bool kScale>
__device__ __forceinline__ float gather_one(float s, float d, float sc) {
    // two separately rounded operations (the library is built with -ffp-contract=off): t = s * scale, then d + t
    const float t = kScale ? s * sc : s;
    return kAcc ? d + t : t;
}

template <bool kAcc, bool kScale>
__global__ __launch_bounds__(kGatherThreads) void grad_gather_kernel(const tt_grad_seg* __restrict__ segs, int nseg,
                                                                     float* __restrict__ flat,
                                                                     const float* __restrict__ scale_dev) {
    const float sc = kScale ? *scale_dev : 1.f;
    const long long lo = segs[0].dst_off;
    const long long hi = segs[nseg - 1].dst_off + segs[nseg - 1].count;
    const long long p0 = lo / kPiece, p1 = (hi + kPiece - 1) / kPiece;
    const int t = threadIdx.x;
    int a = 0;                                   // (a workgroup's pieces ascend: the search resumes from the last hit)
    for (long long p = p0 + blockIdx.x; p < p1; p += gridDim.x) {
        const long long c0 = p * kPiece > lo ? p * kPiece : lo;
        const long long c1 = (p + 1) * kPiece < hi ? (p + 1) * kPiece : hi;
        // the last segment that starts at or before c0 (workgroup-uniform; segment 0 starts at lo <= c0)
        int b = nseg - 1;
        while (a < b) {
            const int m = (a + b + 1) >> 1;
            if (segs[m].dst_off <= c0) a = m; else b = m - 1;
        }
        for (int s = a; s < nseg; ++s) {
            const long long off = segs[s].dst_off;
            if (off >= c1) break;
            const long long end = off + segs[s].count;
            const long long e0 = off > c0 ? off : c0;            // this segment's share of the piece: [e0, e1)
            const long long e1 = end < c1 ? end : c1;
            if (e1 <= e0) continue;                              // (a gap, or an empty segment)
            const int n = (int)(e1 - e0);
            float* __restrict__ d = flat + e0;
            const float* __restrict__ src = reinterpret_cast<const float*>(segs[s].src) + (e0 - off);
            // dword head up to the destination's next 16-byte boundary, 16-byte body, dword tail
            int head = (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2);
            if (head > n) head = n;
            const int nq = (n - head) >> 2;
            const int tail = n - head - (nq << 2);
            if (t < head) d[t] = gather_one<kAcc, kScale>(src[t], kAcc ? d[t] : 0.f, sc);
            float4* __restrict__ dq = reinterpret_cast<float4*>(d + head);
            const float* __restrict__ sb = src + head;
            if ((((uintptr_t)sb) & 15u) == 0) {                  // co-aligned: 16-byte loads and stores
                const float4* __restrict__ sq = reinterpret_cast<const float4*>(sb);
#pragma unroll 4
                for (int q = t; q < nq; q += kGatherThreads) {
                    const float4 v = sq[q];
                    float4 o = kAcc ? dq[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    o.x = gather_one<kAcc, kScale>(v.x, o.x, sc);
                    o.y = gather_one<kAcc, kScale>(v.y, o.y, sc);
                    o.z = gather_one<kAcc, kScale>(v.z, o.z, sc);
                    o.w = gather_one<kAcc, kScale>(v.w, o.w, sc);
                    dq[q] = o;
                }
            } else {                                             // a source view at an odd offset: dword loads, 16-byte stores
#pragma unroll 4
                for (int q = t; q < nq; q += kGatherThreads) {
                    const float* __restrict__ sp = sb + (q << 2);
                    const float v0 = sp[0], v1 = sp[1], v2 = sp[2], v3 = sp[3];
                    float4 o = kAcc ? dq[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    o.x = gather_one<kAcc, kScale>(v0, o.x, sc);
                    o.y = gather_one<kAcc, kScale>(v1, o.y, sc);
                    o.z = gather_one<kAcc, kScale>(v2, o.z, sc);
                    o.w = gather_one<kAcc, kScale>(v3, o.w, sc);
                    dq[q] = o;
                }
            }
            if (t < tail) {
                const int i = head + (nq << 2) + t;
                d[i] = gather_one<kAcc, kScale>(src[i], kAcc ? d[i] : 0.f, sc);
            }
        }
    }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_grad_gather(const tt_grad_seg* segs_dev, int nseg, float* flat, const float* scale_dev_or_null,
                              int accumulate, void* stream) {
    TT_REQUIRE(nseg >= 0, "tt_grad_gather: nseg %d", nseg);
    if (nseg == 0) return 0;                 // nothing to move: no launch
    TT_REQUIRE(segs_dev && flat, "tt_grad_gather: null table / destination");
    TT_REQUIRE(((uintptr_t)flat & 3u) == 0 && ((uintptr_t)segs_dev & 7u) == 0, "tt_grad_gather: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(kGatherBlocks), block(kGatherThreads);
    if (accumulate) {
        if (scale_dev_or_null)
            hipLaunchKernelGGL((grad_gather_kernel<true, true>), grid, block, 0, st, segs_dev, nseg, flat, scale_dev_or_null);
        else
            hipLaunchKernelGGL((grad_gather_kernel<true, false>), grid, block, 0, st, segs_dev, nseg, flat, scale_dev_or_null);
    } else {
        if (scale_dev_or_null)
            hipLaunchKernelGGL((grad_gather_kernel<false, true>), grid, block, 0, st, segs_dev, nseg, flat, scale_dev_or_null);
        else
            hipLaunchKernelGGL((grad_gather_kernel<false, false>), grid, block, 0, st, segs_dev, nseg, flat, scale_dev_or_null);
    }
    return check_launch("tt_grad_gather");
}

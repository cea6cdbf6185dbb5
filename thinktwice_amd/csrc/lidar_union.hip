// tt_lidar_union_sweeps: union2one's multi-sweep cloud (open_loop_training/code/datasets/carla_dataset.py:314-328) and the
// zero rows of mmcv's collate for a whole training batch, one launch.  The contract is stated in include/thinktwice_hip.h.
//
// Pure data movement: 16 bytes read and 20 written per point.  A thread owns one output row per round: it finds the row's
// sweep in the table (per lane: a workgroup may span sweeps and samples), reads the source row as one 16-byte load and leaves
// the five output dwords in LDS at lane * 5 (stride 5 is odd: no bank is hit twice by a half-wave).  The wave's 64 rows are
// 320 contiguous dwords of `out`, which go out as five stores of 64 consecutive dwords each (256 contiguous bytes per
// wave-instruction) instead of five dwords 20 bytes apart per lane.  A workgroup does kRounds such rounds with all its loads
// issued first, so that 64 bytes per lane are in flight, and pays for the table's copy into LDS once per 1024 rows.
#include <limits.h>

#include "tt_common.h"

namespace tt {

constexpr int kUnionThreads = 256;
constexpr int kUnionRounds = 4;
constexpr int kUnionRows = kUnionThreads * kUnionRounds;              // output rows per workgroup
constexpr int kSweepDwords = (int)(sizeof(tt_union_sweep) / 4);       // 20: first_row (2), count, reserved, m (16)
static_assert(sizeof(tt_union_sweep) == 80 && kSweepDwords == 20, "tt_union_sweep is 80 bytes, the matrix at byte 16");

struct UnionTable {
    tt_union_sweep s[TT_UNION_MAX_SWEEPS];
};

__global__ __launch_bounds__(kUnionThreads) void lidar_union_kernel(UnionTable tab, const float4* __restrict__ pts, int num_sweeps,
                                                                    int T, int Np, int total, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[TT_UNION_MAX_SWEEPS * kSweepDwords];
    __shared__ uint32_t s_rows[kUnionRounds][kUnionThreads * 5];
    const int tid = threadIdx.x;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&tab);
        for (int i = tid; i < num_sweeps * kSweepDwords; i += kUnionThreads) s_tab[i] = src[i];
    }
    __syncthreads();

    const int base = blockIdx.x * kUnionRows;                         // (total <= 2^31 - 1024: no overflow below)
    float4 p[kUnionRounds];
    int entry[kUnionRounds], age[kUnionRounds];                       // table entry of the row (-1: padding), t - (T - 1)
#pragma unroll
    for (int k = 0; k < kUnionRounds; ++k) {
        const int g = base + k * kUnionThreads + tid;
        entry[k] = -1;
        age[k] = 0;
        p[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < total) {
            const int b = g / Np;
            int rem = g - b * Np;                                     // row of the sample, then row of the sweep
            for (int t = T - 1; t >= 0 && entry[k] < 0; --t) {
                const int e = b * T + t;
                const int count = (int)s_tab[e * kSweepDwords + 2];
                if (rem < count) {
                    entry[k] = e;
                    age[k] = t - (T - 1);
                } else {
                    rem -= count;
                }
            }
            if (entry[k] >= 0) {
                const long long first = (long long)(((unsigned long long)s_tab[entry[k] * kSweepDwords + 1] << 32) |
                                                    s_tab[entry[k] * kSweepDwords]);
                p[k] = pts[first + rem];
            }
        }
    }

#pragma unroll
    for (int k = 0; k < kUnionRounds; ++k) {
        uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};                         // padding: five +0.0
        if (entry[k] >= 0) {
            const float4 q = p[k];
            if (age[k] == 0) {                                        // key sweep: the bits as they are, time 0.0
                v[0] = __float_as_uint(q.x); v[1] = __float_as_uint(q.y); v[2] = __float_as_uint(q.z); v[3] = __float_as_uint(q.w);
            } else {
                const float4* m = reinterpret_cast<const float4*>(&s_tab[entry[k] * kSweepDwords + 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 r = m[j];
                    v[j] = __float_as_uint(fmaf(r.w, q.w, fmaf(r.z, q.z, fmaf(r.y, q.y, r.x * q.x))));
                }
                v[4] = __float_as_uint((float)age[k]);
            }
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) s_rows[k][tid * 5 + c] = v[c];
    }
    __syncthreads();

    const int wave = tid / kWave, lane = tid % kWave;
    const long long limit = (long long)total * 5;
#pragma unroll
    for (int k = 0; k < kUnionRounds; ++k) {
        const int row0 = k * kUnionThreads + wave * kWave;            // the wave's first row of this round, in the workgroup
        const long long d0 = ((long long)base + row0) * 5;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const long long d = d0 + c * kWave + lane;
            if (d < limit) out[d] = s_rows[k][wave * kWave * 5 + c * kWave + lane];
        }
    }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_lidar_union_sweeps(const float* points_xyzi, long long num_rows, const tt_union_sweep* sweeps, int B, int T,
                                     int Np, float* out, void* stream) {
    const char* me = "tt_lidar_union_sweeps";
    TT_REQUIRE(sweeps && out, "%s: null sweeps / out", me);
    TT_REQUIRE(B >= 1 && Np >= 0 && num_rows >= 0, "%s: bad sizes (B %d, Np %d, num_rows %lld)", me, B, Np, num_rows);
    TT_REQUIRE(T >= 2, "%s: T = %d; a one-frame queue keeps its four-column cloud (carla_dataset.py:327-328 is inside the loop)",
               me, T);
    TT_REQUIRE((long long)B * T <= TT_UNION_MAX_SWEEPS, "%s: B * T = %lld sweeps, at most %d", me, (long long)B * T,
               TT_UNION_MAX_SWEEPS);
    TT_REQUIRE(((uintptr_t)points_xyzi & 15) == 0, "%s: points_xyzi is not 16-byte aligned", me);
    UnionTable tab;
    for (int b = 0; b < B; ++b) {
        long long sum = 0;
        for (int t = 0; t < T; ++t) {
            const tt_union_sweep& s = sweeps[b * T + t];
            TT_REQUIRE(s.first_row >= 0 && s.count >= 0, "%s: sample %d sweep %d: negative first_row %lld / count %d", me, b, t,
                       s.first_row, s.count);
            TT_REQUIRE(s.count == 0 || points_xyzi, "%s: null points_xyzi with %d rows in sample %d sweep %d", me, s.count, b, t);
            // (written as a subtraction: no overflow for any first_row)
            TT_REQUIRE(s.count == 0 || s.first_row <= num_rows - s.count, "%s: sample %d sweep %d: rows %lld + %d end after the %lld rows of points_xyzi",
                       me, b, t, s.first_row, s.count, num_rows);
            sum += s.count;
            tab.s[b * T + t] = s;
        }
        TT_REQUIRE(sum <= Np, "%s: sample %d has %lld points, Np = %d", me, b, sum, Np);
    }
    for (int i = B * T; i < TT_UNION_MAX_SWEEPS; ++i) tab.s[i] = tt_union_sweep{};
    const long long total = (long long)B * Np;
    TT_REQUIRE(total <= (long long)INT_MAX - kUnionRows + 1, "%s: B * Np = %lld output rows, at most %lld", me, total,
               (long long)INT_MAX - kUnionRows + 1);
    if (total == 0) return 0;
    hipLaunchKernelGGL(lidar_union_kernel, dim3((unsigned)div_up(total, kUnionRows)), dim3(kUnionThreads), 0, (hipStream_t)stream,
                       tab, reinterpret_cast<const float4*>(points_xyzi), B * T, T, Np, (int)total,
                       reinterpret_cast<uint32_t*>(out));
    return check_launch(me);
}

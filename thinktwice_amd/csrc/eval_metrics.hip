// Open-loop task metrics on the device (thinktwice_amd/evaluate.py): what a forward's heads say against a loader batch's labels,
// folded into caller-owned accumulators without the host.  The contract of every entry is stated in include/thinktwice_hip.h.
//   tt_eval_seg_confusion   argmax of the seg logits against the label get_downsampled_gt_seg picks (EDF:485-491; the pixel
//                           tt_loss_seg_focal reads) -> a num_classes x num_classes int64 confusion matrix
//   tt_eval_depth_bins      argmax of the depth logits against the bin of get_downsampled_gt_depth (EDF:443-482; the cell
//                           tt_loss_depth_bce supervises) -> five int64 counts
//   tt_eval_decoder         waypoints / Beta parameters / speed of every decoder stage against the expert -> f64 sums
//   tt_eval_pair_*          two precision modes' outputs of one batch against each other
// Counts are integers: each workgroup gathers its own in LDS and issues one global integer add per non-zero cell, so the result
// does not depend on the order and two runs give the same bits.  Maxima of non-negative floats are integer maxima of their bit
// patterns.  f64 sums are formed by ONE workgroup walking the samples in index order (as tt_logvars_accumulate does); no float
// atomic is issued anywhere in this file.  The metric definitions are this project's own; the label conventions are the
// reference's.
#include "tt_common.h"

namespace tt {

constexpr int kEvalThreads = 256;
constexpr int kEvalMaxClasses = 32;     // seg classes (LDS: 32 x 32 counters per workgroup)
constexpr int kEvalMaxStages = 7;       // decoder stages: 8 sums per stage + the speed term fit one wave

typedef unsigned long long u64;

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// argmax over row[0..C) by a group of G adjacent lanes (G a power of two, `sub` = lane % G), ties to the lowest index; nan != 0
// if one of the C values is a NaN (bc is then meaningless).  VEC: the group reads the row as 16-byte pieces (row 16-byte aligned,
// its pitch a multiple of 4 floats; a piece's channels >= C are loaded with it and take no part).  Every lane of the wave calls
// this, `valid` or not: the exchange is a wave operation.
template <int G, bool VEC>
__device__ __forceinline__ void group_argmax(const float* __restrict__ row, int C, int sub, bool valid, float& bv, int& bc,
                                             int& nan) {
    bv = 0.f;
    bc = C;
    nan = 0;
    if (valid) {
        if (VEC) {
            for (int c0 = 4 * sub; c0 < C; c0 += 4 * G) {
                const float4 q = *reinterpret_cast<const float4*>(row + c0);
                const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = c0 + k;
                    if (c < C) {
                        nan |= (e[k] != e[k]) ? 1 : 0;
                        if (bc == C || e[k] > bv) {
                            bv = e[k];
                            bc = c;
                        }
                    }
                }
            }
        } else {
            for (int c = sub; c < C; c += G) {
                const float v = row[c];
                nan |= (v != v) ? 1 : 0;
                if (bc == C || v > bv) {
                    bv = v;
                    bc = c;
                }
            }
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oc = __shfl_xor(bc, m);
        nan |= __shfl_xor(nan, m);
        if (oc < C && (bc == C || ov > bv || (ov == bv && oc < bc))) {
            bv = ov;
            bc = oc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ seg confusion
// G lanes per cell, 256 / G cells per workgroup and pass.  LDS: C*C + 2 counters (bad_label, nonfinite after the matrix).
template <int G, bool VEC>
__global__ __launch_bounds__(kEvalThreads) void eval_seg_confusion_kernel(const float* __restrict__ logits, int cstride, int C,
                                                                          const float* __restrict__ labels, int BN, int H, int W,
                                                                          int factor, u64* __restrict__ conf) {
    __shared__ unsigned int cnt[kEvalMaxClasses * kEvalMaxClasses + 2];
    const int n_cnt = C * C + 2;
    for (int i = threadIdx.x; i < n_cnt; i += kEvalThreads) cnt[i] = 0u;
    __syncthreads();
    const int h = H / factor, w = W / factor;
    const long long total = (long long)BN * h * w;
    constexpr int kCells = kEvalThreads / G;
    const int sub = threadIdx.x % G;
    for (long long base = (long long)blockIdx.x * kCells; base < total; base += (long long)gridDim.x * kCells) {
        const long long i = base + threadIdx.x / G;
        bool valid = i < total;
        float lab_f = 255.f;
        if (valid) {
            const int x = (int)(i % w), y = (int)((i / w) % h);
            const long long bn = i / ((long long)w * h);
            lab_f = labels[(bn * H + (long long)y * factor) * W + (long long)x * factor];
        }
        // the loss's `(long long)label`; 255 = ignore, as there: nothing of the cell is read or counted
        const long long lab = (finite32(lab_f) && fabsf(lab_f) < 1e9f) ? (long long)lab_f : -1;
        const bool lab_ok = lab >= 0 && lab < C;
        const bool skip = !valid || lab == 255;
        float bv;
        int bc, nan;
        group_argmax<G, VEC>(logits + (valid ? i : 0) * cstride, C, sub, !skip && lab_ok, bv, bc, nan);
        if (sub == 0 && !skip) {
            if (!lab_ok) atomicAdd(&cnt[C * C], 1u);
            else if (nan) atomicAdd(&cnt[C * C + 1], 1u);
            else atomicAdd(&cnt[(int)lab * C + bc], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_cnt; i += kEvalThreads)
        if (cnt[i]) atomicAdd(&conf[i], (u64)cnt[i]);
}

// --------------------------------------------------------------------------------------------------------------- depth bins
// One wave per cell: the factor x factor ground-truth pixels and the D logits are each read by the wave's 64 lanes.
template <bool VEC, bool VECGT>
__global__ __launch_bounds__(kEvalThreads) void eval_depth_bins_kernel(const float* __restrict__ logits, int cstride, int D,
                                                                       const float* __restrict__ gt, int BN, int H, int W,
                                                                       int factor, float d0, float dstep, u64* __restrict__ acc) {
    __shared__ u64 sh[5];
    if (threadIdx.x < 5) sh[threadIdx.x] = 0;
    __syncthreads();
    const int h = H / factor, w = W / factor;
    const long long total = (long long)BN * h * w;
    constexpr int kWaves = kEvalThreads / kWave;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    u64 n_fg = 0, n_top1 = 0, n_within1 = 0, sum_abs = 0, n_nan = 0;          // wave-uniform
    for (long long i = (long long)blockIdx.x * kWaves + wave; i < total; i += (long long)gridDim.x * kWaves) {
        const int x = (int)(i % w), y = (int)((i / w) % h);
        const long long bn = i / ((long long)w * h);
        const float* cell = gt + (bn * H + (long long)y * factor) * W + (long long)x * factor;
        float g = 1e5f;
        if (VECGT) {
            const int q_row = factor / 4;
            for (int p = lane; p < factor * q_row; p += kWave) {
                const float4 q = *reinterpret_cast<const float4*>(cell + (long long)(p / q_row) * W + (p % q_row) * 4);
                g = fminf(g, q.x == 0.f ? 1e5f : q.x);
                g = fminf(g, q.y == 0.f ? 1e5f : q.y);
                g = fminf(g, q.z == 0.f ? 1e5f : q.z);
                g = fminf(g, q.w == 0.f ? 1e5f : q.w);
            }
        } else {
            for (int p = lane; p < factor * factor; p += kWave) {
                const float t = cell[(long long)(p / factor) * W + (p % factor)];
                g = fminf(g, t == 0.f ? 1e5f : t);
            }
        }
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) g = fminf(g, __shfl_xor(g, m));   // a minimum: the order does not matter
        g = (g - (d0 - dstep)) / dstep;                                       // the arithmetic of tt_loss_depth_bce
        if (!(g < (float)(D + 1) && g >= 0.f)) g = 0.f;
        const int bin = (int)g;                                               // 0 = background, 1..D = depth bin + 1
        float bv;
        int bc, nan;
        group_argmax<kWave, VEC>(logits + i * cstride, D, lane, bin >= 1, bv, bc, nan);
        if (bin < 1) continue;                                                // (wave-uniform)
        if (nan) {
            n_nan += 1;
            continue;
        }
        const int off = bc > bin - 1 ? bc - (bin - 1) : (bin - 1) - bc;
        n_fg += 1;
        n_top1 += off == 0 ? 1 : 0;
        n_within1 += off <= 1 ? 1 : 0;
        sum_abs += (u64)off;
    }
    if (lane == 0) {
        if (n_fg) atomicAdd(&sh[0], n_fg);
        if (n_top1) atomicAdd(&sh[1], n_top1);
        if (n_within1) atomicAdd(&sh[2], n_within1);
        if (sum_abs) atomicAdd(&sh[3], sum_abs);
        if (n_nan) atomicAdd(&sh[4], n_nan);
    }
    __syncthreads();
    if (threadIdx.x < 5 && sh[threadIdx.x]) atomicAdd(&acc[threadIdx.x], sh[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------ decoder heads
// One workgroup of one wave; thread t < 8 S + 1 owns sum t and walks the samples in index order.  A sample's 8 S + ... reads are
// a few hundred bytes: the kernel is a handful of dependent f64 adds per sample.
__global__ __launch_bounds__(kWave) void eval_decoder_kernel(const float* __restrict__ pred_wp, const float* __restrict__ mu,
                                                             const float* __restrict__ sigma, const float* __restrict__ pred_speed,
                                                             const float* __restrict__ wp, const float* __restrict__ a_mu,
                                                             const float* __restrict__ a_sigma, const float* __restrict__ speed,
                                                             int B, int S, double* __restrict__ sums, u64* __restrict__ counts) {
    const int t = threadIdx.x, n_terms = 8 * S + 1;
    const int s = t / 8, j = t % 8;
    double acc = t < n_terms ? sums[t] : 0.0;             // the running sum goes on: one sequential f64 sum over every sample
    u64 good = 0, bad = 0;
    for (int b = 0; b < B; ++b) {
        int nf = 0;
        for (int k = t; k < S * 8; k += kWave) nf |= finite32(pred_wp[(long long)b * S * 8 + k]) ? 0 : 1;
        for (int k = t; k < S * 2; k += kWave)
            nf |= (finite32(mu[(long long)b * S * 2 + k]) && finite32(sigma[(long long)b * S * 2 + k])) ? 0 : 1;
        if (t == 0) nf |= finite32(pred_speed[b]) ? 0 : 1;
        if (__any(nf)) {                                    // the whole workgroup is this wave
            bad += 1;
            continue;
        }
        good += 1;
        if (t >= n_terms) continue;
        double v;
        if (t == 8 * S) {
            v = fabs(12.0 * (double)pred_speed[b] - (double)speed[b]);         // the head predicts speed / 12 (EDF:198)
        } else if (j < 4) {
            const float* p = pred_wp + ((long long)b * S + s) * 8;
            const float* q = wp + (long long)b * 8;
            double l2 = 0.0, lx = 0.0, ly = 0.0, last = 0.0;
            for (int i = 0; i < 4; ++i) {
                const double dx = (double)p[2 * i] - (double)q[2 * i], dy = (double)p[2 * i + 1] - (double)q[2 * i + 1];
                last = sqrt(dx * dx + dy * dy);
                l2 = l2 + last;
                lx = lx + fabs(dx);
                ly = ly + fabs(dy);
            }
            v = j == 0 ? l2 * 0.25 : j == 1 ? last : j == 2 ? lx * 0.25 : ly * 0.25;
        } else {
            const int c = j & 1;
            const float* pr = j < 6 ? mu : sigma;
            const float* ex = j < 6 ? a_mu : a_sigma;
            v = fabs((double)pr[((long long)b * S + s) * 2 + c] - (double)ex[(long long)b * 2 + c]);
        }
        acc = acc + v;
    }
    if (t < n_terms) sums[t] = acc;
    if (t == 0) {
        counts[0] += good;
        counts[1] += bad;
    }
}

// ---------------------------------------------------------------------------------------------------------- pair deviations
template <bool VEC>
__global__ __launch_bounds__(kEvalThreads) void eval_pair_deviation_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                           long long n, u64* __restrict__ slots) {
    __shared__ unsigned int sh[3];
    if (threadIdx.x < 3) sh[threadIdx.x] = 0u;
    __syncthreads();
    float md = 0.f, ma = 0.f;
    unsigned int nf = 0;
    auto fold = [&](float x, float y) {
        if (!finite32(x) || !finite32(y)) nf += 1;
        else {
            md = fmaxf(md, fabsf(x - y));
            ma = fmaxf(ma, fabsf(x));
        }
    };
    const long long tid = (long long)blockIdx.x * kEvalThreads + threadIdx.x, step = (long long)gridDim.x * kEvalThreads;
    if (VEC) {
        const long long n4 = n / 4;
        for (long long i = tid; i < n4; i += step) {
            const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
            fold(x.x, y.x);
            fold(x.y, y.y);
            fold(x.z, y.z);
            fold(x.w, y.w);
        }
        for (long long i = n4 * 4 + tid; i < n; i += step) fold(a[i], b[i]);
    } else {
        for (long long i = tid; i < n; i += step) fold(a[i], b[i]);
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        md = fmaxf(md, __shfl_xor(md, m));
        ma = fmaxf(ma, __shfl_xor(ma, m));
        nf += __shfl_xor(nf, m);
    }
    if (threadIdx.x % kWave == 0) {      // non-negative floats order as their bit patterns
        atomicMax(&sh[0], __float_as_uint(md));
        atomicMax(&sh[1], __float_as_uint(ma));
        if (nf) atomicAdd(&sh[2], nf);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x]) atomicMax(&slots[threadIdx.x], (u64)sh[threadIdx.x]);
    if (threadIdx.x == 2 && sh[2]) atomicAdd(&slots[2], (u64)sh[2]);
}

// Two waypoint tensors, `points` (x, y) pairs each: the f64 distance of every pair of points, its maximum and its sum in index
// order.  One workgroup: the maximum and the sum are plain read-modify-writes of the caller's slots.
__global__ __launch_bounds__(kWave) void eval_pair_wp_kernel(const float* __restrict__ a, const float* __restrict__ b, int points,
                                                             double* __restrict__ max_sum, u64* __restrict__ counts) {
    __shared__ double d[kWave];
    double mx = 0.0, sum = threadIdx.x == 0 ? max_sum[1] : 0.0;           // the running sum goes on
    u64 good = 0, bad = 0;
    for (int base = 0; base < points; base += kWave) {
        const int i = base + threadIdx.x;
        double v = -1.0;                                                      // -1: not finite, stays out
        if (i < points) {
            const float ax = a[2 * i], ay = a[2 * i + 1], bx = b[2 * i], by = b[2 * i + 1];
            if (finite32(ax) && finite32(ay) && finite32(bx) && finite32(by)) {
                const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
                v = sqrt(dx * dx + dy * dy);
            }
        }
        d[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = points - base < kWave ? points - base : kWave;
            for (int k = 0; k < m; ++k) {
                if (d[k] < 0.0) {
                    bad += 1;
                    continue;
                }
                good += 1;
                sum = sum + d[k];
                mx = fmax(mx, d[k]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        max_sum[0] = fmax(max_sum[0], mx);
        max_sum[1] = sum;
        counts[0] += good;
        counts[1] += bad;
    }
}

template <int G, bool VEC>
__global__ __launch_bounds__(kEvalThreads) void eval_pair_seg_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                     int cstride, int C, long long cells, u64* __restrict__ out) {
    __shared__ unsigned int sh[3];
    if (threadIdx.x < 3) sh[threadIdx.x] = 0u;
    __syncthreads();
    constexpr int kCells = kEvalThreads / G;
    const int sub = threadIdx.x % G;
    unsigned int differ = 0, seen = 0, nonfinite = 0;
    for (long long base = (long long)blockIdx.x * kCells; base < cells; base += (long long)gridDim.x * kCells) {
        const long long i = base + threadIdx.x / G;
        const bool valid = i < cells;
        float va, vb;
        int ca, cb, na, nb;
        group_argmax<G, VEC>(a + (valid ? i : 0) * cstride, C, sub, valid, va, ca, na);
        group_argmax<G, VEC>(b + (valid ? i : 0) * cstride, C, sub, valid, vb, cb, nb);
        if (sub == 0 && valid) {
            if (na | nb) nonfinite += 1;
            else {
                seen += 1;
                differ += ca != cb ? 1 : 0;
            }
        }
    }
    if (differ) atomicAdd(&sh[0], differ);
    if (seen) atomicAdd(&sh[1], seen);
    if (nonfinite) atomicAdd(&sh[2], nonfinite);
    __syncthreads();
    if (threadIdx.x < 3 && sh[threadIdx.x]) atomicAdd(&out[threadIdx.x], (u64)sh[threadIdx.x]);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static inline int eval_grid(long long items, int per_block) {
    const long long need = (items + per_block - 1) / per_block;
    return (int)(need < kNumCU * 8 ? need : kNumCU * 8);
}
// lanes per cell of the 16-byte form: the power of two >= ceil(C / 4), C <= 32
static inline int lanes_per_cell(int C) {
    const int pieces = (C + 3) / 4;
    return pieces <= 1 ? 1 : pieces <= 2 ? 2 : pieces <= 4 ? 4 : 8;
}

}  // namespace tt

using namespace tt;

#define TT_EVAL_SEG_DISPATCH(KERNEL, G_, ...)                                                                               \
    switch (G_) {                                                                                                           \
        case 0: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<1, false>), __VA_ARGS__); break;                                  \
        case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<1, true>), __VA_ARGS__); break;                                   \
        case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<2, true>), __VA_ARGS__); break;                                   \
        case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<4, true>), __VA_ARGS__); break;                                   \
        default: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<8, true>), __VA_ARGS__); break;                                  \
    }

extern "C" int tt_eval_seg_confusion(const float* logits_cl, int cstride, int num_classes, const float* labels, int BN, int H,
                                     int W, int factor, long long* conf, void* stream) {
    TT_REQUIRE(logits_cl && labels && conf, "tt_eval_seg_confusion: null");
    TT_REQUIRE(num_classes >= 1 && num_classes <= kEvalMaxClasses, "tt_eval_seg_confusion: num_classes %d outside 1..%d",
               num_classes, kEvalMaxClasses);
    TT_REQUIRE(cstride >= num_classes, "tt_eval_seg_confusion: num_classes %d > cstride %d", num_classes, cstride);
    TT_REQUIRE(BN > 0 && H > 0 && W > 0 && factor > 0, "tt_eval_seg_confusion: bad sizes BN %d, H %d, W %d, factor %d", BN, H, W,
               factor);
    TT_REQUIRE(H % factor == 0 && W % factor == 0, "tt_eval_seg_confusion: H %d, W %d not divisible by factor %d", H, W, factor);
    const long long total = (long long)BN * (H / factor) * (W / factor);
    const bool vec = cstride % 4 == 0 && aligned16(logits_cl);
    const int G = vec ? lanes_per_cell(num_classes) : 0;
    const dim3 grid(eval_grid(total, kEvalThreads / (G ? G : 1))), block(kEvalThreads);
    TT_EVAL_SEG_DISPATCH(eval_seg_confusion_kernel, G, grid, block, 0, (hipStream_t)stream, logits_cl, cstride, num_classes,
                         labels, BN, H, W, factor, (u64*)conf)
    return check_launch("tt_eval_seg_confusion");
}

extern "C" int tt_eval_depth_bins(const float* logits_cl, int cstride, int D, const float* gt_depth, int BN, int H, int W,
                                  int factor, float d_lo, float d_step, long long* acc, void* stream) {
    TT_REQUIRE(logits_cl && gt_depth && acc, "tt_eval_depth_bins: null");
    TT_REQUIRE(D >= 1 && cstride >= D, "tt_eval_depth_bins: D %d > cstride %d (or D < 1)", D, cstride);
    TT_REQUIRE(BN > 0 && H > 0 && W > 0 && factor > 0 && d_step > 0.f,
               "tt_eval_depth_bins: bad sizes BN %d, H %d, W %d, factor %d, d_step %g", BN, H, W, factor, (double)d_step);
    TT_REQUIRE(H % factor == 0 && W % factor == 0, "tt_eval_depth_bins: H %d, W %d not divisible by factor %d", H, W, factor);
    const long long total = (long long)BN * (H / factor) * (W / factor);
    const bool vec = cstride % 4 == 0 && aligned16(logits_cl);
    const bool vecgt = factor % 4 == 0 && W % 4 == 0 && aligned16(gt_depth);
    const dim3 grid(eval_grid(total, kEvalThreads / kWave)), block(kEvalThreads);
#define TT_EVAL_DEPTH(V, VG)                                                                                              \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_depth_bins_kernel<V, VG>), grid, block, 0, (hipStream_t)stream, logits_cl,    \
                       cstride, D, gt_depth, BN, H, W, factor, d_lo, d_step, (u64*)acc)
    if (vec && vecgt) TT_EVAL_DEPTH(true, true);
    else if (vec) TT_EVAL_DEPTH(true, false);
    else if (vecgt) TT_EVAL_DEPTH(false, true);
    else TT_EVAL_DEPTH(false, false);
#undef TT_EVAL_DEPTH
    return check_launch("tt_eval_depth_bins");
}

extern "C" int tt_eval_decoder(const float* pred_wp, const float* mu_branches, const float* sigma_branches,
                               const float* pred_speed, const float* waypoints, const float* action_mu,
                               const float* action_sigma, const float* speed, int B, int S, double* sums, long long* counts,
                               void* stream) {
    TT_REQUIRE(pred_wp && mu_branches && sigma_branches && pred_speed && waypoints && action_mu && action_sigma && speed && sums &&
                   counts, "tt_eval_decoder: null");
    TT_REQUIRE(B >= 1 && S >= 1 && S <= kEvalMaxStages, "tt_eval_decoder: B %d >= 1, S %d in 1..%d", B, S, kEvalMaxStages);
    hipLaunchKernelGGL(eval_decoder_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, pred_wp, mu_branches, sigma_branches,
                       pred_speed, waypoints, action_mu, action_sigma, speed, B, S, sums, (u64*)counts);
    return check_launch("tt_eval_decoder");
}

extern "C" int tt_eval_pair_deviation(const float* a, const float* b, long long n, long long* slots, void* stream) {
    TT_REQUIRE(a && b && slots, "tt_eval_pair_deviation: null");
    TT_REQUIRE(n >= 1, "tt_eval_pair_deviation: n %lld < 1", n);
    const dim3 grid(eval_grid(n, kEvalThreads * 8)), block(kEvalThreads);
    if (aligned16(a) && aligned16(b))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_pair_deviation_kernel<true>), grid, block, 0, (hipStream_t)stream, a, b, n,
                           (u64*)slots);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_pair_deviation_kernel<false>), grid, block, 0, (hipStream_t)stream, a, b, n,
                           (u64*)slots);
    return check_launch("tt_eval_pair_deviation");
}

extern "C" int tt_eval_pair_wp(const float* a, const float* b, int points, double* max_sum, long long* counts, void* stream) {
    TT_REQUIRE(a && b && max_sum && counts, "tt_eval_pair_wp: null");
    TT_REQUIRE(points >= 1, "tt_eval_pair_wp: points %d < 1", points);
    hipLaunchKernelGGL(eval_pair_wp_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, a, b, points, max_sum, (u64*)counts);
    return check_launch("tt_eval_pair_wp");
}

extern "C" int tt_eval_pair_seg(const float* a_cl, const float* b_cl, int cstride, int num_classes, long long cells,
                                long long* out, void* stream) {
    TT_REQUIRE(a_cl && b_cl && out, "tt_eval_pair_seg: null");
    TT_REQUIRE(num_classes >= 1 && num_classes <= kEvalMaxClasses, "tt_eval_pair_seg: num_classes %d outside 1..%d", num_classes,
               kEvalMaxClasses);
    TT_REQUIRE(cstride >= num_classes && cells >= 1, "tt_eval_pair_seg: num_classes %d > cstride %d (or cells %lld < 1)",
               num_classes, cstride, cells);
    const bool vec = cstride % 4 == 0 && aligned16(a_cl) && aligned16(b_cl);
    const int G = vec ? lanes_per_cell(num_classes) : 0;
    const dim3 grid(eval_grid(cells, kEvalThreads / (G ? G : 1))), block(kEvalThreads);
    TT_EVAL_SEG_DISPATCH(eval_pair_seg_kernel, G, grid, block, 0, (hipStream_t)stream, a_cl, b_cl, cstride, num_classes, cells,
                         (u64*)out)
    return check_launch("tt_eval_pair_seg");
}

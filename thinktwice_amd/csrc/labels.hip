// The two label inputs of the training image pipeline from the dataset's raw bytes: LoadDepth.__call__ and LoadSeg.__call__
// with red_green_yellow (datasets/pipelines/loading.py:84-93, :96-113, :132-162).  thinktwice_hip.h states each entry's
// arithmetic; the conventions (class map, thresholds, the HSV division tables) are built on the host
// (thinktwice_amd/labels.py) and the kernels here execute them.
//
// tt_decode_seg_u8 labels the 8-connected components of every image's traffic-light mask by label equivalence with
// union-find.  A label is a pixel index within the image, a pixel's label never exceeds its own index and only ever
// decreases, so every find and every union loop ends, and no component links two images.  The phases, one launch each (no
// workgroup waits for another):
//   tile      one workgroup per 64 x 16 tile: the class map of every pixel; the tile's mask in LDS, each mask pixel united
//             with its W, NW, N and NE neighbours inside the tile, paths compressed, the root written as an image index
//   edges     every mask pixel on a tile's first row, first column or last column united with those of its W, NW, N and NE
//             neighbours that lie in another tile (corners included)
//   flatten   every mask pixel to its root; a root zeroes its own statistics slot
//   stats S   count and sum of S at the root's slot
//   stats HV  green and red counts at the root's slot, under the threshold that follows from the first two
//   write     light_base + light_type, 0 for a component under min_pixels
// The statistics are integer atomics, a wave's contributions to one root folded into one atomic: the result does not depend
// on their order.
#include <limits.h>

#include <algorithm>

#include "tt_common.h"

namespace tt {

constexpr int kSegTW = 64, kSegTH = 16;             // the tile of the local pass: 4 pixels per thread of a 256-thread workgroup
constexpr int kSegMaxBlocks = 8192;                 // grid-stride launches: 32 workgroups per CU at the most

// ---------------------------------------------------------------------------------------------------------------- depth
__device__ __forceinline__ float depth_of(uint32_t r, uint32_t g, uint32_t b) {
    const float code = (float)(r + 256u * g + 65536u * b);         // < 2^24: exact
    return __fmul_rn(__fdiv_rn(code, 16777215.0f), 1000.0f);
}

// four pixels per thread (12 bytes in, 16 out) where both pointers allow it: `quads` of them, then the scalar tail
__global__ __launch_bounds__(256) void decode_depth_kernel(const uint8_t* __restrict__ rgb, long long n, long long quads,
                                                           float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(rgb);
    for (long long q = t0; q < quads; q += stride) {
        const uint32_t a = w[3 * q], b = w[3 * q + 1], c = w[3 * q + 2];          // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        float4 o;
        o.x = depth_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
        o.y = depth_of(a >> 24, b & 255u, (b >> 8) & 255u);
        o.z = depth_of((b >> 16) & 255u, b >> 24, c & 255u);
        o.w = depth_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
        reinterpret_cast<float4*>(out)[q] = o;
    }
    for (long long p = 4 * quads + t0; p < n; p += stride) out[p] = depth_of(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
}

// ------------------------------------------------------------------------------------------------------------------ HSV
struct HsvPx {
    int h, s, v;
};

// the tables' arithmetic (thinktwice_hip.h); s saturates like the uint8 store it stands for
__device__ __forceinline__ HsvPx hsv_of(int r, int g, int b, const int* sdiv, const int* hdiv) {
    HsvPx o;
    o.v = max(r, max(g, b));
    const int diff = o.v - min(r, min(g, b));
    o.s = min(max((diff * sdiv[o.v] + 2048) >> 12, 0), 255);
    const int h0 = o.v == r ? g - b : (o.v == g ? b - r + 2 * diff : r - g + 4 * diff);
    const int h = (h0 * hdiv[diff] + 2048) >> 12;
    o.h = h < 0 ? h + 180 : h;
    return o;
}

__global__ __launch_bounds__(256) void rgb2hsv_kernel(const uint8_t* __restrict__ rgb, long long n, tt_hsv_tables tab,
                                                      uint8_t* __restrict__ hsv) {
    __shared__ int s_sdiv[256], s_hdiv[256];
    s_sdiv[threadIdx.x] = tab.sdiv[threadIdx.x];
    s_hdiv[threadIdx.x] = tab.hdiv[threadIdx.x];
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const HsvPx o = hsv_of(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], s_sdiv, s_hdiv);
        hsv[3 * p] = (uint8_t)o.h;
        hsv[3 * p + 1] = (uint8_t)o.s;
        hsv[3 * p + 2] = (uint8_t)o.v;
    }
}

// ------------------------------------------------------------------------------------------------------------ union-find
// Labels change under other threads' atomics: every read is an atomic load (never a stale cached line that would hide a
// finished union from the flatten pass's launch; within a launch an older value is only a longer way to the same root).
template <typename P>
__device__ __forceinline__ int lab_load(P* L, int i) {
    return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename P>
__device__ __forceinline__ int uf_find(P* L, int i) {
    int p = lab_load(L, i);
    while (p != i) {            // L[i] <= i: strictly decreasing until a root
        i = p;
        p = lab_load(L, i);
    }
    return i;
}

// Link the larger root under the smaller.  atomicMin returns the slot's value: if it still was the root we are done; if
// another thread linked it meanwhile (to `old` < root) the minimum keeps one of the two links and the loop goes on to unite
// the other pair, so no equivalence is lost.  Each round strictly lowers a or b.
template <typename P>
__device__ __forceinline__ void uf_union(P* L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }        // a > b
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

struct SegMapArgs {
    unsigned char class_of_tag[256];
    int light_tag;
};

struct SegGeom {
    int H, W, HW, cams;
    int tiles_x, tiles_y;
    long long rgb_sample_stride;
    long long total;            // num_images * HW
};

struct SegWork {                // the workspace's arrays, one slot per pixel of the call
    unsigned long long* sum_s;
    int* labels;
    unsigned *count, *green, *red;
};

__global__ __launch_bounds__(256) void seg_tile_kernel(const uint8_t* __restrict__ tags, SegMapArgs m, SegGeom g,
                                                       int* __restrict__ labels, float* __restrict__ out) {
    __shared__ int s_lab[kSegTH * kSegTW];
    const int tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
    const int y0 = ty * kSegTH, x0 = tx * kSegTW;
    const long long img = (long long)blockIdx.y * g.HW;
    const int lx = tid & (kSegTW - 1);
    unsigned mine = 0;          // bit k: this thread's pixel of row (tid >> 6) + 4 k is in the mask
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k, i = ly * kSegTW + lx;
        const int y = y0 + ly, x = x0 + lx;
        bool in_mask = false;
        if (y < g.H && x < g.W) {
            const long long p = img + (long long)y * g.W + x;
            const int tag = tags[p];
            in_mask = tag == m.light_tag;
            out[p] = in_mask ? 0.f : (float)m.class_of_tag[tag];
        }
        s_lab[i] = in_mask ? i : -1;
        mine |= (in_mask ? 1u : 0u) << k;
    }
    if (!__syncthreads_or((int)mine)) return;            // (also the barrier after the fill)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mine >> k) & 1u)) continue;
        const int ly = (tid >> 6) + 4 * k, i = ly * kSegTW + lx;
        if (lx > 0 && lab_load(s_lab, i - 1) >= 0) uf_union(s_lab, i, i - 1);
        if (ly > 0) {
            if (lx > 0 && lab_load(s_lab, i - kSegTW - 1) >= 0) uf_union(s_lab, i, i - kSegTW - 1);
            if (lab_load(s_lab, i - kSegTW) >= 0) uf_union(s_lab, i, i - kSegTW);
            if (lx < kSegTW - 1 && lab_load(s_lab, i - kSegTW + 1) >= 0) uf_union(s_lab, i, i - kSegTW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mine >> k) & 1u)) continue;
        const int ly = (tid >> 6) + 4 * k, i = ly * kSegTW + lx;
        const int r = uf_find(s_lab, i);
        labels[img + (long long)(y0 + ly) * g.W + x0 + lx] = (y0 + r / kSegTW) * g.W + x0 + (r & (kSegTW - 1));
    }
}

// jobs of one image: the pixels of every tile row's first line but the image's, then of every tile column's first and the
// previous tile column's last line
__global__ __launch_bounds__(256) void seg_edges_kernel(const uint8_t* __restrict__ tags, int light_tag, SegGeom g,
                                                        int jobs, int* __restrict__ labels) {
    const uint8_t* t = tags + (long long)blockIdx.y * g.HW;
    int* L = labels + (long long)blockIdx.y * g.HW;
    const int row_jobs = (g.tiles_y - 1) * g.W;
    for (int j = (int)(blockIdx.x * blockDim.x + threadIdx.x); j < jobs; j += (int)(gridDim.x * blockDim.x)) {
        int y, x;
        if (j < row_jobs) {
            y = (j / g.W + 1) * kSegTH;
            x = j % g.W;
        } else {
            const int c = (j - row_jobs) / g.H;
            y = (j - row_jobs) - c * g.H;
            x = ((c >> 1) + 1) * kSegTW - (c & 1);
        }
        const int p = y * g.W + x;
        if (t[p] != light_tag) continue;
        const int tyy = y / kSegTH, txx = x / kSegTW;
        const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qy = y + dy[k], qx = x + dx[k];
            if (qy < 0 || qx < 0 || qx >= g.W) continue;
            if (qy / kSegTH == tyy && qx / kSegTW == txx) continue;        // the tile pass united these
            const int q = qy * g.W + qx;
            if (t[q] == light_tag) uf_union(L, p, q);
        }
    }
}

// the call's pixel p -> image and pixel within it; a wave's lanes share `base`, so the loops below are wave-uniform
struct SegPixel {
    long long img0;             // first pixel of the image
    int i;                      // pixel within the image
    int n;                      // image
};

__device__ __forceinline__ SegPixel seg_pixel(const SegGeom& g, long long p) {
    SegPixel s;
    s.n = (int)(p / g.HW);
    s.img0 = (long long)s.n * g.HW;
    s.i = (int)(p - s.img0);
    return s;
}

__device__ __forceinline__ const uint8_t* seg_rgb(const SegGeom& g, const uint8_t* rgb, const SegPixel& s) {
    const int b = s.n / g.cams, c = s.n - b * g.cams;
    return rgb + (long long)b * g.rgb_sample_stride + ((long long)c * g.HW + s.i) * 3;
}

__global__ __launch_bounds__(256) void seg_flatten_kernel(const uint8_t* __restrict__ tags, int light_tag, SegGeom g, SegWork w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < g.total; p += stride) {
        if (tags[p] != light_tag) continue;
        const SegPixel s = seg_pixel(g, p);
        const int r = uf_find(w.labels + s.img0, s.i);
        w.labels[p] = r;
        if (r == s.i) {
            w.sum_s[p] = 0;
            w.count[p] = 0;
            w.green[p] = 0;
            w.red[p] = 0;
        }
    }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// One round per distinct root among the wave's active lanes: `fn(is_leader, root_slot, in_group, group_ballot)` runs on ALL
// lanes (it may reduce across the wave); the first lane of the root's group is its leader.  Called from wave-uniform code.
template <typename Fn>
__device__ __forceinline__ void for_each_root_in_wave(bool active, long long slot, Fn fn) {
    const int lane = (int)(threadIdx.x & (kWave - 1));
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long s0 = __shfl(slot, leader, kWave);
        const bool in_group = active && slot == s0;
        const unsigned long long group = __ballot(in_group);
        fn(lane == leader, s0, in_group, group);
        todo &= ~group;
    }
}

struct SegSatArgs {
    int sdiv[256];
};

__global__ __launch_bounds__(256) void seg_stats_s_kernel(const uint8_t* __restrict__ tags, int light_tag,
                                                          const uint8_t* __restrict__ rgb, SegSatArgs a, SegGeom g, SegWork w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < g.total; base += stride) {
        const long long p = base + threadIdx.x;
        const bool active = p < g.total && tags[p] == light_tag;
        long long slot = -1;
        unsigned sat = 0;
        if (active) {
            const SegPixel s = seg_pixel(g, p);
            slot = s.img0 + w.labels[p];
            const uint8_t* c = seg_rgb(g, rgb, s);
            const int r = c[0], gg = c[1], b = c[2];
            const int v = max(r, max(gg, b)), diff = v - min(r, min(gg, b));
            sat = (unsigned)min(max((diff * a.sdiv[v] + 2048) >> 12, 0), 255);
        }
        for_each_root_in_wave(active, slot, [&](bool leader, long long s0, bool in_group, unsigned long long group) {
            const unsigned sum = wave_sum(in_group ? sat : 0u);
            if (leader) {
                atomicAdd(w.count + s0, (unsigned)__popcll(group));
                atomicAdd(w.sum_s + s0, (unsigned long long)sum);
            }
        });
    }
}

struct SegHueArgs {
    int min_pixels, val_low, green_lo, green_hi, red_lo, red_hi;
    int sat_low_of_avg[256];
    tt_hsv_tables hsv;
};

__global__ __launch_bounds__(256) void seg_stats_hv_kernel(const uint8_t* __restrict__ tags, int light_tag,
                                                           const uint8_t* __restrict__ rgb, SegHueArgs a, SegGeom g, SegWork w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < g.total; base += stride) {
        const long long p = base + threadIdx.x;
        bool active = p < g.total && tags[p] == light_tag;
        long long slot = -1;
        bool green = false, red = false;
        if (active) {
            const SegPixel s = seg_pixel(g, p);
            slot = s.img0 + w.labels[p];
            const unsigned n = w.count[slot];
            active = n >= (unsigned)max(a.min_pixels, 1);          // a smaller component stays 0 whatever its colours
            if (active) {
                const int avg = (int)min(w.sum_s[slot] / n, 255ull);
                const int sat_low = a.sat_low_of_avg[avg];
                const uint8_t* c = seg_rgb(g, rgb, s);
                const HsvPx o = hsv_of(c[0], c[1], c[2], a.hsv.sdiv, a.hsv.hdiv);
                const bool lit = o.s >= sat_low && o.v >= a.val_low;
                green = lit && o.h >= a.green_lo && o.h <= a.green_hi;
                red = lit && o.h >= a.red_lo && o.h <= a.red_hi;
                active = green || red;
            }
        }
        for_each_root_in_wave(active, slot, [&](bool leader, long long s0, bool in_group, unsigned long long group) {
            const unsigned ng = (unsigned)__popcll(__ballot(in_group && green));
            const unsigned nr = (unsigned)__popcll(__ballot(in_group && red));
            if (leader) {
                if (ng) atomicAdd(w.green + s0, ng);
                if (nr) atomicAdd(w.red + s0, nr);
            }
        });
    }
}

__global__ __launch_bounds__(256) void seg_write_kernel(const uint8_t* __restrict__ tags, int light_tag, int light_base,
                                                        int min_pixels, SegGeom g, SegWork w, float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < g.total; p += stride) {
        if (tags[p] != light_tag) continue;
        const long long slot = p - (long long)(p % g.HW) + w.labels[p];
        int cls = 0;
        if (w.count[slot] >= (unsigned)max(min_pixels, 0)) {
            const unsigned ng = w.green[slot], nr = w.red[slot];
            cls = light_base + ((nr < 3 && ng < 3) ? 0 : (nr >= ng ? 1 : 2));
        }
        out[p] = (float)cls;
    }
}

static int pixel_blocks(long long n) { return (int)std::min<long long>((n + 255) / 256, kSegMaxBlocks); }

}  // namespace tt

using namespace tt;

extern "C" int tt_decode_depth_u8(const uint8_t* rgb_u8, long long n_pixels, float* out_f32, void* stream) {
    TT_REQUIRE(rgb_u8 && out_f32, "tt_decode_depth_u8: null pointer");
    TT_REQUIRE(n_pixels > 0 && n_pixels <= LLONG_MAX / 4, "tt_decode_depth_u8: %lld pixels", n_pixels);
    const bool vec = ((uintptr_t)rgb_u8 & 3) == 0 && ((uintptr_t)out_f32 & 15) == 0;
    TT_REQUIRE(((uintptr_t)out_f32 & 3) == 0, "tt_decode_depth_u8: the output must be 4-byte aligned");
    const long long quads = vec ? n_pixels / 4 : 0;
    hipLaunchKernelGGL(decode_depth_kernel, dim3(pixel_blocks(std::max(quads, n_pixels - 4 * quads))), dim3(256), 0,
                       (hipStream_t)stream, rgb_u8, n_pixels, quads, out_f32);
    return check_launch("tt_decode_depth_u8");
}

extern "C" int tt_rgb2hsv_u8(const uint8_t* rgb_u8, long long n_pixels, const tt_hsv_tables* tables, uint8_t* hsv_u8,
                             void* stream) {
    TT_REQUIRE(rgb_u8 && hsv_u8 && tables, "tt_rgb2hsv_u8: null pointer");
    TT_REQUIRE(n_pixels > 0 && n_pixels <= LLONG_MAX / 4, "tt_rgb2hsv_u8: %lld pixels", n_pixels);
    hipLaunchKernelGGL(rgb2hsv_kernel, dim3(pixel_blocks(n_pixels)), dim3(256), 0, (hipStream_t)stream, rgb_u8, n_pixels, *tables,
                       hsv_u8);
    return check_launch("tt_rgb2hsv_u8");
}

// per pixel: sum of S (8 bytes), label, count, green, red (4 bytes each)
extern "C" long long tt_decode_seg_workspace_bytes(long long num_images, int H, int W) {
    if (num_images <= 0 || H <= 0 || W <= 0 || (long long)H * W > INT_MAX || num_images > LLONG_MAX / 24 / ((long long)H * W))
        return 0;
    return num_images * H * W * 24;
}

extern "C" int tt_decode_seg_u8_phases(const uint8_t* tags_u8, int num_samples, int cams, int H, int W, const uint8_t* rgb_u8,
                                       long long rgb_sample_stride_bytes, const tt_seg_decode_conf* conf, void* workspace,
                                       long long workspace_bytes, float* out_f32, int last_phase, void* stream) {
    TT_REQUIRE(last_phase >= 0 && last_phase <= 5, "tt_decode_seg_u8: last phase %d outside 0..5", last_phase);
    TT_REQUIRE(tags_u8 && rgb_u8 && conf && workspace && out_f32, "tt_decode_seg_u8: null pointer");
    TT_REQUIRE(num_samples > 0 && cams > 0 && H > 0 && W > 0, "tt_decode_seg_u8: bad sizes %d x %d images of %d x %d", num_samples,
               cams, H, W);
    TT_REQUIRE((long long)H * W <= INT_MAX, "tt_decode_seg_u8: %d x %d pixels per image, at most 2^31 - 1", H, W);
    const long long num_images = (long long)num_samples * cams, HW = (long long)H * W;
    TT_REQUIRE(num_images <= 65535, "tt_decode_seg_u8: %lld images in one call, at most 65535", num_images);
    TT_REQUIRE(rgb_sample_stride_bytes >= cams * HW * 3, "tt_decode_seg_u8: an RGB sample stride of %lld bytes, %d images take %lld",
               rgb_sample_stride_bytes, cams, cams * HW * 3);
    TT_REQUIRE(conf->light_tag >= -1 && conf->light_tag <= 255, "tt_decode_seg_u8: traffic-light tag %d outside -1..255",
               conf->light_tag);
    TT_REQUIRE(conf->light_tag < 0 || (conf->light_base >= 0 && conf->light_base <= 253),
               "tt_decode_seg_u8: traffic-light base class %d outside 0..253", conf->light_base);
    const long long need = tt_decode_seg_workspace_bytes(num_images, H, W);
    TT_REQUIRE(need > 0 && workspace_bytes >= need, "tt_decode_seg_u8: need %lld bytes of workspace, got %lld", need, workspace_bytes);
    TT_REQUIRE(((uintptr_t)workspace & 7) == 0, "tt_decode_seg_u8: the workspace must be 8-byte aligned");

    SegGeom g;
    g.H = H; g.W = W; g.HW = (int)HW; g.cams = cams;
    g.tiles_x = div_up(W, kSegTW); g.tiles_y = div_up(H, kSegTH);
    g.rgb_sample_stride = rgb_sample_stride_bytes;
    g.total = num_images * HW;
    SegWork w;
    w.sum_s = (unsigned long long*)workspace;
    w.labels = (int*)(w.sum_s + g.total);
    w.count = (unsigned*)(w.labels + g.total);
    w.green = w.count + g.total;
    w.red = w.green + g.total;
    const long long tiles = (long long)g.tiles_x * g.tiles_y;
    TT_REQUIRE(tiles <= INT_MAX, "tt_decode_seg_u8: too many tiles");
    const int light = conf->light_tag;
    hipStream_t st = (hipStream_t)stream;

    SegMapArgs m;
    for (int i = 0; i < 256; ++i) m.class_of_tag[i] = conf->class_of_tag[i];
    m.light_tag = light;
    hipLaunchKernelGGL(seg_tile_kernel, dim3((unsigned)tiles, (unsigned)num_images), dim3(256), 0, st, tags_u8, m, g, w.labels,
                       out_f32);
    if (light >= 0 && last_phase >= 1) {
        const long long jobs = (long long)(g.tiles_y - 1) * W + 2LL * (g.tiles_x - 1) * H;         // < 2 H W / 16: an int
        if (jobs > 0)
            hipLaunchKernelGGL(seg_edges_kernel, dim3(pixel_blocks(jobs), (unsigned)num_images), dim3(256), 0, st, tags_u8, light, g,
                               (int)jobs, w.labels);
        const int blocks = pixel_blocks(g.total);
        if (last_phase >= 2) hipLaunchKernelGGL(seg_flatten_kernel, dim3(blocks), dim3(256), 0, st, tags_u8, light, g, w);
        SegSatArgs sa;
        SegHueArgs ha;
        for (int i = 0; i < 256; ++i) {
            sa.sdiv[i] = conf->hsv.sdiv[i];
            ha.sat_low_of_avg[i] = conf->sat_low_of_avg[i];
        }
        ha.hsv = conf->hsv;
        ha.min_pixels = conf->min_pixels; ha.val_low = conf->val_low;
        ha.green_lo = conf->green_lo; ha.green_hi = conf->green_hi;
        ha.red_lo = conf->red_lo; ha.red_hi = conf->red_hi;
        if (last_phase >= 3) hipLaunchKernelGGL(seg_stats_s_kernel, dim3(blocks), dim3(256), 0, st, tags_u8, light, rgb_u8, sa, g, w);
        if (last_phase >= 4) hipLaunchKernelGGL(seg_stats_hv_kernel, dim3(blocks), dim3(256), 0, st, tags_u8, light, rgb_u8, ha, g, w);
        if (last_phase >= 5)
            hipLaunchKernelGGL(seg_write_kernel, dim3(blocks), dim3(256), 0, st, tags_u8, light, conf->light_base, conf->min_pixels, g,
                               w, out_f32);
    }
    return check_launch("tt_decode_seg_u8");
}

extern "C" int tt_decode_seg_u8(const uint8_t* tags_u8, int num_samples, int cams, int H, int W, const uint8_t* rgb_u8,
                                long long rgb_sample_stride_bytes, const tt_seg_decode_conf* conf, void* workspace,
                                long long workspace_bytes, float* out_f32, void* stream) {
    return tt_decode_seg_u8_phases(tags_u8, num_samples, cams, H, W, rgb_u8, rgb_sample_stride_bytes, conf, workspace, workspace_bytes,
                                   out_f32, 5, stream);
}

// The train-mode IDA gather (IDAImageTransform(is_train=True), transform.py:248-341), stated once for preprocess.hip and
// photometric.hip: the undistorted-pixel read, the table of draws, the tap coordinates and the host check of a table.
#pragma once
#include "tt_common.h"

namespace tt {

__device__ __forceinline__ float raw_at(const uint8_t* __restrict__ img, int H, int W, int y, int x, int c) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? (float)img[((long long)y * W + x) * 3 + c] : 0.f;
}

// undistorted(Y, X, c) = grid_sample(raw, map)(Y, X): bilinear at (mapx - 0.5, mapy - 0.5), zeros outside
__device__ __forceinline__ void undist_px(const uint8_t* __restrict__ img, const float* __restrict__ mapx,
                                          const float* __restrict__ mapy, int H, int W, int Y, int X, float out[3]) {
    const float px = mapx[(long long)Y * W + X] - 0.5f;   // ((mapx-W/2)/(W/2) + 1) * W / 2 - 0.5
    const float py = mapy[(long long)Y * W + X] - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    const int x0 = (int)fx, y0 = (int)fy;
    const float lx = px - fx, ly = py - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = raw_at(img, H, W, y0, x0, c), v01 = raw_at(img, H, W, y0, x0 + 1, c);
        const float v10 = raw_at(img, H, W, y0 + 1, x0, c), v11 = raw_at(img, H, W, y0 + 1, x0 + 1, c);
        out[c] = v00 * (1.f - lx) * (1.f - ly) + v01 * lx * (1.f - ly) + v10 * (1.f - lx) * ly + v11 * lx * ly;
    }
}

// ---- train-mode pipeline: IDAImageTransform(is_train=True) (transform.py:248-341), one draw per (sample, camera) ----
// The table of draws travels in the kernel arguments (tt_ida_set of thinktwice_hip.h, TT_IDA_MAX_SETS entries at the most),
// so the entry can check every set on the host and needs neither a device buffer nor a copy.
struct IdaTable {
    tt_ida_set s[TT_IDA_MAX_SETS];
};

struct IdaArgs {
    int NI, H, W;            // raw images (frames: B*T*N, labels: B*N)
    int per_sample, N;       // images per sample (frames: T*N, labels: N) and cameras: set = (n / per_sample) * N + n % N
    int OH, OW, Cp;          // output size and padded channels
    int pixel16;             // channel-last pixels are 16 bytes and 16-byte aligned
    float mean[3], inv_std[3];
};

// The evaluation kernel's source coordinates for output pixel (oy, ox) of an image under set `p`; a flip mirrors the column.
struct IdaTaps {
    int y0, y1, x0, x1;
    float ly, lx;
};

__device__ __forceinline__ IdaTaps ida_taps(const tt_ida_set& p, int H, int W, int OW, int oy, int ox) {
    const int cx = p.flip ? OW - 1 - ox : ox;
    // F.interpolate(bilinear, align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0
    const float sy = fmaxf(((float)(oy + p.crop_y) + 0.5f) * ((float)H / (float)p.resized_h) - 0.5f, 0.f);
    const float sx = fmaxf(((float)(cx + p.crop_x) + 0.5f) * ((float)W / (float)p.resized_w) - 0.5f, 0.f);
    IdaTaps t;
    t.y0 = min((int)sy, H - 1);   // (never binds for a crop inside the resized image, which the entry requires: the map
    t.x0 = min((int)sx, W - 1);   //  is read unchecked at these coordinates)
    t.y1 = min(t.y0 + 1, H - 1);
    t.x1 = min(t.x0 + 1, W - 1);
    t.ly = sy - (float)t.y0;
    t.lx = sx - (float)t.x0;
    return t;
}

// every draw of the table against the output size, on the host, before anything is launched
static int ida_fill(const char* what, const tt_ida_set* sets, int num_sets, int out_h, int out_w, IdaTable* tab) {
    TT_REQUIRE(sets && num_sets > 0 && num_sets <= TT_IDA_MAX_SETS, "%s: need 1..%d parameter sets, got %d", what,
               TT_IDA_MAX_SETS, num_sets);
    for (int i = 0; i < num_sets; ++i) {
        const tt_ida_set& p = sets[i];
        TT_REQUIRE(p.resized_h > 0 && p.resized_w > 0, "%s: set %d: resized size %d x %d is not positive", what, i,
                   p.resized_h, p.resized_w);
        TT_REQUIRE(p.crop_y >= 0 && p.crop_x >= 0, "%s: set %d: negative crop origin (%d, %d)", what, i, p.crop_y, p.crop_x);
        // (written as subtractions: no overflow for any int crop)
        TT_REQUIRE(p.crop_y <= p.resized_h - out_h && p.crop_x <= p.resized_w - out_w,
                   "%s: set %d: crop (%d, %d) + output %d x %d leaves the resized image %d x %d", what, i, p.crop_y, p.crop_x,
                   out_h, out_w, p.resized_h, p.resized_w);
        TT_REQUIRE(p.flip == 0 || p.flip == 1, "%s: set %d: flip must be 0 or 1", what, i);
        tab->s[i] = p;
    }
    return 0;
}

}  // namespace tt

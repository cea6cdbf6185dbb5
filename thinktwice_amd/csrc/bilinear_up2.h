// Bilinear x2 upsampling with align_corners=True (nn.Upsample of UNet.unet_layer0, lss.py:267) in bf16x3 pair format: the arithmetic,
// stated once.  bilinear_up2_ac_pair_kernel (elementwise.hip) writes it to memory, conv_x3_up2_kernel (conv_x3_up2.hip) stages it as
// the operand of a 3 x 3 convolution; the two give the same bits because both call these two functions (the library is built with
// -ffp-contract=off: every product and sum below rounds on its own).
#pragma once
#include "bf16x3.h"

namespace tt {

// Where output pixel (oy, ox) of the [2 H][2 W] map reads the [H][W] source: the four source coordinates and the two weights.
struct Up2Tap {
    int y0, y1, x0, x1;
    float ly, lx;
};
__device__ __forceinline__ Up2Tap up2_tap(int H, int W, int oy, int ox) {
    const int OH = 2 * H, OW = 2 * W;
    const float sh = (OH > 1) ? (float)(H - 1) / (float)(OH - 1) : 0.f;
    const float sw = (OW > 1) ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    const float fy = sh * oy, fx = sw * ox;
    Up2Tap t;
    t.y0 = (int)fy;
    t.x0 = (int)fx;
    t.y1 = min(t.y0 + 1, H - 1);
    t.x1 = min(t.x0 + 1, W - 1);
    t.ly = fy - t.y0;
    t.lx = fx - t.x0;
    return t;
}

// Eight consecutive channels of one output pixel from their four source vectors (p00 = row y0, column x0; p01 = row y0, column x1;
// p10 / p11 = row y1), in ATen's upsample_bilinear2d operation order, split into the bf16 pair format's halves (bf16x3.h).
__device__ __forceinline__ void up2_pair8(const float* p00, const float* p01, const float* p10, const float* p11, float ly, float lx,
                                          uint4& hi, uint4& lo) {
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float4 a4 = *reinterpret_cast<const float4*>(p00 + 4 * h), b4 = *reinterpret_cast<const float4*>(p01 + 4 * h);
        const float4 c4 = *reinterpret_cast<const float4*>(p10 + 4 * h), d4 = *reinterpret_cast<const float4*>(p11 + 4 * h);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
        const float c[4] = {c4.x, c4.y, c4.z, c4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float top = (1.f - lx) * a[k] + lx * b[k];
            const float bot = (1.f - lx) * c[k] + lx * d[k];
            v[4 * h + k] = (1.f - ly) * top + ly * bot;
        }
    }
    split8(v, hi, lo);
}

}  // namespace tt

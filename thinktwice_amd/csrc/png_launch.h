// What csrc/png.hip (tt_png_decode_u8) and csrc/png_verify.hip (tt_png_decode_u8_verified) share: the workspace's layout and the
// host functions of png.hip that the verified entry calls.  The two are separate translation units so that the kernels
// tt_png_decode_u8 launches are compiled exactly as they were before the verified entry existed.
#pragma once
#include "tt_common.h"

namespace tt {

constexpr long long kPngSlotAlign = 256;

static inline __host__ __device__ long long png_expect(const tt_png_image& im) {
    return (long long)im.height * (1 + (long long)im.width * im.channels);
}
static inline __host__ __device__ long long png_slot(const tt_png_image& im) {
    return (png_expect(im) + kPngSlotAlign - 1) / kPngSlotAlign * kPngSlotAlign;
}

// the workspace offset of image `img`: the sum of the earlier slots, by the whole wave
__device__ __forceinline__ long long png_slot_offset(const tt_png_image* images, int img) {
    long long off = 0;
    for (int j = (int)threadIdx.x; j < img; j += kWave) off += png_slot(images[j]);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) off += __shfl_xor(off, o, kWave);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)off);          // the same in every lane: scalar
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)off >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// every check of the entry that needs only the table's sizes; 0 or the expected byte count (png.hip)
long long png_sizes_ok(const tt_png_image& im);
// every refusal of tt_png_decode_u8 but the workspace's size: 0, or -1 with the error text set (png.hip)
int png_check_args(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host, const tt_png_image* images_dev,
                   int num_images, void* workspace, uint8_t* out_base, long long out_bytes, int32_t* status_dev);
// tt_png_decode_u8's own launches: the plain inflate (if `inflate`), then the unfilter (png.hip)
void png_launch_unverified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_dev, int num_images,
                           uint8_t* workspace, uint8_t* out_base, int32_t* status_dev, bool inflate, hipStream_t st);

}  // namespace tt

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

// The segment table of tt_png_decode_u8_segmented, host and device copy, after png_segments.hip has checked it.
struct PngSegments {
    const tt_png_segment* host;
    const tt_png_segment* dev;
    int count;
};
// tt_png_verify_workspace_bytes plus one int32 per segment, which starts at *segment_status_at; 0 for refused tables
// (png_verify.hip)
long long png_verified_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host, int num_chunks,
                                       int verify_flags, int num_segments, long long* segment_status_at);
// tt_png_decode_u8_verified; with `seg` its inflate launch is png_launch_segmented_inflate (png_verify.hip)
int png_decode_verified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host, const tt_png_image* images_dev,
                        int num_images, const tt_png_chunk* chunks_host, const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags,
                        const PngSegments* seg, void* workspace, long long workspace_bytes, uint8_t* out_base, long long out_bytes,
                        int32_t* status_dev, int phases, void* stream);
// one workgroup per segment and one per image (its tail or its whole stream), then the statuses' fold; trailer may be null
// (png_segments.hip)
void png_launch_segmented_inflate(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_dev, int num_images,
                                  const PngSegments& seg, uint8_t* workspace, int32_t* segment_status, int32_t* status_dev,
                                  uint32_t* trailer, hipStream_t st);

}  // namespace tt

// PNG files whose zlib stream has restart points, one wave per segment (thinktwice_hip.h, tt_png_decode_u8_segmented).
//
// A stream written with a full flush after every R rows falls into SEGMENTS that inflate alone to their own rows, and a TAIL
// (one final empty block, the Adler-32); thinktwice_amd/png.py::segment_png writes such files and records the cut points.  The
// inflate launch here has one 64-lane workgroup per segment and one per image: the image's tail if it has segments, else its
// whole stream, as csrc/png.hip decodes it.  All three run png_inflate.h's inflate_span, ONE inlined copy of the decode whose
// kind is a run-time value.  Every workgroup writes one status of its own (a segment's into the workspace, an image's into
// status_dev) and a second launch, one lane per image, folds them: the image's status is that of its lowest-numbered failing
// segment, whatever order the waves ran in.  No workgroup waits for another.
//
// Stores.  A segment's rows start at first_row * (1 + W * C) of the image's slot, in general not 16-byte aligned, and the
// 16-byte groups at its two ends are shared with the neighbouring segments, which other waves write at the same time.
// inflate_span stores 16 bytes only where the whole aligned group is the span's own and bytes at the two ends
// (png_inflate.h, Output::lo, flush_full, flush_tail_owned).
//
// Trust.  The host copy of the table is checked before any launch: every segment lies inside its image's stream and the rows
// of an image tile [0, H), so every span's input and output ranges are inside the packed bytes and the image's slot.  WHAT
// the bytes hold is not trusted: a distance is checked against the segment's own output, so a wrong index or a stream cut at
// a sync flush ends in a status code and never reads another wave's rows.
#include <limits.h>

#include "tt_common.h"          // (first: png_inflate.h's barrier is the HIP runtime's)
#include "png_inflate.h"
#include "png_launch.h"

namespace tt {

// the first entry of the table (sorted by image) whose image is >= img
__device__ __forceinline__ int png_first_segment_of(const tt_png_segment* __restrict__ segs, int num_segs, int img) {
    int lo = 0, hi = num_segs;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (segs[mid].image < img) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void png_inflate_segments_kernel(const uint8_t* __restrict__ packed, long long packed_bytes,
                                                                  const tt_png_image* __restrict__ images,
                                                                  const tt_png_segment* __restrict__ segs, int num_segs,
                                                                  uint8_t* __restrict__ ws, int32_t* __restrict__ seg_status,
                                                                  int32_t* __restrict__ status, uint32_t* __restrict__ trailer) {
    __shared__ tt_png::SegmentState S;                           // four workgroups per CU (png_inflate.h)
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const bool is_seg = b < num_segs;
    const int img = is_seg ? segs[b].image : b - num_segs;
    const tt_png_image im = images[img];
    const long long stride = 1 + (long long)im.width * im.channels;
    const long long stream_end = im.stream_offset + im.stream_bytes;

    tt_png::Span J;
    long long at, bytes;                                         // the span's bytes of `packed`
    J.slot = ws + png_slot_offset(images, img);
    if (is_seg) {
        const tt_png_segment s = segs[b];
        at = s.offset;
        bytes = s.bytes;
        J.kind = tt_png::kSpanSegment;
        J.slot_pos = s.first_row * stride;
        J.expect = (int)(s.rows * stride);
    } else {
        const int first = png_first_segment_of(segs, num_segs, img), end = png_first_segment_of(segs, num_segs, img + 1);
        J.slot_pos = 0;
        if (end > first) {                                       // the tail: what follows the image's last segment
            at = segs[end - 1].offset + segs[end - 1].bytes;
            bytes = stream_end - at;
            J.kind = tt_png::kSpanTail;
            J.expect = 0;
        } else {
            at = im.stream_offset;
            bytes = im.stream_bytes;
            J.kind = tt_png::kSpanZlib;
            J.expect = (int)png_expect(im);
        }
    }
    int st = TT_PNG_OK;
    J.window = tt_png::kWindow;
    if (J.kind != tt_png::kSpanZlib) {                           // the stream's header, as inflate_zlib reads it
        const uint32_t cmf = packed[im.stream_offset], flg = packed[im.stream_offset + 1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) st = TT_PNG_BAD_ZLIB_HEADER;
        else J.window = 1 << ((int)(cmf >> 4) + 8);
    }
    st = tt_png::uniform(st);
    if (st == TT_PNG_OK) {
        const int skew = (int)(at & 3);                          // `packed` is 16-byte aligned: read from the word the span starts in
        const long long word0 = at - skew;
        J.base = packed + word0;
        J.limit = packed_bytes - word0;
        J.start = skew;
        J.end = skew + (int)bytes;
        st = tt_png::inflate_span(S, J, lane, kWave, (!is_seg && trailer) ? trailer + img : nullptr);
    }
    if (lane == 0) {
        if (is_seg) seg_status[b] = st;
        else status[img] = st;
    }
}

// One lane per image: the status of its lowest-numbered failing segment, else what its tail (or whole stream) left.
__global__ __launch_bounds__(256) void png_segment_status_kernel(const tt_png_segment* __restrict__ segs, int num_segs,
                                                                 const int32_t* __restrict__ seg_status, int num_images,
                                                                 int32_t* __restrict__ status) {
    const int img = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (img >= num_images) return;
    const int first = png_first_segment_of(segs, num_segs, img), end = png_first_segment_of(segs, num_segs, img + 1);
    for (int j = first; j < end; ++j) {
        const int st = seg_status[j];
        if (st != TT_PNG_OK) {
            status[img] = st;
            return;
        }
    }
}

// every refusal of the segment table: 0, or -1 with the error text set.  images_host has passed png_check_args.
static int png_check_segments(const tt_png_image* images_host, int num_images, const tt_png_segment* segs_host,
                              const tt_png_segment* segs_dev, int num_segs, bool need_dev) {
    TT_REQUIRE(num_segs >= 0 && num_segs <= TT_PNG_MAX_SEGMENTS, "tt_png_decode_u8_segmented: %d segments, 0..%d", num_segs,
               TT_PNG_MAX_SEGMENTS);
    if (num_segs == 0) return 0;
    TT_REQUIRE(segs_host && (!need_dev || (segs_dev && ((uintptr_t)segs_dev & 7) == 0)),
               "tt_png_decode_u8_segmented: %d segments need the host table and the device's, 8-byte aligned", num_segs);
    int img = -1, next_row = 0;
    long long at = 0;                                            // where the next segment of image `img` must start
    const auto close_image = [&](int j) {
        const tt_png_image& im = images_host[img];
        TT_REQUIRE(next_row == im.height, "tt_png_decode_u8_segmented: the segments of image %d end at row %d of %d (before entry %d): "
                   "they must tile [0, H)", img, next_row, im.height, j);
        return 0;
    };
    for (int j = 0; j < num_segs; ++j) {
        const tt_png_segment& s = segs_host[j];
        TT_REQUIRE(s.image >= 0 && s.image < num_images, "tt_png_decode_u8_segmented: segment %d belongs to image %d of %d", j, s.image,
                   num_images);
        TT_REQUIRE(s.image >= img, "tt_png_decode_u8_segmented: segment %d of image %d follows image %d's: the table lists the images "
                   "in increasing order", j, s.image, img);
        if (s.image != img) {
            if (img >= 0 && close_image(j)) return -1;
            img = s.image;
            next_row = 0;
            at = images_host[img].stream_offset + 2;
            TT_REQUIRE(png_expect(images_host[img]) <= INT_MAX - 16, "tt_png_decode_u8_segmented: image %d has more than 2^31 - 17 "
                       "scanline bytes", img);
        }
        const tt_png_image& im = images_host[img];
        TT_REQUIRE(s.rows >= 1 && s.first_row == next_row && s.rows <= im.height - next_row,
                   "tt_png_decode_u8_segmented: segment %d: rows [%d, +%d) of image %d, whose next row is %d of %d: an image's segments "
                   "are in row order and tile [0, H)", j, s.first_row, s.rows, img, next_row, im.height);
        TT_REQUIRE(s.bytes >= 1 && s.offset == at && s.bytes <= im.stream_offset + im.stream_bytes - 6 - at,
                   "tt_png_decode_u8_segmented: segment %d: [%lld, +%lld) is empty, does not continue image %d's stream "
                   "at byte %lld, or leaves fewer than 6 of its bytes (to %lld) for the tail", j, s.offset, s.bytes, img, at,
                   im.stream_offset + im.stream_bytes);
        next_row += s.rows;
        at += s.bytes;
    }
    return close_image(num_segs);
}

void png_launch_segmented_inflate(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_dev, int num_images,
                                  const PngSegments& seg, uint8_t* workspace, int32_t* segment_status, int32_t* status_dev,
                                  uint32_t* trailer, hipStream_t st) {
    hipLaunchKernelGGL(png_inflate_segments_kernel, dim3((unsigned)(seg.count + num_images)), dim3(kWave), 0, st, packed_dev, packed_bytes,
                       images_dev, seg.dev, seg.count, workspace, segment_status, status_dev, trailer);
    if (seg.count > 0)
        hipLaunchKernelGGL(png_segment_status_kernel, dim3((unsigned)div_up(num_images, 256)), dim3(256), 0, st, seg.dev, seg.count,
                           (const int32_t*)segment_status, num_images, status_dev);
}

}  // namespace tt

using namespace tt;

extern "C" long long tt_png_segmented_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host,
                                                      int num_chunks, int verify_flags, const tt_png_segment* segments_host,
                                                      int num_segments) {
    if (tt_png_workspace_bytes(images_host, num_images) <= 0) return 0;
    for (int i = 0; i < num_images; ++i)                         // (the stream ranges png_check_segments reads)
        if (images_host[i].stream_bytes < 6 || images_host[i].stream_offset < 0) return 0;
    if (png_check_segments(images_host, num_images, segments_host, nullptr, num_segments, false)) return 0;
    return png_verified_workspace_bytes(images_host, num_images, chunks_host, num_chunks, verify_flags, num_segments, nullptr);
}

extern "C" int tt_png_decode_u8_segmented_phases(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                                 const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                                                 const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags,
                                                 const tt_png_segment* segments_host, const tt_png_segment* segments_dev,
                                                 int num_segments, void* workspace, long long workspace_bytes, uint8_t* out_base,
                                                 long long out_bytes, int32_t* status_dev, int phases, void* stream) {
    TT_REQUIRE(phases == 1 || phases == 2, "tt_png_decode_u8_segmented: %d phases, 1 or 2", phases);
    if (png_check_args(packed_dev, packed_bytes, images_host, images_dev, num_images, workspace, out_base, out_bytes, status_dev))
        return -1;
    if (png_check_segments(images_host, num_images, segments_host, segments_dev, num_segments, true)) return -1;
    const PngSegments seg{segments_host, segments_dev, num_segments};
    return png_decode_verified(packed_dev, packed_bytes, images_host, images_dev, num_images, chunks_host, chunks_dev, num_chunks,
                               verify_flags, &seg, workspace, workspace_bytes, out_base, out_bytes, status_dev, phases, stream);
}

extern "C" int tt_png_decode_u8_segmented(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                          const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                                          const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags,
                                          const tt_png_segment* segments_host, const tt_png_segment* segments_dev, int num_segments,
                                          void* workspace, long long workspace_bytes, uint8_t* out_base, long long out_bytes,
                                          int32_t* status_dev, void* stream) {
    return tt_png_decode_u8_segmented_phases(packed_dev, packed_bytes, images_host, images_dev, num_images, chunks_host, chunks_dev,
                                             num_chunks, verify_flags, segments_host, segments_dev, num_segments, workspace,
                                             workspace_bytes, out_base, out_bytes, status_dev, 2, stream);
}

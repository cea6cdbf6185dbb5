// The HIP side of file_slots.h, shared by png_encode.hip and jpeg_encode.hip: the refusals of a table that both entries make
// before any launch, and the device call behind their compaction kernels.
#pragma once
#include "tt_common.h"
#include "file_slots.h"

namespace tt {

// Every refusal of tt_<format>_encode_u8 that does not depend on the totals, in the entry's order; per image the format's own
// checks come first (image_check: 0, or -1 with the error set).  `bound_entry` names the bound in the text.
template <class F>
static int check_file_table(const char* entry, const char* bound_entry, const uint8_t* pixels_dev, long long pixel_bytes,
                            const typename F::Image* images_host, const typename F::Image* images_dev, int num_images, void* workspace,
                            uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev,
                            int (*image_check)(const typename F::Image&, int)) {
    TT_REQUIRE(pixels_dev && images_host && images_dev && workspace && files_dev && file_sizes_dev, "%s: null pointer", entry);
    TT_REQUIRE(num_images >= 1 && num_images <= TT_PNG_MAX_IMAGES, "%s: %d images, 1..%d", entry, num_images, TT_PNG_MAX_IMAGES);
    TT_REQUIRE(((uintptr_t)images_dev & 7) == 0 && ((uintptr_t)files_dev & 3) == 0 && ((uintptr_t)file_sizes_dev & 7) == 0 &&
                   ((uintptr_t)workspace & (tt_slots::kAlign - 1)) == 0,
               "%s: misaligned table, files, file sizes or workspace (8, 4, 8, 256 bytes)", entry);
    TT_REQUIRE(pixel_bytes >= 0 && files_bytes >= 0, "%s: %lld pixel bytes, %lld file bytes", entry, pixel_bytes, files_bytes);
    for (int i = 0; i < num_images; ++i) {
        const typename F::Image& im = images_host[i];
        if (image_check(im, i)) return -1;
        const long long bound = F::bound(im);
        const long long image = (long long)im.height * im.width * im.channels;
        TT_REQUIRE(im.pixel_offset >= 0 && im.pixel_offset <= pixel_bytes && image <= pixel_bytes - im.pixel_offset,
                   "%s: image %d: pixels [%lld, +%lld) outside the %lld pixel bytes", entry, i, im.pixel_offset, image, pixel_bytes);
        TT_REQUIRE((im.file_offset & 3) == 0, "%s: image %d: file_offset %lld is not a multiple of 4", entry, i, im.file_offset);
        TT_REQUIRE(im.file_capacity >= bound, "%s: image %d: a slot of %lld bytes, %s is %lld", entry, i, im.file_capacity, bound_entry, bound);
        TT_REQUIRE(im.file_offset >= 0 && im.file_offset <= files_bytes && im.file_capacity <= files_bytes - im.file_offset,
                   "%s: image %d: slot [%lld, +%lld) outside the %lld file bytes", entry, i, im.file_offset, im.file_capacity, files_bytes);
        for (int j = 0; j < i; ++j)
            TT_REQUIRE(im.file_offset >= images_host[j].file_offset + images_host[j].file_capacity ||
                           images_host[j].file_offset >= im.file_offset + im.file_capacity,
                       "%s: the slots of images %d and %d overlap", entry, j, i);
    }
    return 0;
}

using tt_slots::kCopyLanes;
template <class F>
static __device__ __forceinline__ void compact_block(const typename F::Image* images, int num_images, const uint8_t* ws, const int32_t* sizes,
                                                     const long long* part_at, uint8_t* files) {
    struct { __device__ operator long long() const { return threadIdx.x; } } lane;      // (read where the copy loop starts)
    tt_slots::compact_part<F>(images, num_images, blockIdx.x, ws, sizes, part_at, files, lane, kCopyLanes);
}

}  // namespace tt

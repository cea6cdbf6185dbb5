// The slot table of the device file encoders, written once, as plain functions without a HIP type: png_encode.hip and
// jpeg_encode.hip compile them as device code, the host checkers under tools/ as host C++, over a table of several images.
// An encoder runs a FIRST PASS over units of an image (PNG: the filter, a row; JPEG: the transform, 64 blocks) and then codes
// PARTS of it (segments; restart intervals), each into a worst-case slot.  The workspace: the images' regions, then `sizes`
// (int32 per part: what the coder wrote) and `part_at` (int64 per part: where the part goes in its file).
// A format description F (tt_pngenc::SlotFormat, tt_jpeg::SlotFormat), through which alone the image structs are read, names
// F::Image (pixel_offset, file_offset, file_capacity and the format's parameters), F::Geom and F::geom(im), F::units(im, g)
// (int or long long) and F::parts(g) (int >= 1), F::first_bytes(g), F::slot_bytes(im, g, last) and F::bound(im) (0: refused).
#pragma once
#include <stdint.h>

#include "../../include/thinktwice_hip.h"
#include "lanes.h"          // TT_HD

namespace tt_slots {

constexpr long long kAlign = 256;
TT_HD inline long long up(long long n) { return (n + kAlign - 1) / kAlign * kAlign; }

// One image's part of the workspace, [first-pass output | one slot per part], each half rounded up to 256 bytes.
template <class F>
struct Region {
    typename F::Geom g;
    long long slot_full, slot_last;     // the slot of a full part, of the last
    long long slots_at, bytes;          // where the first slot starts (the first pass's output comes first), the region's bytes
};

template <class F>
TT_HD inline Region<F> region(const typename F::Image& im) {
    Region<F> r;
    r.g = F::geom(im);
    r.slot_full = F::slot_bytes(im, r.g, false);
    r.slot_last = F::slot_bytes(im, r.g, true);
    r.slots_at = up(F::first_bytes(r.g));
    r.bytes = r.slots_at + up((F::parts(r.g) - 1) * r.slot_full + r.slot_last);
    return r;
}

// Part k of the region that starts at `base`: its slot, and the slot's bytes.
template <class F, class P>
TT_HD inline P slot_at(P base, const Region<F>& r, long long k) { return base + r.slots_at + k * r.slot_full; }
template <class F>
TT_HD inline long long slot_cap(const Region<F>& r, long long k) { return k == F::parts(r.g) - 1 ? r.slot_last : r.slot_full; }

// Where an image, or the image of a unit or of a part, lies: the running sums over the table; image = -1 past its last.
struct Where {
    int image;
    long long region_at;                // of the image's region in the workspace
    long long first_part, local;        // the image's first entry in sizes / part_at, the unit or part within the image
};

enum { kByImage = 0, kByUnit = 1, kByPart = 2 };
template <class F>
TT_HD inline Where find(const typename F::Image* images, int num_images, int by, long long index) {
    Where w{0, 0, 0, 0};
    long long count = 0;
    for (int i = 0; i < num_images; ++i) {
        const Region<F> r = region<F>(images[i]);
        const long long mine = by == kByImage ? 1 : by == kByUnit ? F::units(images[i], r.g) : F::parts(r.g);
        if (index < count + mine) {
            w.image = i;
            w.local = index - count;
            return w;
        }
        count += mine;
        w.region_at += r.bytes;
        w.first_part += F::parts(r.g);
    }
    w.image = -1;
    return w;
}

constexpr int kCopyLanes = 256;         // lanes of the compaction's workgroup, one workgroup per part of the table
// The compaction of part `part`, lane `lane` of `nlanes` (an int, or what becomes the lane's index at the copy loop): sizes[part]
// bytes of its slot go to part_at[part] in the file.  A size above the slot is clamped; a negative one or a place outside copies nothing.
template <class F, class Lane>
TT_HD inline void compact_part(const typename F::Image* images, int num_images, long long part, const uint8_t* ws, const int32_t* sizes,
                               const long long* part_at, uint8_t* files, Lane lane, int nlanes) {
    const Where w = find<F>(images, num_images, kByPart, part);
    if (w.image < 0) return;
    const typename F::Image im = images[w.image];
    const Region<F> r = region<F>(im);
    const long long cap = slot_cap(r, w.local);
    long long n = sizes[part];
    if (n > cap) n = cap;
    const long long at = part_at[part];
    if (n < 0 || at < 0 || at > im.file_capacity - n) return;
    const uint8_t* src = slot_at(ws + w.region_at, r, w.local);
    uint8_t* dst = files + im.file_offset + at;
    for (long long i = lane; i < n; i += nlanes) dst[i] = src[i];
}

// The sums over a table and the tail of the workspace.  A format with more tables (PNG's checksums) appends them at `end`.
struct Totals {
    long long units, parts, regions;    // of all images: first-pass units, parts, bytes of the regions
    long long sizes, part_at, end;      // offsets in the workspace
};

// The sum of the images' bounds; 0 where the table is refused: null, a bad count, an image without a bound.
template <class F>
inline long long bound_sum(const typename F::Image* images, int num_images) {
    if (!images || num_images < 1 || num_images > TT_PNG_MAX_IMAGES) return 0;
    long long total = 0;
    for (int i = 0; i < num_images; ++i) {
        const long long bound = F::bound(images[i]);
        if (!bound) return 0;
        total += bound;
    }
    return total;
}

// false where the table is refused: no bound_sum, or more than INT_MAX units or parts
template <class F>
inline bool totals(const typename F::Image* images, int num_images, Totals& T) {
    T = Totals{};
    if (!bound_sum<F>(images, num_images)) return false;
    for (int i = 0; i < num_images; ++i) {
        const Region<F> r = region<F>(images[i]);
        T.units += F::units(images[i], r.g);
        T.parts += F::parts(r.g);
        T.regions += r.bytes;
    }
    if (T.units > 2147483647LL || T.parts > 2147483647LL) return false;
    T.sizes = T.regions;
    T.part_at = T.sizes + up(4 * T.parts);
    T.end = T.part_at + up(8 * T.parts);
    return true;
}

}  // namespace tt_slots

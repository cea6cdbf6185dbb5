// Stand-alone checker of thinktwice_amd/csrc/jpeg_core.h and csrc/file_slots.h on the CPU: the same source the device kernels
// run, with one thread playing the lanes, over the case file tests/jpeg_encode_cases.py::write_case_file writes.  Every case is
// encoded to a complete JPEG file (the bytes tt_jpeg_encode_u8 writes) the way the device does it: every block transformed on
// its own, every restart interval coded into its own slot, the header, then the intervals copied behind it.  Then all cases are
// encoded once more as ONE table, the way tt_jpeg_encode_u8 lays it out: one workspace and one file buffer, every block group
// and every interval located through file_slots.h's find, the intervals compacted by its compaction body; every file must
// equal the case's own.  Every buffer is a heap block of the exact size between two runs of guard bytes: a build with
// -fsanitize=address,undefined sees any access outside the pixels, the coefficients, an interval's slot, the workspace or the
// files, and the guards are checked for a stray write that stays inside the heap block.
//
//   jpeg_encode_host_check <case file> <output directory>
//       writes <output directory>/<case index>.jpg and prints per case "ok   <name>: bytes B intervals N bound M", then
//       "batch: N images, U units, P parts, W workspace bytes: ok|FAIL"; exit 0 if every case stayed inside its bounds and its
//       guards and the batch equals the cases
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/jpeg_core.h"
#include "../thinktwice_amd/csrc/file_slots.h"

namespace jpg = tt_jpeg;
namespace slots = tt_slots;
using Fmt = jpg::SlotFormat;

constexpr int kGuard = 64;
constexpr uint8_t kGuardByte = 0xA5;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint8_t* guarded(long long n) {
    uint8_t* p = (uint8_t*)malloc((size_t)n + 2 * kGuard);
    memset(p, kGuardByte, (size_t)n + 2 * kGuard);
    return p + kGuard;
}
static bool guards_ok(const uint8_t* p, long long n) {
    for (int i = 0; i < kGuard; ++i)
        if (p[-1 - i] != kGuardByte || p[n + i] != kGuardByte) return false;
    return true;
}
static void release(uint8_t* p) { free(p - kGuard); }

struct Case {
    tt_jpeg_enc_image im;
    std::vector<uint8_t> pixels, file;
};

// All cases as one table.  Prints the batch line; true where every file equals the case's own and every guard is intact.
static bool batch(std::vector<Case>& cases, jpg::State& S, const jpg::Lanes L) {
    const int n = (int)cases.size();
    std::vector<tt_jpeg_enc_image> images((size_t)n);
    long long pixel_bytes = 0, files_bytes = 0;
    for (int i = 0; i < n; ++i) {
        images[(size_t)i] = cases[(size_t)i].im;
        images[(size_t)i].pixel_offset = pixel_bytes;
        images[(size_t)i].file_offset = files_bytes;
        images[(size_t)i].file_capacity = Fmt::bound(images[(size_t)i]);
        pixel_bytes += (long long)cases[(size_t)i].pixels.size();
        files_bytes += images[(size_t)i].file_capacity;
    }
    slots::Totals T;
    bool ok = slots::totals<Fmt>(images.data(), n, T) && files_bytes == slots::bound_sum<Fmt>(images.data(), n);
    if (!ok) {
        printf("batch: %d images: the table is refused: FAIL\n", n);
        return false;
    }
    uint8_t* pixels = guarded(pixel_bytes);
    for (int i = 0; i < n; ++i) memcpy(pixels + images[(size_t)i].pixel_offset, cases[(size_t)i].pixels.data(), cases[(size_t)i].pixels.size());
    uint8_t* ws = guarded(T.end);
    uint8_t* files = guarded(files_bytes);
    int32_t* sizes = (int32_t*)(ws + T.sizes);
    long long* int_at = (long long*)(ws + T.part_at);

    for (long long u = 0; u < T.units; ++u) {                     // jpeg_transform_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByUnit, u);
        const tt_jpeg_enc_image& im = images[(size_t)w.image];
        const jpg::Geom g = Fmt::geom(im);
        uint16_t q[128];
        jpg::fill_quant(q, im.quality, L);
        for (long long b = w.local * jpg::kLanes; b < (w.local + 1) * jpg::kLanes && b < g.blocks; ++b)
            jpg::transform_block(pixels + im.pixel_offset, im.height, im.width, g, b, q, reinterpret_cast<int16_t*>(ws + w.region_at + b * 128));
    }
    for (long long p = 0; p < T.parts; ++p) {                     // jpeg_entropy_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByPart, p);
        const tt_jpeg_enc_image& im = images[(size_t)w.image];
        const slots::Region<Fmt> r = slots::region<Fmt>(im);
        const int k = (int)w.local;
        const int16_t* coefs = reinterpret_cast<const int16_t*>(ws + w.region_at) + jpg::interval_first_block(r.g, im.restart_rows, k) * 64;
        sizes[p] = (int32_t)jpg::encode_interval(S, coefs, jpg::interval_blocks(r.g, im.restart_rows, k), r.g.bpm,
                                                 slots::slot_at(ws + w.region_at, r, k), slots::slot_cap(r, k), k == r.g.nint - 1 ? jpg::kEoi : jpg::kRst0 + (k & 7), L);
    }
    std::vector<long long> file_sizes((size_t)n);
    for (int i = 0; i < n; ++i) {                                 // jpeg_layout_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByImage, i);
        const tt_jpeg_enc_image& im = images[(size_t)i];
        const jpg::Geom g = Fmt::geom(im);
        long long at = jpg::write_header(files + im.file_offset, im.height, im.width, im.quality, g);
        for (int k = 0; k < g.nint; ++k) {
            int_at[w.first_part + k] = at;
            at += sizes[w.first_part + k];
        }
        file_sizes[(size_t)i] = at;
    }
    for (long long p = 0; p < T.parts; ++p)                       // jpeg_compact_kernel
        for (int lane = 0; lane < slots::kCopyLanes; ++lane) slots::compact_part<Fmt>(images.data(), n, p, ws, sizes, int_at, files, lane, slots::kCopyLanes);
    for (int i = 0; i < n; ++i) {
        const std::vector<uint8_t>& want = cases[(size_t)i].file;
        ok = ok && file_sizes[(size_t)i] == (long long)want.size() && memcmp(files + images[(size_t)i].file_offset, want.data(), want.size()) == 0;
    }
    ok = ok && slots::find<Fmt>(images.data(), n, slots::kByImage, n).image == -1 &&
         slots::find<Fmt>(images.data(), n, slots::kByUnit, T.units).image == -1 && slots::find<Fmt>(images.data(), n, slots::kByPart, T.parts).image == -1;
    ok = ok && guards_ok(pixels, pixel_bytes) && guards_ok(ws, T.end) && guards_ok(files, files_bytes);
    printf("batch: %d images, %lld units, %lld parts, %lld workspace bytes: %s\n", n, T.units, T.parts, T.end, ok ? "ok" : "FAIL");
    release(pixels);
    release(ws);
    release(files);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case file> <output directory>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTJPGE01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    jpg::State* S = new jpg::State;
    const jpg::Lanes L{0, jpg::kLanes};
    std::vector<Case> cases;
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, p[6];
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, p, 24)) return 2;
        const int H = p[0], W = p[1], C = p[2], quality = p[3], sub = p[4], rr = p[5];
        cases.emplace_back();
        Case& c = cases.back();
        c.im = tt_jpeg_enc_image{0, 0, 0, W, H, C, quality, sub, rr, 0, 0};
        const long long bound = Fmt::bound(c.im);
        if (!bound) return 2;
        const slots::Region<Fmt> r = slots::region<Fmt>(c.im);
        const jpg::Geom& g = r.g;
        const long long image = (long long)H * W * C;
        c.pixels.resize((size_t)image);
        uint8_t* pixels = guarded(image);
        if (!read_exact(f, pixels, (size_t)image)) return 2;
        memcpy(c.pixels.data(), pixels, (size_t)image);

        uint16_t q[128];
        jpg::fill_quant(q, quality, L);
        uint8_t* coef_bytes = guarded(g.blocks * 128);
        int16_t* coefs = (int16_t*)coef_bytes;
        for (long long b = 0; b < g.blocks; ++b) jpg::transform_block(pixels, H, W, g, b, q, coefs + b * 64);

        std::vector<uint8_t*> slot_at((size_t)g.nint);
        std::vector<long long> sizes((size_t)g.nint);
        long long total = 0;
        bool ok = true;
        for (int k = 0; k < g.nint; ++k) {
            const long long n = jpg::interval_blocks(g, rr, k), cap = slots::slot_cap(r, k);
            slot_at[(size_t)k] = guarded(cap);
            const long long got = jpg::encode_interval(*S, coefs + jpg::interval_first_block(g, rr, k) * 64, n, g.bpm, slot_at[(size_t)k], cap,
                                                       k == g.nint - 1 ? jpg::kEoi : jpg::kRst0 + (k & 7), L);
            ok = ok && got >= 2 && got <= jpg::interval_bound(n) && guards_ok(slot_at[(size_t)k], cap);
            sizes[(size_t)k] = got;
            total += got;
        }
        const long long bytes = g.header + total;
        ok = ok && bytes <= bound && guards_ok(pixels, image) && guards_ok(coef_bytes, g.blocks * 128);
        uint8_t* file = guarded(bytes);
        ok = ok && jpg::write_header(file, H, W, quality, g) == g.header;
        long long at = g.header;
        for (int k = 0; k < g.nint; ++k) {
            memcpy(file + at, slot_at[(size_t)k], (size_t)sizes[(size_t)k]);
            at += sizes[(size_t)k];
        }
        ok = ok && guards_ok(file, bytes);
        c.file.assign(file, file + bytes);
        const std::string path = std::string(argv[2]) + "/" + std::to_string(i) + ".jpg";
        FILE* o = fopen(path.c_str(), "wb");
        if (!o || fwrite(file, 1, (size_t)bytes, o) != (size_t)bytes) return 2;
        fclose(o);
        printf("%s %s: bytes %lld intervals %d bound %lld header %d\n", ok ? "ok  " : "FAIL", name.c_str(), bytes, g.nint, bound, g.header);
        failed += ok ? 0 : 1;
        for (uint8_t* s : slot_at) release(s);
        release(pixels);
        release(coef_bytes);
        release(file);
    }
    fclose(f);
    if (count > 0) failed += batch(cases, *S, L) ? 0 : 1;
    delete S;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}

// Stand-alone checker of thinktwice_amd/csrc/png_deflate.h and csrc/file_slots.h on the CPU: the same source the device kernels
// run, with one thread playing the lanes, over the case file tests/png_encode_cases.py::write_case_file writes.  Every case is
// encoded to a complete PNG file (the bytes tt_png_encode_u8 writes), then inflated again by the host build of png_inflate.h --
// the whole stream, and every segment alone at the offsets of the file's own ttSG chunk -- unfiltered and compared with the
// pixels.  Then all cases are encoded once more as ONE table, the way tt_png_encode_u8 lays it out: one workspace and one file
// buffer, every row and every segment located through file_slots.h's find, the segments compacted by its compaction body; every
// file must equal the case's own.  Every buffer is a heap block of the exact size between two runs of guard bytes, so a build
// with -fsanitize=address,undefined sees any access outside the pixels, the scanlines, a segment's slot, the workspace or the
// files, and the guards show a stray write that stays inside the heap block.
//
//   png_encode_host_check <case file> <output directory>
//       writes <output directory>/<case index>.png and prints per case
//       "ok   <name>: bytes B dynamic D stored S limited L" (blocks written as dynamic, as stored, and blocks whose code
//       lengths the 15 / 7 bit limit changed), then "batch: N images, U units, P parts, W workspace bytes: ok|FAIL"; exit 0 if
//       every round trip is clean and the batch equals the cases
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/png_deflate.h"
#include "../thinktwice_amd/csrc/png_checksum.h"
#include "../thinktwice_amd/csrc/file_slots.h"

namespace enc = tt_pngenc;
namespace slots = tt_slots;
using Fmt = enc::SlotFormat;

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

static uint32_t crc32_of(const uint8_t* p, long long n) {
    uint32_t c = ~0u;
    for (long long i = 0; i < n; ++i) c = tt_cksum::crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
    return ~c;
}

static uint32_t adler32_of(const uint8_t* p, long long n) {
    uint32_t a = 1, b = 0;
    for (long long i = 0; i < n; ++i) {
        a = (a + p[i]) % tt_cksum::kBase;
        b = (b + a) % tt_cksum::kBase;
    }
    return (b << 16) | a;
}

// the Adler-32 of the scanlines and the three CRC-32 fields of a file whose segments are in place
static void write_checksums(uint8_t* file, const enc::FileGeom& g, long long payload, const uint8_t* lines) {
    uint8_t* idat = file + g.idat_at;
    enc::put_be32(idat + 8 + payload - 4, adler32_of(lines, g.expect));
    enc::put_be32(file + 29, crc32_of(file + 12, 17));
    enc::put_be32(file + g.idat_at - 4, crc32_of(file + enc::kTtsgAt + 4, g.idat_at - 4 - (enc::kTtsgAt + 4)));
    enc::put_be32(idat + 8 + payload, crc32_of(idat + 4, 4 + payload));
}

struct Case {
    tt_png_enc_image im;
    std::vector<uint8_t> pixels, file;
};

// All cases as one table.  Prints the batch line; true where every file equals the case's own and every guard is intact.
static bool batch(std::vector<Case>& cases, enc::State& S, enc::FilterState& F, const enc::Lanes L) {
    const int n = (int)cases.size();
    std::vector<tt_png_enc_image> images((size_t)n);
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
    long long* seg_at = (long long*)(ws + T.part_at);

    for (long long u = 0; u < T.units; ++u) {                     // png_filter_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByUnit, u);
        const tt_png_enc_image& im = images[(size_t)w.image];
        const long long row = (long long)im.width * im.channels;
        const uint8_t* cur = pixels + im.pixel_offset + w.local * row;
        enc::filter_row(F, cur, w.local ? cur - row : nullptr, (int)row, im.channels, im.filter, ws + w.region_at + w.local * (row + 1), L);
    }
    for (long long p = 0; p < T.parts; ++p) {                     // png_deflate_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByPart, p);
        const tt_png_enc_image& im = images[(size_t)w.image];
        const slots::Region<Fmt> r = slots::region<Fmt>(im);
        enc::Stats st;
        sizes[p] = (int32_t)enc::deflate_segment(S, ws + w.region_at + w.local * r.g.n_full, (int)(w.local == r.g.nseg - 1 ? r.g.n_last : r.g.n_full),
                                                 slots::slot_at(ws + w.region_at, r, w.local), slots::slot_cap(r, w.local), L, st);
    }
    std::vector<long long> file_sizes((size_t)n);
    for (int i = 0; i < n; ++i) {                                 // png_layout_kernel
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByImage, i);
        const tt_png_enc_image& im = images[(size_t)i];
        file_sizes[(size_t)i] = enc::write_container(files + im.file_offset, im.height, im.width, im.channels, im.rows_per_segment, Fmt::geom(im),
                                                     sizes + w.first_part, seg_at + w.first_part);
    }
    for (long long p = 0; p < T.parts; ++p)                       // png_compact_kernel
        for (int lane = 0; lane < slots::kCopyLanes; ++lane) slots::compact_part<Fmt>(images.data(), n, p, ws, sizes, seg_at, files, lane, slots::kCopyLanes);
    for (int i = 0; i < n; ++i) {
        const tt_png_enc_image& im = images[(size_t)i];
        const enc::FileGeom g = Fmt::geom(im);
        const slots::Where w = slots::find<Fmt>(images.data(), n, slots::kByImage, i);
        write_checksums(files + im.file_offset, g, file_sizes[(size_t)i] - g.idat_at - 12 - 12, ws + w.region_at);
        const std::vector<uint8_t>& want = cases[(size_t)i].file;
        ok = ok && file_sizes[(size_t)i] == (long long)want.size() && memcmp(files + im.file_offset, want.data(), want.size()) == 0;
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
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTPNGE01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    enc::State* S = new enc::State;
    enc::FilterState* F = new enc::FilterState;
    tt_png::State* D = new tt_png::State;
    const enc::Lanes L{0, enc::kLanes};
    std::vector<Case> cases;
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, p[5];
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, p, 20)) return 2;
        const int H = p[0], W = p[1], C = p[2], R = p[3], mode = p[4];
        if (H < 1 || W < 1 || (C != 1 && C != 3) || R < 1 || mode < 0 || mode > enc::kAdaptive) return 2;
        cases.emplace_back();
        Case& c = cases.back();
        c.im = tt_png_enc_image{0, 0, 0, W, H, C, R, mode, 0};
        if (!Fmt::bound(c.im)) return 2;
        const slots::Region<Fmt> r = slots::region<Fmt>(c.im);
        const enc::FileGeom& g = r.g;
        const long long row = (long long)W * C, image = H * row;
        c.pixels.resize((size_t)image);
        uint8_t* pixels = guarded(image);
        if (!read_exact(f, pixels, (size_t)image)) return 2;
        memcpy(c.pixels.data(), pixels, (size_t)image);

        uint8_t* lines = guarded(g.expect);
        for (int y = 0; y < H; ++y)
            enc::filter_row(*F, pixels + y * row, y ? pixels + (y - 1) * row : nullptr, (int)row, C, mode, lines + y * g.stride, L);
        std::vector<uint8_t*> slot_at((size_t)g.nseg);
        int32_t* sizes = (int32_t*)malloc(4 * (size_t)g.nseg);
        long long* seg_at = (long long*)malloc(8 * (size_t)g.nseg);
        long long total = 0;
        int dynamic = 0, stored = 0, limited = 0;
        bool ok = true;
        for (int s = 0; s < g.nseg; ++s) {
            const long long n = s == g.nseg - 1 ? g.n_last : g.n_full, cap = slots::slot_cap(r, s);
            slot_at[(size_t)s] = guarded(cap);
            enc::Stats st;
            const long long got = enc::deflate_segment(*S, lines + (long long)s * g.rows * g.stride, (int)n, slot_at[(size_t)s], cap, L, st);
            ok = ok && got <= enc::stored_only_bytes(n) && got <= cap && guards_ok(slot_at[(size_t)s], cap);
            sizes[s] = (int32_t)got;
            total += got;
            dynamic += st.dynamic_blocks;
            stored += st.stored_blocks;
            limited += st.limited_blocks;
        }
        const long long bytes = enc::file_bytes(g, total);
        c.file.resize((size_t)bytes);
        uint8_t* file = guarded(bytes);
        ok = ok && bytes <= Fmt::bound(c.im) && enc::write_container(file, H, W, C, R, g, sizes, seg_at) == bytes;
        for (int s = 0; s < g.nseg; ++s) memcpy(file + seg_at[s], slot_at[(size_t)s], (size_t)sizes[s]);
        const long long payload = 2 + total + 6;
        write_checksums(file, g, payload, lines);
        ok = ok && guards_ok(pixels, image) && guards_ok(lines, g.expect) && guards_ok(file, bytes);
        memcpy(c.file.data(), file, (size_t)bytes);

        // the round trip: the whole stream, then every segment alone
        uint8_t* stream = (uint8_t*)malloc((size_t)payload);      // (a block of its own: 4-byte aligned, exact)
        memcpy(stream, file + g.idat_at + 8, (size_t)payload);
        uint8_t* back = (uint8_t*)malloc((size_t)g.expect);
        uint8_t* decoded = (uint8_t*)malloc((size_t)image);
        int st = tt_png::inflate_zlib(*D, stream, 0, (int)payload, payload, back, (int)g.expect, 0, 1);
        ok = ok && st == TT_PNG_OK && memcmp(back, lines, (size_t)g.expect) == 0;
        if (ok) ok = tt_png::unfilter_serial(back, H, W, C, decoded) == TT_PNG_OK && memcmp(decoded, pixels, (size_t)image) == 0;
        long long at = 2;
        for (int s = 0; ok && s < g.nseg; ++s) {
            const long long n = s == g.nseg - 1 ? g.n_last : g.n_full;
            uint8_t* alone = (uint8_t*)malloc((size_t)n);
            const int skew = (int)(at & 3);
            st = tt_png::inflate_segment(*D, stream + (at - skew), skew, skew + sizes[s], payload - (at - skew), alone, 0, (int)n, 32768, 0, 1);
            ok = st == TT_PNG_OK && memcmp(alone, lines + (long long)s * g.rows * g.stride, (size_t)n) == 0;
            free(alone);
            at += sizes[s];
        }
        const std::string path = std::string(argv[2]) + "/" + std::to_string(i) + ".png";
        FILE* o = fopen(path.c_str(), "wb");
        if (!o || fwrite(file, 1, (size_t)bytes, o) != (size_t)bytes) return 2;
        fclose(o);
        printf("%s %s: bytes %lld dynamic %d stored %d limited %d\n", ok ? "ok  " : "FAIL", name.c_str(), bytes, dynamic, stored, limited);
        failed += ok ? 0 : 1;
        for (uint8_t* s : slot_at) release(s);
        release(pixels); release(lines); release(file);
        free(sizes); free(seg_at); free(stream); free(back); free(decoded);
    }
    fclose(f);
    if (count > 0) failed += batch(cases, *S, *F, L) ? 0 : 1;
    delete S;
    delete F;
    delete D;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}

// Stand-alone checker of thinktwice_amd/csrc/png_deflate.h on the CPU: the same source the device kernels run, with one thread
// playing the 64 lanes, over the case file tests/png_encode_cases.py::write_case_file writes.  Every case is encoded to a
// complete PNG file (the bytes tt_png_encode_u8 writes), then inflated again by the host build of png_inflate.h -- the whole
// stream, and every segment alone at the offsets of the file's own ttSG chunk -- unfiltered and compared with the pixels.
// Every buffer is a heap block of the exact size, so a build with -fsanitize=address,undefined sees any access outside the
// pixels, the scanlines, a segment's slot or the file.
//
//   png_encode_host_check <case file> <output directory>
//       writes <output directory>/<case index>.png and prints per case
//       "ok   <name>: bytes B dynamic D stored S limited L" (blocks written as dynamic, as stored, and blocks whose code
//       lengths the 15 / 7 bit limit changed); exit 0 if every round trip is clean
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/png_deflate.h"
#include "../thinktwice_amd/csrc/png_checksum.h"

namespace enc = tt_pngenc;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

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
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, p[5];
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, p, 20)) return 2;
        const int H = p[0], W = p[1], C = p[2], R = p[3], mode = p[4];
        if (H < 1 || W < 1 || (C != 1 && C != 3) || R < 1 || mode < 0 || mode > enc::kAdaptive) return 2;
        const enc::FileGeom g = enc::file_geom(H, W, C, R);
        const long long row = (long long)W * C, image = H * row;
        uint8_t* pixels = (uint8_t*)malloc((size_t)image);
        if (!read_exact(f, pixels, (size_t)image)) return 2;

        uint8_t* lines = (uint8_t*)malloc((size_t)g.expect);
        for (int y = 0; y < H; ++y)
            enc::filter_row(*F, pixels + y * row, y ? pixels + (y - 1) * row : nullptr, (int)row, C, mode, lines + y * g.stride, L);
        std::vector<uint8_t*> slots((size_t)g.nseg);
        int32_t* sizes = (int32_t*)malloc(4 * (size_t)g.nseg);
        long long* seg_at = (long long*)malloc(8 * (size_t)g.nseg);
        long long total = 0;
        int dynamic = 0, stored = 0, limited = 0;
        bool ok = true;
        for (int s = 0; s < g.nseg; ++s) {
            const long long n = enc::segment_rows(g, H, s) * g.stride, cap = enc::segment_slot_bytes(n);
            slots[(size_t)s] = (uint8_t*)malloc((size_t)cap);
            enc::Stats st;
            const long long got = enc::deflate_segment(*S, lines + (long long)s * g.rows * g.stride, (int)n, slots[(size_t)s], cap, L, st);
            ok = ok && got <= enc::stored_only_bytes(n) && got <= cap;
            sizes[s] = (int32_t)got;
            total += got;
            dynamic += st.dynamic_blocks;
            stored += st.stored_blocks;
            limited += st.limited_blocks;
        }
        const long long bytes = enc::file_bytes(g, total);
        uint8_t* file = (uint8_t*)malloc((size_t)bytes);
        ok = ok && bytes <= enc::file_bound(g, H) && enc::write_container(file, H, W, C, R, g, sizes, seg_at) == bytes;
        for (int s = 0; s < g.nseg; ++s) memcpy(file + seg_at[s], slots[(size_t)s], (size_t)sizes[s]);
        const long long payload = 2 + total + 6;
        uint8_t* idat = file + g.idat_at;
        enc::put_be32(idat + 8 + payload - 4, adler32_of(lines, g.expect));
        enc::put_be32(file + 29, crc32_of(file + 12, 17));
        enc::put_be32(file + g.idat_at - 4, crc32_of(file + enc::kTtsgAt + 4, g.idat_at - 4 - (enc::kTtsgAt + 4)));
        enc::put_be32(idat + 8 + payload, crc32_of(idat + 4, 4 + payload));

        // the round trip: the whole stream, then every segment alone
        uint8_t* stream = (uint8_t*)malloc((size_t)payload);      // (a block of its own: 4-byte aligned, exact)
        memcpy(stream, idat + 8, (size_t)payload);
        uint8_t* back = (uint8_t*)malloc((size_t)g.expect);
        uint8_t* decoded = (uint8_t*)malloc((size_t)image);
        int st = tt_png::inflate_zlib(*D, stream, 0, (int)payload, payload, back, (int)g.expect, 0, 1);
        ok = ok && st == TT_PNG_OK && memcmp(back, lines, (size_t)g.expect) == 0;
        if (ok) ok = tt_png::unfilter_serial(back, H, W, C, decoded) == TT_PNG_OK && memcmp(decoded, pixels, (size_t)image) == 0;
        long long at = 2;
        for (int s = 0; ok && s < g.nseg; ++s) {
            const long long n = enc::segment_rows(g, H, s) * g.stride;
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
        for (uint8_t* s : slots) free(s);
        free(pixels); free(lines); free(sizes); free(seg_at); free(file); free(stream); free(back); free(decoded);
    }
    fclose(f);
    delete S;
    delete F;
    delete D;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}

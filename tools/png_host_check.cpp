// Stand-alone checker of thinktwice_amd/csrc/png_inflate.h on the CPU: the same source the device kernels run, as one lane of
// one, over the case file tests/png_cases.py::write_case_file writes.  Every buffer is a heap block of the exact size, so a
// build with -fsanitize=address,undefined sees any access outside the stream, the scanlines or the image.
//
//   png_host_check <case file>      exit 0: every good case byte-equal, every malformed case its expected status
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/png_inflate.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTPNGC01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    tt_png::State* S = new tt_png::State;
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, hwcs[4];
        int64_t stream_len = 0, pixel_len = 0;
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, hwcs, 16) || !read_exact(f, &stream_len, 8)) return 2;
        uint8_t* stream = (uint8_t*)malloc((size_t)stream_len);
        if (!read_exact(f, stream, (size_t)stream_len) || !read_exact(f, &pixel_len, 8)) return 2;
        uint8_t* want = (uint8_t*)malloc((size_t)pixel_len + 1);
        if (!read_exact(f, want, (size_t)pixel_len)) return 2;
        const int H = hwcs[0], W = hwcs[1], C = hwcs[2], expected = hwcs[3];
        const long long expect = (long long)H * (1 + (long long)W * C), image = (long long)H * W * C;
        uint8_t* lines = (uint8_t*)malloc((size_t)expect);
        uint8_t* pixels = (uint8_t*)malloc((size_t)image);
        memset(pixels, 0xA5, (size_t)image);
        int st = tt_png::inflate_zlib(*S, stream, 0, (int)stream_len, stream_len, lines, (int)expect, 0, 1);
        if (st == TT_PNG_OK) st = tt_png::unfilter_serial(lines, H, W, C, pixels);
        bool ok = st == expected;
        if (ok && expected == TT_PNG_OK) ok = pixel_len == image && memcmp(pixels, want, (size_t)image) == 0;
        if (ok && st == TT_PNG_BAD_FILTER)
            for (long long k = 0; k < image; ++k) ok = ok && pixels[k] == 0xA5;
        printf("%s %s: status %d, expected %d\n", ok ? "ok  " : "FAIL", name.c_str(), st, expected);
        failed += ok ? 0 : 1;
        free(stream);
        free(want);
        free(lines);
        free(pixels);
    }
    fclose(f);
    delete S;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}

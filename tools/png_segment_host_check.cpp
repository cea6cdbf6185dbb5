// Stand-alone checker of the segment inflate of thinktwice_amd/csrc/png_inflate.h (inflate_segment, inflate_span) on the CPU:
// the same source the device kernel runs (csrc/png_segments.hip), as one lane of one, over the case file
// tests/png_segment_cases.py::write_case_file writes.  Every segment's input is a heap block of its exact size and the image's
// scanlines are one heap block of exactly H * (1 + W * C) bytes, so a build with -fsanitize=address,undefined sees any access
// outside the segment or the image; and after every segment the checker itself compares every byte of the scanlines OUTSIDE
// the segment's rows with what it was before: the neighbouring rows belong to other waves on the device.
//
//   png_segment_host_check <case file>   exit 0: every good case byte-equal, every malformed case its expected status
//                                        (expected -1: any status but TT_PNG_OK)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../thinktwice_amd/csrc/png_inflate.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Segment {
    int64_t offset, bytes;
    int32_t first_row, rows;
};

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || !read_exact(f, magic, 8) || memcmp(magic, "TTPNGS01", 8) != 0 || !read_exact(f, &count, 4)) {
        fprintf(stderr, "%s: not a segment case file\n", argv[1]);
        return 2;
    }
    tt_png::SegmentState* S = new tt_png::SegmentState;          // the device kernel's: 2 KiB of staged input
    int failed = 0;
    for (int i = 0; i < count; ++i) {
        int32_t name_len = 0, head[6];                           // h, w, c, expected status, window, number of segments
        int64_t payload_len = 0, want_len = 0;
        if (!read_exact(f, &name_len, 4) || name_len < 0 || name_len > 4096) return 2;
        std::string name((size_t)name_len, ' ');
        if (!read_exact(f, &name[0], (size_t)name_len) || !read_exact(f, head, 24) || !read_exact(f, &payload_len, 8)) return 2;
        std::vector<uint8_t> payload((size_t)payload_len);
        if (!read_exact(f, payload.data(), (size_t)payload_len)) return 2;
        const int H = head[0], W = head[1], C = head[2], expected = head[3], window = head[4], nseg = head[5];
        std::vector<Segment> segs((size_t)nseg);
        for (Segment& s : segs)
            if (!read_exact(f, &s.offset, 8) || !read_exact(f, &s.bytes, 8) || !read_exact(f, &s.first_row, 4) || !read_exact(f, &s.rows, 4))
                return 2;
        if (!read_exact(f, &want_len, 8)) return 2;
        std::vector<uint8_t> want((size_t)want_len);
        if (!read_exact(f, want.data(), (size_t)want_len)) return 2;

        const long long stride = 1 + (long long)W * C, expect = H * stride;
        uint8_t* lines = nullptr;                                // 16-byte aligned, exactly the image's scanlines
        if (posix_memalign((void**)&lines, 16, (size_t)expect) != 0) return 2;
        memset(lines, 0xA5, (size_t)expect);
        std::vector<uint8_t> before((size_t)expect);
        int st = TT_PNG_OK;
        bool outside = false;
        for (int k = 0; k < nseg; ++k) {                         // every segment runs, as on the device; the first error is the image's
            const Segment& s = segs[(size_t)k];
            if (s.offset < 0 || s.bytes < 1 || s.offset + s.bytes > payload_len || s.first_row < 0 || s.rows < 1 ||
                s.first_row + s.rows > H)
                return 2;                                        // (what the entry refuses before any launch)
            uint8_t* in = (uint8_t*)malloc((size_t)s.bytes);
            memcpy(in, payload.data() + s.offset, (size_t)s.bytes);
            memcpy(before.data(), lines, (size_t)expect);
            const long long lo = s.first_row * stride, hi = lo + s.rows * stride;
            const int one = tt_png::inflate_segment(*S, in, 0, (int)s.bytes, s.bytes, lines, lo, (int)(hi - lo), window, 0, 1);
            for (long long p = 0; p < expect; ++p)
                if ((p < lo || p >= hi) && lines[p] != before[(size_t)p]) outside = true;
            if (st == TT_PNG_OK) st = one;
            free(in);
        }
        if (nseg > 0) {                                          // the tail: one final block without output, the Adler-32
            const int64_t at = segs[(size_t)nseg - 1].offset + segs[(size_t)nseg - 1].bytes, n = payload_len - at;
            if (n < 1) return 2;
            uint8_t* in = (uint8_t*)malloc((size_t)n);
            memcpy(in, payload.data() + at, (size_t)n);
            memcpy(before.data(), lines, (size_t)expect);
            tt_png::Span J;
            J.base = in; J.limit = n; J.slot = lines; J.slot_pos = 0;
            J.start = 0; J.end = (int)n; J.expect = 0; J.window = window; J.kind = tt_png::kSpanTail;
            uint32_t trailer = 0;
            const int one = tt_png::inflate_span(*S, J, 0, 1, &trailer);
            if (memcmp(before.data(), lines, (size_t)expect) != 0) outside = true;
            if (st == TT_PNG_OK) st = one;
            if (one == TT_PNG_OK && n >= 4) {
                const uint8_t* a = in + n - 4;
                if (trailer != (((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3])) outside = true;
            }
            free(in);
        }
        bool ok = !outside && (expected < 0 ? st != TT_PNG_OK : st == expected);
        if (ok && expected == TT_PNG_OK) ok = want_len == expect && memcmp(lines, want.data(), (size_t)expect) == 0;
        printf("%s %s: status %d, expected %d%s\n", ok ? "ok  " : "FAIL", name.c_str(), st, expected,
               outside ? ", bytes outside a segment's rows were written" : "");
        failed += ok ? 0 : 1;
        free(lines);
    }
    fclose(f);
    delete S;
    printf("%d cases, %d failed\n", count, failed);
    return failed ? 1 : 0;
}

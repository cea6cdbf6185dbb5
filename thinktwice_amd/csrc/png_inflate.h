// The inflate core of the PNG decoder, written once: the bit reader, the fixed and dynamic Huffman tables (RFC 1951 3.2), the
// symbol loop, the zlib wrapper (RFC 1950) and the five PNG filter reconstructions (PNG specification, section 9).  Plain
// functions over byte spans, no HIP type in any signature.  csrc/png.hip compiles them as device code (one 64-lane wave per
// stream), csrc/png_segments.hip one wave per SEGMENT of a stream that has restart points (inflate_segment, inflate_span,
// below the zlib wrapper); tools/png_host_check.cpp and tools/png_segment_host_check.cpp compile the same text as host C++
// with lane = 0 of 1, only so that it can be run under sanitizers on the CPU.  The library has no CPU path.
//
// Execution model.  Every lane of the wave runs the same decode: the reader state and every decision depend only on the
// stream, so control flow is wave-uniform and TT_PNG_SYNC() (a workgroup barrier on the device, nothing on the host) is
// always reached by all lanes.  The lanes differ where bytes move: the input is staged into the state's buffer by all lanes,
// a match is copied 64 bytes per step, the fast decode tables are filled and the window is flushed by all lanes.  The last
// 32 KiB of output live in the state's ring (LDS on the device): a back-reference reads the ring, never memory that another
// lane has just stored through the vector cache.
//
// Bounds.  Every loop iteration consumes at least one input bit or produces at least one output byte, and both counts are
// checked against the stream's length and the expected output size BEFORE the access.  A malformed stream ends in a status
// code after a finite number of steps.  The expected size, H * (1 + W * C), is known up front; more or fewer bytes are errors.
//
// Codes.  Over-subscribed code lengths are refused; an incomplete code is accepted exactly where zlib's inflate_table accepts
// it: a literal/length or distance code that consists of ONE code of length 1 (what deflate writes for a single distance),
// or no code at all (using it is TT_PNG_BAD_SYMBOL); the code-length code must be complete.  A bit pattern no code has, and
// the symbols 286, 287 (length) and 30, 31 (distance), are TT_PNG_BAD_SYMBOL.
//
// NOT verified here: the Adler-32 trailer.  Its four bytes must be present (else TT_PNG_TRUNCATED); inflate_zlib hands their
// value out on request and tt_png_decode_u8_verified compares it with the checksum of the scanlines (png_checksum.h).
#pragma once
#include <stdint.h>

#include "../../include/thinktwice_hip.h"
#include "lanes.h"          // TT_HD, TT_PNG_SYNC, TT_PNG_UNIFORM / uniform

namespace tt_png {

constexpr int kWindow = 32768;          // the ring: deflate's largest window
constexpr int kFlush = 8192;            // bytes per flush of the ring to the output; divides kWindow, a multiple of 16
constexpr int kInWords = 1024;          // staged input, 4-byte words: State's; the functions below take any StateT<kInW>
constexpr int kFastBits = 10;           // codes up to this length decode with one table read
constexpr int kMaxBits = 15;

struct alignas(16) Quad {
    uint32_t w[4];
};

struct Huff {
    uint16_t count[kMaxBits + 1];       // codes of each length
    uint16_t symbol[288];               // symbols in canonical order
    uint16_t fast[1 << kFastBits];      // (symbol << 4) | length for a code of length <= the table's bits, 0 otherwise
    int status;                         // of its construction
};

template <int kInW>
struct StateT {
    alignas(16) uint8_t ring[kWindow];
    alignas(16) uint32_t in[kInW];
    Huff lit, dist;
    uint8_t lens[320];                  // code lengths of the block header: literal/length then distance
};
using State = StateT<kInWords>;         // 42,496 bytes: three one-wave workgroups in a CU's 160 KiB of LDS
// The state of csrc/png_segments.hip: half the staged input, 40,448 bytes, so that FOUR workgroups fit (4 x 40 KiB), one wave
// on each of the CU's four SIMDs.  Measured gain and what it costs the whole-stream kernels if they share it:
// profiles/train_png_segmented.txt.
constexpr int kSegmentInWords = 512;
using SegmentState = StateT<kSegmentInWords>;

// The stream is bytes [start, end) of `base`, a 4-byte aligned pointer of which [0, limit) may be read; end <= 2^31 - 8.
struct Reader {
    const uint8_t* base;
    long long limit;
    int start, end;
    int next_word;                      // next word of `base` that goes into `bits`
    int buf_word0;                      // the word State::in[0] holds
    uint64_t bits;
    int cnt;                            // valid bits in `bits`, stream bytes only
};

template <int kInW>
TT_HD inline void stage_input(StateT<kInW>& S, Reader& R, int lane, int nlanes) {
    TT_PNG_SYNC();
    for (int w = lane; w < kInW; w += nlanes) {
        const long long b0 = 4LL * (R.buf_word0 + w);
        uint32_t v = 0;
        if (b0 < R.end) {
            if (b0 + 4 <= R.limit) {
                v = *reinterpret_cast<const uint32_t*>(R.base + b0);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (b0 + j < R.limit) v |= (uint32_t)R.base[b0 + j] << (8 * j);
            }
        }
        S.in[w] = v;
    }
    TT_PNG_SYNC();
}

// The reader's state is the same in every lane; saying so at the head of every symbol keeps it in scalar registers whatever
// the compiler concluded about the loops in between.
TT_HD inline void assert_uniform(Reader& R) {
    R.cnt = uniform(R.cnt);
    R.start = uniform(R.start);
    R.next_word = uniform(R.next_word);
    R.buf_word0 = uniform(R.buf_word0);
    R.bits = ((uint64_t)uniform((uint32_t)(R.bits >> 32)) << 32) | uniform((uint32_t)R.bits);
}

// Tops `bits` up to more than 32 valid bits while the stream has bytes left (at most two rounds: the first word may start
// inside the word, the last may end inside it).
template <int kInW>
TT_HD inline void refill(StateT<kInW>& S, Reader& R, int lane, int nlanes) {
    while (R.cnt <= 32 && 4 * R.next_word < R.end) {
        if (R.next_word >= R.buf_word0 + kInW) {
            R.buf_word0 = R.next_word;
            stage_input(S, R, lane, nlanes);
        }
        const int b0 = 4 * R.next_word;
        uint64_t v = TT_PNG_UNIFORM(S.in[R.next_word - R.buf_word0]);
        if (b0 >= R.start && b0 + 4 <= R.end) {                  // a whole word of the stream: all but its first and last
            R.bits |= v << R.cnt;
            R.cnt += 32;
        } else {
            const int lo = b0 < R.start ? R.start - b0 : 0;
            const int hi = R.end - b0 < 4 ? R.end - b0 : 4;
            if (hi > lo) {
                if (hi < 4) v &= (1ull << (8 * hi)) - 1;
                v >>= 8 * lo;
                R.bits |= v << R.cnt;
                R.cnt += 8 * (hi - lo);
            }
        }
        ++R.next_word;
    }
}

// n <= 32.  False: the stream ends before n more bits.
template <int kInW>
TT_HD inline bool need(StateT<kInW>& S, Reader& R, int n, int lane, int nlanes) {
    if (R.cnt < n) refill(S, R, lane, nlanes);
    return R.cnt >= n;
}

TT_HD inline uint32_t take(Reader& R, int n) {      // after need(n)
    const uint32_t v = (uint32_t)(R.bits & ((1ull << n) - 1));
    R.bits >>= n;
    R.cnt -= n;
    return v;
}

// Canonical decode of the code in the low bits of v (first bit of the code lowest), lengths 1..max_len: (symbol << 4) | length,
// 0 when no code of those lengths matches.
TT_HD inline uint32_t decode_slow(const Huff& h, uint32_t v, int max_len) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= max_len; ++len) {
        code |= (int)(v & 1);
        v >>= 1;
        const int count = h.count[len];
        if (code - count < first) return ((uint32_t)h.symbol[index + (code - first)] << 4) | (uint32_t)len;
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

// `lens[0..n)` -> h.  is_code_lengths: the code-length code, which must be complete.
TT_HD inline int build(Huff& h, const uint8_t* lens, int n, int fast_bits, bool is_code_lengths, int lane, int nlanes) {
    TT_PNG_SYNC();
    if (lane == 0) {
        int status = TT_PNG_OK;
        for (int l = 0; l <= kMaxBits; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) ++h.count[lens[s]];
        int max_len = 0;
        for (int l = 1; l <= kMaxBits; ++l)
            if (h.count[l]) max_len = l;
        int left = 1;
        for (int l = 1; l <= kMaxBits; ++l) {
            left <<= 1;
            left -= h.count[l];
            if (left < 0) break;
        }
        if (max_len != 0 && (left < 0 || (left > 0 && (is_code_lengths || max_len != 1)))) status = TT_PNG_BAD_CODE_LENGTHS;
        if (status == TT_PNG_OK) {
            uint16_t offs[kMaxBits + 1];
            offs[1] = 0;
            for (int l = 1; l < kMaxBits; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
            for (int s = 0; s < n; ++s)
                if (lens[s]) h.symbol[offs[lens[s]]++] = (uint16_t)s;
        }
        h.count[0] = 0;
        h.status = status;
    }
    TT_PNG_SYNC();
    const int status = TT_PNG_UNIFORM(h.status);
    if (status == TT_PNG_OK)
        for (int e = lane; e < (1 << fast_bits); e += nlanes) h.fast[e] = (uint16_t)decode_slow(h, (uint32_t)e, fast_bits);
    TT_PNG_SYNC();
    return status;
}

// One symbol of h, whose fast table was built for `fast_bits`: >= 0, or -(status).  Peeks up to 15 bits, zero-padded past
// the stream's end; a code that needs more bits than the stream has left is TT_PNG_TRUNCATED, and so is an unmatched
// pattern when fewer than 15 real bits were seen.
template <int kInW>
TT_HD inline int decode(StateT<kInW>& S, Reader& R, const Huff& h, int fast_bits, int lane, int nlanes) {
    assert_uniform(R);
    if (R.cnt < kMaxBits) refill(S, R, lane, nlanes);
    const uint32_t v = (uint32_t)R.bits & 0x7fffu;
    uint32_t e = TT_PNG_UNIFORM((uint32_t)h.fast[v & ((1u << fast_bits) - 1)]);
    if (e == 0) e = TT_PNG_UNIFORM(decode_slow(h, v, kMaxBits));
    if (e == 0) return R.cnt < kMaxBits ? -TT_PNG_TRUNCATED : -TT_PNG_BAD_SYMBOL;
    const int len = (int)(e & 15u);
    if (len > R.cnt) return -TT_PNG_TRUNCATED;
    R.bits >>= len;
    R.cnt -= len;
    return (int)(e >> 4);
}

// The decoded stream: `pos` bytes so far, the first `flushed` of them (a multiple of kFlush) already in `out`.  The caller
// owns bytes [lo, expect) of `out` and nothing else is stored to: a whole stream has lo = 0; a segment (inflate_segment) that
// starts at any byte of its image's scanlines has `out` rounded down to 16 bytes and lo = 0..15, and the 16-byte groups at
// its two ends belong in part to the neighbouring segments, which other waves write at the same time.  pos starts at lo.
struct Output {
    uint8_t* out;                       // 16-byte aligned
    int expect, pos, flushed;
    int lo;
};

template <int kInW>
TT_HD inline void flush_full(StateT<kInW>& S, Output& O, int lane, int nlanes) {
    while (O.pos - O.flushed >= kFlush) {
        TT_PNG_SYNC();
        const Quad* src = reinterpret_cast<const Quad*>(S.ring + (O.flushed & (kWindow - 1)));
        Quad* dst = reinterpret_cast<Quad*>(O.out + O.flushed);
        const int q0 = O.flushed < O.lo ? 1 : 0;                   // the first group of a segment: only its bytes from `lo`
        for (int q = q0 + lane; q < kFlush / 16; q += nlanes) dst[q] = src[q];
        if (q0)
            for (int p = O.lo + lane; p < 16; p += nlanes) O.out[p] = S.ring[p];
        O.flushed += kFlush;
    }
}

template <int kInW>
TT_HD inline void flush_tail(StateT<kInW>& S, Output& O, int lane, int nlanes) {
    TT_PNG_SYNC();
    for (int p = O.flushed + lane; p < O.pos; p += nlanes) O.out[p] = S.ring[p & (kWindow - 1)];
    TT_PNG_SYNC();
}

// flush_tail for an output that owns [lo, pos) only, with 16-byte stores where a whole group is owned: bytes up to the first
// 16-byte boundary at or above max(flushed, lo), groups up to the last boundary at or below pos, bytes after it.
template <int kInW>
TT_HD inline void flush_tail_owned(StateT<kInW>& S, Output& O, int lane, int nlanes) {
    TT_PNG_SYNC();
    const int from = O.flushed > O.lo ? O.flushed : O.lo;
    int a = (from + 15) & ~15, b = O.pos & ~15;
    if (a > b) a = b = O.pos;                                     // no whole group: bytes only
    for (int p = from + lane; p < a; p += nlanes) O.out[p] = S.ring[p & (kWindow - 1)];
    for (int p = a + 16 * lane; p < b; p += 16 * nlanes)
        *reinterpret_cast<Quad*>(O.out + p) = *reinterpret_cast<const Quad*>(S.ring + (p & (kWindow - 1)));
    for (int p = b + lane; p < O.pos; p += nlanes) O.out[p] = S.ring[p & (kWindow - 1)];
    TT_PNG_SYNC();
}

// Byte i of a match is out[pos - dist + (i mod dist)]: every source byte was written before the match began, so the lanes
// of one step never depend on each other, whatever the overlap.  A slot of the ring is reused 32 KiB later, at the earliest
// by the lane that has just read it (dist = 32768).
template <int kInW>
TT_HD inline void copy_match(StateT<kInW>& S, int pos, int len, int dist, int lane, int nlanes) {
    const int src0 = pos - dist;
    for (int i0 = 0; i0 < len; i0 += nlanes) {
        TT_PNG_SYNC();
        const int i = i0 + lane;
        if (i < len) {
            const int k = dist >= len ? i : (dist == 1 ? 0 : i % dist);
            const uint8_t b = S.ring[(src0 + k) & (kWindow - 1)];
            S.ring[(pos + i) & (kWindow - 1)] = b;
        }
    }
}

template <int kInW>
TT_HD inline int read_dynamic_header(StateT<kInW>& S, Reader& R, int lane, int nlanes) {
    if (!need(S, R, 14, lane, nlanes)) return TT_PNG_TRUNCATED;
    const int nlen = (int)take(R, 5) + 257, ndist = (int)take(R, 5) + 1, ncode = (int)take(R, 4) + 4;
    if (nlen > 286 || ndist > 30) return TT_PNG_BAD_CODE_LENGTHS;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    TT_PNG_SYNC();
    for (int i = 0; i < 19; ++i) {
        int l = 0;
        if (i < ncode) {
            if (!need(S, R, 3, lane, nlanes)) return TT_PNG_TRUNCATED;
            l = (int)take(R, 3);
        }
        if (lane == 0) S.lens[order[i]] = (uint8_t)l;
    }
    int st = build(S.lit, S.lens, 19, 7, true, lane, nlanes);
    if (st != TT_PNG_OK) return st;
    int idx = 0, prev = 0;
    while (idx < nlen + ndist) {
        const int sym = decode(S, R, S.lit, 7, lane, nlanes);
        if (sym < 0) return sym == -TT_PNG_BAD_SYMBOL ? TT_PNG_BAD_CODE_LENGTHS : -sym;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (idx == 0) return TT_PNG_BAD_CODE_LENGTHS;
            if (!need(S, R, 2, lane, nlanes)) return TT_PNG_TRUNCATED;
            rep = 3 + (int)take(R, 2);
            val = prev;
        } else if (sym == 17) {
            if (!need(S, R, 3, lane, nlanes)) return TT_PNG_TRUNCATED;
            rep = 3 + (int)take(R, 3);
            val = 0;
        } else if (sym == 18) {
            if (!need(S, R, 7, lane, nlanes)) return TT_PNG_TRUNCATED;
            rep = 11 + (int)take(R, 7);
            val = 0;
        }
        if (idx + rep > nlen + ndist) return TT_PNG_BAD_CODE_LENGTHS;
        // (S.lit holds the code-length code by now: the 19 lengths it was built from may be overwritten)
        if (lane == 0)
            for (int j = 0; j < rep; ++j) S.lens[idx + j] = (uint8_t)val;
        idx += rep;
        prev = val;
    }
    TT_PNG_SYNC();
    if (TT_PNG_UNIFORM((int)S.lens[256]) == 0) return TT_PNG_BAD_CODE_LENGTHS;        // no end-of-block code
    st = build(S.lit, S.lens, nlen, kFastBits, false, lane, nlanes);
    if (st != TT_PNG_OK) return st;
    return build(S.dist, S.lens + nlen, ndist, kFastBits, false, lane, nlanes);
}

template <int kInW>
TT_HD inline int build_fixed(StateT<kInW>& S, int lane, int nlanes) {
    TT_PNG_SYNC();
    for (int s = lane; s < 320; s += nlanes) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    int st = build(S.lit, S.lens, 288, kFastBits, false, lane, nlanes);
    if (st != TT_PNG_OK) return st;
    return build(S.dist, S.lens + 288, 32, kFastBits, false, lane, nlanes);
}

template <int kInW>
TT_HD inline int stored_block(StateT<kInW>& S, Reader& R, Output& O, int lane, int nlanes) {
    take(R, R.cnt & 7);                                           // to the byte boundary (R.cnt counts whole stream bytes)
    if (!need(S, R, 32, lane, nlanes)) return TT_PNG_TRUNCATED;
    const uint32_t len = take(R, 16), nlen = take(R, 16);
    if (len != ((~nlen) & 0xffffu)) return TT_PNG_BAD_STORED_LEN;
    if ((int)len > O.expect - O.pos) return TT_PNG_OUTPUT_OVERRUN;
    int left = (int)len;
    while (left > 0 && R.cnt >= 8) {                              // the whole bytes the bit buffer holds already, at most 8
        int n = R.cnt >> 3;
        if (n > left) n = left;
        if (n > 4) n = 4;
        const uint32_t v = take(R, 8 * n);
        for (int j = lane; j < n; j += nlanes) S.ring[(O.pos + j) & (kWindow - 1)] = (uint8_t)(v >> (8 * j));
        O.pos += n;
        left -= n;
    }
    flush_full(S, O, lane, nlanes);
    if (left == 0) return TT_PNG_OK;
    // The bit buffer is empty and the stream stands at byte p: the rest of the run goes from the staged input to the ring,
    // one byte per lane and step, at most one stage (4 KiB or less, under kFlush) between two flushes.
    int p = 4 * R.next_word;
    if (p < R.start) p = R.start;
    if (p > R.end) p = R.end;
    const uint8_t* staged = reinterpret_cast<const uint8_t*>(S.in);
    while (left > 0) {
        p = uniform(p);
        left = uniform(left);
        O.pos = uniform(O.pos);
        O.flushed = uniform(O.flushed);
        if (p >= R.end) return TT_PNG_TRUNCATED;
        if (p >= 4 * (R.buf_word0 + kInW)) {
            R.buf_word0 = p >> 2;
            stage_input(S, R, lane, nlanes);
        }
        const int stage_end = 4 * (R.buf_word0 + kInW);
        int n = (R.end < stage_end ? R.end : stage_end) - p;      // >= 1
        if (n > left) n = left;
        TT_PNG_SYNC();
        for (int i = lane; i < n; i += nlanes) S.ring[(O.pos + i) & (kWindow - 1)] = staged[p - 4 * R.buf_word0 + i];
        O.pos += n;
        left -= n;
        p += n;
        flush_full(S, O, lane, nlanes);
    }
    p = uniform(p);
    R.start = p;                                                  // the bytes below p are consumed: the next word may start inside
    R.next_word = p >> 2;
    R.bits = 0;
    R.cnt = 0;
    refill(S, R, lane, nlanes);
    return TT_PNG_OK;
}

template <int kInW>
TT_HD inline int huffman_block(StateT<kInW>& S, Reader& R, Output& O, int window, int lane, int nlanes) {
    for (;;) {
        O.pos = uniform(O.pos);
        O.flushed = uniform(O.flushed);
        int sym = decode(S, R, S.lit, kFastBits, lane, nlanes);
        if (sym < 0) return -sym;
        if (sym < 256) {
            if (O.pos >= O.expect) return TT_PNG_OUTPUT_OVERRUN;
            if (lane == 0) S.ring[O.pos & (kWindow - 1)] = (uint8_t)sym;
            ++O.pos;
        } else if (sym == 256) {
            return TT_PNG_OK;
        } else {
            sym -= 257;
            if (sym >= 29) return TT_PNG_BAD_SYMBOL;
            int len = 258;
            if (sym < 28) {
                const int ext = sym < 8 ? 0 : (sym - 4) >> 2;
                if (!need(S, R, ext, lane, nlanes)) return TT_PNG_TRUNCATED;
                len = (sym < 8 ? 3 + sym : 3 + ((4 + (sym & 3)) << ext)) + (int)take(R, ext);
            }
            const int dsym = decode(S, R, S.dist, kFastBits, lane, nlanes);
            if (dsym < 0) return -dsym;
            if (dsym >= 30) return TT_PNG_BAD_SYMBOL;
            const int dext = dsym < 4 ? 0 : (dsym >> 1) - 1;
            if (!need(S, R, dext, lane, nlanes)) return TT_PNG_TRUNCATED;
            const int dist = (dsym < 4 ? 1 + dsym : 1 + ((2 + (dsym & 1)) << dext)) + (int)take(R, dext);
            if (dist > O.pos - O.lo || dist > window) return TT_PNG_BAD_DISTANCE;
            if (len > O.expect - O.pos) return TT_PNG_OUTPUT_OVERRUN;
            copy_match(S, O.pos, len, dist, lane, nlanes);
            O.pos += len;
        }
        flush_full(S, O, lane, nlanes);
    }
}

// The zlib stream in bytes [start, end) of `base` (4-byte aligned, readable in [0, limit), start < 4, end <= 2^31 - 8) ->
// exactly `expect` bytes at `out` (16-byte aligned).  Returns a TT_PNG_* status; on an error `out` holds an unspecified
// prefix.  start, end, expect (and limit, out) are the same in every lane.  trailer, if not null: where the stream's Adler-32
// field goes, written once, and only when the status is TT_PNG_OK: the four big-endian bytes after the final block's padding
// to a byte boundary, wherever the stream ends.  Comparing it is the caller's (csrc/png.hip, png_checksum.h).
template <int kInW>
TT_HD inline int inflate_zlib(StateT<kInW>& S, const uint8_t* base, int start, int end, long long limit, uint8_t* out, int expect, int lane,
                              int nlanes, uint32_t* trailer = nullptr) {
    Reader R;
    R.base = base; R.start = start; R.end = end; R.limit = limit;
    R.next_word = 0; R.buf_word0 = 0; R.bits = 0; R.cnt = 0;
    stage_input(S, R, lane, nlanes);
    Output O;
    O.out = out; O.expect = expect; O.pos = 0; O.flushed = 0; O.lo = 0;

    if (!need(S, R, 16, lane, nlanes)) return TT_PNG_TRUNCATED;
    const uint32_t cmf = take(R, 8), flg = take(R, 8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return TT_PNG_BAD_ZLIB_HEADER;
    const int window = 1 << ((int)(cmf >> 4) + 8);

    for (;;) {
        if (!need(S, R, 3, lane, nlanes)) return TT_PNG_TRUNCATED;
        const uint32_t last = take(R, 1), type = take(R, 2);
        int st;
        if (type == 0) {
            st = stored_block(S, R, O, lane, nlanes);
        } else if (type == 3) {
            st = TT_PNG_BAD_BLOCK_TYPE;
        } else {
            st = type == 1 ? build_fixed(S, lane, nlanes) : read_dynamic_header(S, R, lane, nlanes);
            if (st == TT_PNG_OK) st = huffman_block(S, R, O, window, lane, nlanes);
        }
        if (st != TT_PNG_OK) return st;
        if (last) break;
    }
    if (O.pos != O.expect) return TT_PNG_OUTPUT_SHORT;
    flush_tail(S, O, lane, nlanes);
    take(R, R.cnt & 7);
    const int unread = R.end - 4 * R.next_word;
    if ((R.cnt >> 3) + (unread > 0 ? unread : 0) < 4) return TT_PNG_TRUNCATED;      // the Adler-32: present, not verified here
    if (trailer) {                                                // (four more bytes exist: need() cannot fail)
        need(S, R, 32, lane, nlanes);
        const uint32_t v = take(R, 32);                           // the stream's next four bytes, the first one lowest
        if (lane == 0) *trailer = (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
    }
    return TT_PNG_OK;
}

// ------------------------------------------------------------------------------------------------- segments of a stream
// A zlib stream written with a full flush (Z_FULL_FLUSH) after every R rows has restart points: at each one the deflate
// stream is byte-aligned, the block before it is an empty stored block (00 00 FF FF) and no later match reaches back across
// it.  The pieces between them are SEGMENTS: whole non-final blocks, the last of them that empty stored block, which inflate
// alone to their own rows.  What follows the last segment is the stream's TAIL: one final block with no output, then the
// Adler-32.  inflate_span decodes any of the three kinds of span with the block routines above; the kind is a run-time
// value, the same in every lane, so that a kernel that meets all three holds ONE copy of the decode.
enum SpanKind {
    kSpanZlib = 0,          // a whole stream: RFC 1950 header, blocks up to the final one, the Adler-32 field
    kSpanSegment = 1,       // non-final blocks only; ends where a stored block leaves the reader at `end`
    kSpanTail = 2           // no header: blocks up to the final one, the Adler-32 field (a segmented stream's last bytes)
};

// Bytes [start, end) of `base` (4-byte aligned, readable in [0, limit), start < 4, end <= 2^31 - 8) -> exactly `expect` bytes
// at slot + slot_pos.  `slot` is 16-byte aligned and slot_pos may be any byte of it: no store touches a byte outside
// [slot_pos, slot_pos + expect), 16 bytes at a time only where a whole aligned group lies inside (expect <= 2^31 - 17).
// window: deflate's window in bytes, for the two kinds without a header.  Every field is the same in every lane.
struct Span {
    const uint8_t* base;
    long long limit;
    uint8_t* slot;
    long long slot_pos;
    int start, end, expect, window, kind;
};

// Returns a TT_PNG_* status; on an error the span's bytes of `slot` hold an unspecified prefix.
//   kSpanSegment  a block with BFINAL set is TT_PNG_BAD_BLOCK_TYPE: a segment never ends its stream.  TT_PNG_OK exactly when
//                 a stored block leaves the reader at `end` with `expect` bytes produced; at `end` with fewer is
//                 TT_PNG_OUTPUT_SHORT; input that ends anywhere else is TT_PNG_TRUNCATED; input left over is decoded as further
//                 blocks and ends in whatever they are (an output past `expect` is TT_PNG_OUTPUT_OVERRUN).  A distance is
//                 checked against the bytes THIS span has produced: a match that reaches before the segment's first byte is
//                 TT_PNG_BAD_DISTANCE, whatever the stream held there.  A wrong index therefore ends in a status.
//   trailer       as inflate_zlib's, for the two kinds that end in the Adler-32 field.
template <int kInW>
TT_HD inline int inflate_span(StateT<kInW>& S, const Span& J, int lane, int nlanes, uint32_t* trailer = nullptr) {
    Reader R;
    R.base = J.base; R.start = J.start; R.end = J.end; R.limit = J.limit;
    R.next_word = 0; R.buf_word0 = 0; R.bits = 0; R.cnt = 0;
    stage_input(S, R, lane, nlanes);
    const int lo = (int)(J.slot_pos & 15);
    Output O;
    O.out = J.slot + (J.slot_pos - lo); O.lo = lo; O.pos = lo; O.flushed = 0; O.expect = lo + J.expect;
    const bool segment = J.kind == kSpanSegment;
    int window = J.window;

    if (J.kind == kSpanZlib) {
        if (!need(S, R, 16, lane, nlanes)) return TT_PNG_TRUNCATED;
        const uint32_t cmf = take(R, 8), flg = take(R, 8);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return TT_PNG_BAD_ZLIB_HEADER;
        window = 1 << ((int)(cmf >> 4) + 8);
    }
    for (;;) {
        if (!need(S, R, 3, lane, nlanes)) return TT_PNG_TRUNCATED;
        const uint32_t last = take(R, 1), type = take(R, 2);
        if (segment && last) return TT_PNG_BAD_BLOCK_TYPE;
        int st;
        if (type == 0) {
            st = stored_block(S, R, O, lane, nlanes);
        } else if (type == 3) {
            st = TT_PNG_BAD_BLOCK_TYPE;
        } else {
            st = type == 1 ? build_fixed(S, lane, nlanes) : read_dynamic_header(S, R, lane, nlanes);
            if (st == TT_PNG_OK) st = huffman_block(S, R, O, window, lane, nlanes);
        }
        if (st != TT_PNG_OK) return st;
        if (last) break;
        if (segment && type == 0 && !need(S, R, 1, lane, nlanes)) break;      // a stored block has left the reader at `end`
    }
    if (O.pos != O.expect) return TT_PNG_OUTPUT_SHORT;
    flush_tail_owned(S, O, lane, nlanes);
    if (segment) return TT_PNG_OK;
    take(R, R.cnt & 7);
    const int unread = R.end - 4 * R.next_word;
    if ((R.cnt >> 3) + (unread > 0 ? unread : 0) < 4) return TT_PNG_TRUNCATED;
    if (trailer) {
        need(S, R, 32, lane, nlanes);
        const uint32_t v = take(R, 32);
        if (lane == 0) *trailer = (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
    }
    return TT_PNG_OK;
}

// One segment of a stream, next to inflate_zlib: bytes [start, end) of `base` -> `expect` bytes at slot + slot_pos, under
// the stream's window (from its CMF byte, which the caller has).  See Span and inflate_span.
template <int kInW>
TT_HD inline int inflate_segment(StateT<kInW>& S, const uint8_t* base, int start, int end, long long limit, uint8_t* slot, long long slot_pos,
                                 int expect, int window, int lane, int nlanes) {
    Span J;
    J.base = base; J.limit = limit; J.slot = slot; J.slot_pos = slot_pos;
    J.start = start; J.end = end; J.expect = expect; J.window = window; J.kind = kSpanSegment;
    return inflate_span(S, J, lane, nlanes);
}

// ------------------------------------------------------------------------------------------------------------ the filters
TT_HD inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Recon(x) of filter type ft (0..4): a = left, b = up, c = upper left, each 0 outside the image.
TT_HD inline int recon(int ft, int x, int a, int b, int c) {
    const int add = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x + add) & 255;
}

// The serial statement of the unfilter (the device runs rows as a skewed wavefront, csrc/png.hip): filtered scanlines
// [H][1 + W * C] -> dst [H][W][C].  TT_PNG_BAD_FILTER, with dst untouched, if any row's type is above 4.
TT_HD inline int unfilter_serial(const uint8_t* filt, int H, int W, int C, uint8_t* dst) {
    const long long row = (long long)W * C;
    for (int y = 0; y < H; ++y)
        if (filt[y * (row + 1)] > 4) return TT_PNG_BAD_FILTER;
    for (int y = 0; y < H; ++y) {
        const uint8_t* s = filt + y * (row + 1);
        uint8_t* d = dst + y * row;
        const int ft = s[0];
        for (long long i = 0; i < row; ++i) {
            const int a = i >= C ? d[i - C] : 0, b = y > 0 ? d[i - row] : 0, c = (i >= C && y > 0) ? d[i - row - C] : 0;
            d[i] = (uint8_t)recon(ft, s[1 + i], a, b, c);
        }
    }
    return TT_PNG_OK;
}

}  // namespace tt_png

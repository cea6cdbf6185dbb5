// The PNG encoder's core, written once: the five scanline filters with the adaptive choice (PNG specification, sections 9 and
// 12.8) and a deflate compressor (RFC 1951) that writes SEGMENTS -- whole non-final blocks that end in the empty stored block
// 00 00 FF FF and inflate alone, what png_inflate.h's inflate_segment reads.  Plain functions over byte spans, no HIP type in
// any signature.  csrc/png_encode.hip compiles them as device code, one 64-lane workgroup per row (filter) or per segment
// (deflate); tools/png_encode_host_check.cpp compiles the same text as host C++.  Execution model: lanes.h's.
//
// Determinism.  The bytes are a function of the input and the parameters.  No result depends on which lane's LDS update
// lands first: the three shared updates of a phase are commutative and associative (integer add into a histogram, or into the
// output's bit buffer, max into the hash table), ballot and prefix sum are exact integer functions of all 64 lanes' values.
//
// LZ77.  Matches of 4..258 bytes (the format allows 3; a hash of 4 bytes finds none, and on camera frames, depth ramps and tag
// maps the files are 5 to 10 % smaller than with a 3-byte hash: profiles/png_encode.txt) at distances 1..32768 (kWindow,
// ENFORCED: a segment may be longer than the window).  A step
// takes the 64 positions p .. p + 63.  Every lane hashes the 4 bytes at its position into S.hash and reads the entry AS THE
// STEPS BEFORE LEFT IT (candidate = the highest earlier position with that hash), measures the match against the input in
// memory, and only then all 64 positions are inserted: an entry becomes the MAXIMUM of what it held and the positions
// inserted, so the highest position wins whatever the order.  The candidates are resolved greedily from p upwards: at an
// uncovered position with a match the match is taken and the positions it covers are skipped, else the byte is a literal; a
// match may run past p + 63 and the next step then starts where it ends.  A match of 4 bytes further than kFar away is not
// one (its distance costs about what four literals do).
//
// Blocks.  Tokens live in LDS (S.tok, 4 bytes each): a block is cut when fewer than 65 token slots are left, or at the end
// of the segment.  Then: histograms -> length-limited Huffman codes (15 bits; 7 for the code-length code) -> the run-length
// coded header -> the exact size in bits.  The same is sized for the block's bytes as literals only (no match: where matches
// have flattened a skewed byte histogram the tokens' code is the longer one), and the smaller of the two is the dynamic
// block.  If that is not smaller than the same bytes stored, the bytes join the
// pending stored run, which is written in pieces of at most 65,535 bytes before the next dynamic block or at the end.  If
// the finished segment came out larger than the segment stored whole, it is written again as stored blocks only: a
// segment is never larger than stored_only_bytes(n).
// LDS: sizeof(State) = 49,924 bytes per workgroup (16 KiB hash, 24 KiB tokens, 2 KiB bit buffer, the code tables), so three
// one-wave workgroups share a CU's 160 KiB.  Tokens in the workspace instead would free 24 KiB (six workgroups) at the price
// of a global round trip per token; 6144 tokens are also what lets one block hold a histogram deep enough to need the length
// limiter (Fibonacci counts over 17 symbols are 4180 tokens).
//
// Codes.  Lengths by the in-place minimum-redundancy algorithm of Moffat and Katajainen over the symbols sorted by (count,
// symbol); a code deeper than the limit is repaired on the counts per length (one code leaves the deepest level, one
// shallower leaf becomes two) until Kraft's sum is 1, and the lengths are handed out again, longest to rarest.  Edge cases,
// the ones png_inflate.h accepts because zlib does: a block without a match sends ONE distance code (symbol 0, length 1); a
// block that uses one distance sends that one code with length 1; the code-length code is always complete (a lone symbol
// gets a partner of length 1).  The literal/length code always has the end-of-block symbol and at least one more.
#pragma once
#include <stdint.h>

#include "lanes.h"
#include "png_inflate.h"

namespace tt_pngenc {

constexpr int kWindow = 32768;
constexpr int kMinMatch = 4, kMaxMatch = 258;       // what the parse takes; the format's lengths start at kLenBase
constexpr int kLenBase = 3;
constexpr int kFar = 4096;
constexpr int kHashBits = 12;
constexpr int kBlockTokens = 6144;
constexpr int kOutWords = 512;
constexpr int kStoredMax = 65535;
constexpr uint32_t kEob = 256u;                 // token values: 0..255 a literal, 256 end of block, bit 31 a match
enum FilterMode { kNone = 0, kSub = 1, kUp = 2, kAvg = 3, kPaeth = 4, kAdaptive = 5 };

// ---------------------------------------------------------------------------------------------------------------- sizes
// A segment of n >= 1 bytes as stored blocks only: 5 bytes a piece (3 header bits padded to a byte, LEN, NLEN), then the
// closing empty stored block.
TT_HD inline long long stored_only_bytes(long long n) { return n + 5 * ((n + kStoredMax - 1) / kStoredMax) + 5; }
// What deflate_segment may write before it falls back to stored_only_bytes: a dynamic block is taken only when it is smaller
// than its bytes stored behind a 5-byte header, a block but the last has at least kBlockTokens - 65 tokens, and a stored run
// between two of them pays its own headers: under 12 bytes per (kBlockTokens - 65) input bytes, and the stored headers.
TT_HD inline long long segment_slot_bytes(long long n) { return (n + n / 256 + 64 + 15) / 16 * 16; }

// ---------------------------------------------------------------------------------------------------------------- filters
struct FilterState {
    uint32_t sum[5];
};

TT_HD inline int residual(int ft, int x, int a, int b, int c) {
    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : tt_png::paeth(a, b, c);
    return (x - pred) & 255;
}

// One row: cur [row_bytes] (W * C pixels bytes), prev the raw row above or null for the first -> dst [1 + row_bytes].  mode: a
// FilterMode.  kAdaptive: for each of the five types the sum over the row of |residual read as int8|; the smallest sum wins,
// the lowest type number on a tie.  Returns the row's type (the same in every lane).
TT_HD inline int filter_row(FilterState& F, const uint8_t* cur, const uint8_t* prev, int row_bytes, int C, int mode, uint8_t* dst, Lanes L) {
    int ft = mode;
    if (mode == kAdaptive) {
        TT_PNG_SYNC();
        TT_ENC_LANES(l) if (l < 5) F.sum[l] = 0;
        TT_PNG_SYNC();
        TT_ENC_LANES(l) {
            uint32_t s[5] = {0, 0, 0, 0, 0};
            for (int i = l; i < row_bytes; i += kLanes) {
                const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = prev ? prev[i] : 0, c = (prev && i >= C) ? prev[i - C] : 0;
                for (int t = 0; t < 5; ++t) {
                    const int r = residual(t, x, a, b, c);
                    s[t] += (uint32_t)(r < 128 ? r : 256 - r);
                }
            }
            for (int t = 0; t < 5; ++t) TT_ENC_ADD(&F.sum[t], s[t]);
        }
        TT_PNG_SYNC();
        ft = 0;
        uint32_t best = TT_PNG_UNIFORM(F.sum[0]);
        for (int t = 1; t < 5; ++t) {
            const uint32_t s = TT_PNG_UNIFORM(F.sum[t]);
            if (s < best) {
                best = s;
                ft = t;
            }
        }
    }
    TT_ENC_LANES(l) {
        if (l == 0) dst[0] = (uint8_t)ft;
        for (int i = l; i < row_bytes; i += kLanes) {
            const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = prev ? prev[i] : 0, c = (prev && i >= C) ? prev[i - C] : 0;
            dst[1 + i] = (uint8_t)residual(ft, x, a, b, c);
        }
    }
    return ft;
}

// ---------------------------------------------------------------------------------------------------------------- deflate
struct State {
    uint32_t hash[1 << kHashBits];      // position + 1 of the highest earlier position with this hash, 0: none
    uint32_t tok[kBlockTokens];
    uint32_t obuf[kOutWords + 2];       // the output's bits not yet in memory, from byte Writer::base on
    uint32_t ll_freq[288], d_freq[32], cl_freq[20];
    uint32_t lit_freq[288], no_freq[32]; // the block's bytes as literals only: their counts; no distance
    uint32_t key[288], sorted[288];     // code construction
    uint32_t bc[8];                     // what lane 0 computed, for all
    uint32_t cnt[36];                   // code construction: codes per length, the next code of a length
    uint16_t ll_code[288], d_code[32], cl_code[20];
    uint16_t mlen[kLanes];
    uint8_t ll_len[288], d_len[32], cl_len[20];
    uint8_t rle_sym[320], rle_ext[320];
};

struct Stats {
    int dynamic_blocks, stored_blocks, limited_blocks;
};

// `base` bytes of the segment are in memory at out[0, base) (only those below cap are stored), nbits more in S.obuf.
struct Writer {
    uint8_t* out;
    long long cap, base;
    int nbits;
};

TT_HD inline uint32_t obuf_byte(const State& S, int i) { return (S.obuf[i >> 2] >> (8 * (i & 3))) & 255u; }

// n <= 48 bits of v at bit `at` of the buffer
TT_HD inline void or_bits(State& S, int at, uint64_t v, int n) {
    if (n == 0) return;
    const int w = at >> 5, sh = at & 31;
    const uint32_t w0 = (uint32_t)(v << sh);
    const uint64_t rest = (v >> 1) >> (31 - sh);
    if (w0) TT_ENC_OR(&S.obuf[w], w0);
    if ((uint32_t)rest) TT_ENC_OR(&S.obuf[w + 1], (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) TT_ENC_OR(&S.obuf[w + 2], (uint32_t)(rest >> 32));
}

// The whole bytes of the buffer go to memory (with `all`, the last partial byte too, zero-padded); what is left moves to the
// buffer's start.  Bytes up to a 4-byte boundary of the destination, whole words, bytes.
TT_HD inline void flush(State& S, Writer& W, Lanes L, bool all) {
    TT_PNG_SYNC();
    const int nbytes = all ? (W.nbits + 7) >> 3 : W.nbits >> 3;
    const int rem = all ? 0 : W.nbits & 7;
    uint8_t* dst = W.out + W.base;
    long long room = W.cap - W.base;
    if (room < 0) room = 0;
    const int n = nbytes < room ? nbytes : (int)room;
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > n) head = n;
    const int words = (n - head) >> 2;
    TT_ENC_LANES(l) {
        for (int i = l; i < head; i += kLanes) dst[i] = (uint8_t)obuf_byte(S, i);
        for (int w = l; w < words; w += kLanes) {
            const int i = head + 4 * w, sh = 8 * (i & 3);
            uint32_t v = S.obuf[i >> 2] >> sh;
            if (sh) v |= S.obuf[(i >> 2) + 1] << (32 - sh);
            *reinterpret_cast<uint32_t*>(dst + i) = v;
        }
        for (int i = head + 4 * words + l; i < n; i += kLanes) dst[i] = (uint8_t)obuf_byte(S, i);
    }
    const uint32_t carry = rem ? (TT_PNG_UNIFORM(obuf_byte(S, nbytes)) & ((1u << rem) - 1)) : 0u;
    const int used = (W.nbits + 31) >> 5;
    TT_PNG_SYNC();
    TT_ENC_LANES(l)
        for (int w = l; w <= used && w < kOutWords + 2; w += kLanes) S.obuf[w] = w == 0 ? carry : 0u;
    TT_PNG_SYNC();
    W.base += nbytes;
    W.nbits = rem;
}

TT_HD inline void reserve(State& S, Writer& W, Lanes L, int bits) {
    if (W.nbits + bits > kOutWords * 32) flush(S, W, L, false);
}

// n <= 32 bits, the same in every lane; room was reserved
TT_HD inline void put(State& S, Writer& W, Lanes L, uint32_t v, int n) {
    if (L.lo == 0) or_bits(S, W.nbits, v, n);
    W.nbits += n;
}

// Bytes [a, b) of `in` as stored blocks of at most 65,535 bytes; a == b: the empty stored block.
TT_HD inline void emit_stored(State& S, Writer& W, Lanes L, const uint8_t* in, int a, int b, Stats& stats) {
    do {
        const int len = b - a < kStoredMax ? b - a : kStoredMax;
        reserve(S, W, L, 48);
        put(S, W, L, 0u, 3);                                      // BFINAL 0, BTYPE 00
        W.nbits = (W.nbits + 7) & ~7;
        put(S, W, L, (uint32_t)len | ((uint32_t)(~len & 0xffff) << 16), 32);
        flush(S, W, L, true);
        uint8_t* dst = W.out + W.base;
        long long room = W.cap - W.base;
        if (room < 0) room = 0;
        const int n = len < room ? len : (int)room;
        TT_ENC_LANES(l)
            for (int i = l; i < n; i += kLanes) dst[i] = in[a + i];
        W.base += len;
        a += len;
        if (len) ++stats.stored_blocks;
    } while (a < b);
}

TT_HD inline uint32_t hash4(const uint8_t* p) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// the common prefix of a[0, max) and b[0, max)
TT_HD inline int match_length(const uint8_t* a, const uint8_t* b, int max) {
    int n = 0;
    while (n + 8 <= max) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + n, 8);
        __builtin_memcpy(&y, b + n, 8);
        if (x != y) return n + (__builtin_ctzll(x ^ y) >> 3);
        n += 8;
    }
    while (n < max && a[n] == b[n]) ++n;
    return n;
}

TT_HD inline int length_symbol(int len, int& ext, int& extra) {           // 257..285
    const int l = len - kLenBase;
    if (l == 255) { ext = 0; extra = 0; return 285; }
    if (l < 8) { ext = 0; extra = 0; return 257 + l; }
    ext = 29 - __builtin_clz((unsigned)l);                                  // floor(log2 l) - 2
    extra = l & ((1 << ext) - 1);
    return 257 + 4 * ext + 4 + ((l >> ext) & 3);
}

TT_HD inline int distance_symbol(int dist, int& ext, int& extra) {       // 0..29
    const int d = dist - 1;
    if (d < 4) { ext = 0; extra = 0; return d; }
    ext = 30 - __builtin_clz((unsigned)d);                                  // floor(log2 d) - 1
    extra = d & ((1 << ext) - 1);
    return 2 * ext + 2 + ((d >> ext) & 1);
}

TT_HD inline int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
TT_HD inline int distance_extra_bits(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// entry i of 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 (RFC 1951 3.2.7), five bits each
TT_HD inline int code_length_order(int i) {
    return (int)((i < 12 ? 0x22caa324e804a30ull >> (5 * i) : 0x3c2e1346cull >> (5 * (i - 12))) & 31u);
}

TT_HD inline uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// freq[0, n) -> len[0, n), code[0, n) (canonical, bit-reversed: ready to be written low bit first), lengths at most max_len.
// pair: a lone used symbol gets a partner (symbol 0, or 1) so that the code is complete.  lone: the symbol that gets a code of
// length 1 when none is used, or -1.  Returns (in every lane) whether the length limit changed the code.
TT_HD inline bool build_code(State& S, const uint32_t* freq, int n, int max_len, bool pair, int lone, uint8_t* len, uint16_t* code, Lanes L) {
    TT_PNG_SYNC();
    TT_ENC_LANES(l)
        for (int s = l; s < n; s += kLanes) {
            S.key[s] = freq[s] ? (freq[s] << 9) | (uint32_t)s : 0u;
            len[s] = 0;
            code[s] = 0;
        }
    TT_PNG_SYNC();
    TT_ENC_LANES(l)
        for (int s = l; s < n; s += kLanes) {
            const uint32_t k = S.key[s];
            if (!k) continue;
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += (S.key[j] != 0u && S.key[j] < k) ? 1 : 0;
            S.sorted[rank] = k;
        }
    TT_PNG_SYNC();
    if (L.lo == 0) {
        int m = 0;
        for (int s = 0; s < n; ++s) m += S.key[s] != 0u;
        bool limited = false;
        if (m == 0) {
            if (lone >= 0) len[lone] = 1;
        } else if (m == 1) {
            const int s = (int)(S.sorted[0] & 511u);
            len[s] = 1;
            if (pair) len[s == 0 ? 1 : 0] = 1;
        } else {
            uint32_t* A = S.key;                                  // the counts, ascending; then depths
            for (int i = 0; i < m; ++i) A[i] = S.sorted[i] >> 9;
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < m - 1; ++next) {
                if (leaf >= m || A[root] < A[leaf]) {
                    A[next] = A[root];
                    A[root++] = (uint32_t)next;
                } else {
                    A[next] = A[leaf++];
                }
                if (leaf >= m || (root < next && A[root] < A[leaf])) {
                    A[next] += A[root];
                    A[root++] = (uint32_t)next;
                } else {
                    A[next] += A[leaf++];
                }
            }
            A[m - 2] = 0;
            for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avail = 1, used = 0, depth = 0, next = m - 1;
            root = m - 2;
            while (avail > 0) {
                while (root >= 0 && (int)A[root] == depth) {
                    ++used;
                    --root;
                }
                while (avail > used) {
                    A[next--] = (uint32_t)depth;
                    --avail;
                }
                avail = 2 * used;
                ++depth;
                used = 0;
            }
            // A[i]: the depth of the i-th rarest symbol, deepest first
            uint32_t* count = S.cnt;
            for (int d = 0; d <= max_len; ++d) count[d] = 0;
            for (int i = 0; i < m; ++i) {
                if ((int)A[i] > max_len) limited = true;
                ++count[(int)A[i] > max_len ? max_len : (int)A[i]];
            }
            if (limited) {
                uint32_t total = 0;
                for (int d = 1; d <= max_len; ++d) total += count[d] << (max_len - d);
                while (total > (1u << max_len)) {
                    --count[max_len];
                    for (int d = max_len - 1; d > 0; --d)
                        if (count[d]) {
                            --count[d];
                            count[d + 1] += 2;
                            break;
                        }
                    --total;
                }
                int i = 0;
                for (int d = max_len; d >= 1; --d)
                    for (uint32_t k = 0; k < count[d]; ++k) A[i++] = (uint32_t)d;
            }
            for (int i = 0; i < m; ++i) len[S.sorted[i] & 511u] = (uint8_t)A[i];
        }
        uint32_t *count = S.cnt, *next_code = S.cnt + 18;
        for (int d = 0; d <= 16; ++d) count[d] = 0;
        for (int s = 0; s < n; ++s) ++count[len[s]];
        count[0] = 0;
        uint32_t c = 0;
        for (int d = 1; d <= 16; ++d) {
            c = (c + count[d - 1]) << 1;
            next_code[d] = c;
        }
        for (int s = 0; s < n; ++s)
            if (len[s]) code[s] = (uint16_t)reverse_bits(next_code[len[s]]++, len[s]);
        S.bc[7] = limited ? 1u : 0u;
    }
    TT_PNG_SYNC();
    return TT_PNG_UNIFORM(S.bc[7]) != 0u;
}

// A dynamic block whose symbols have the counts ll_freq (end of block included) and d_freq: the three codes, the header's
// run-length code and the block's exact size in bits -> S.ll_len / ll_code, d_*, cl_*, rle_*, and S.bc[0..4] = HLIT + 257,
// HDIST + 1, the header's symbols, HCLEN + 4, the bits.  Returns whether a length limit changed a code.
TT_HD inline bool plan_block(State& S, Lanes L, const uint32_t* ll_freq, const uint32_t* d_freq) {
    bool limited = build_code(S, ll_freq, 286, 15, false, -1, S.ll_len, S.ll_code, L);
    limited = build_code(S, d_freq, 30, 15, false, 0, S.d_len, S.d_code, L) || limited;
    TT_PNG_SYNC();
    if (L.lo == 0) {                                              // the header's run-length code, the code-length counts
        int nlit = 286, ndist = 30;
        while (nlit > 257 && S.ll_len[nlit - 1] == 0) --nlit;
        while (ndist > 1 && S.d_len[ndist - 1] == 0) --ndist;
        for (int s = 0; s < 20; ++s) S.cl_freq[s] = 0;
        const int total = nlit + ndist;
        int nrle = 0, i = 0;
        while (i < total) {
            const int v = i < nlit ? S.ll_len[i] : S.d_len[i - nlit];
            int run = 1;
            while (i + run < total && (i + run < nlit ? S.ll_len[i + run] : S.d_len[i + run - nlit]) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const int r = run < 138 ? run : 138;
                    S.rle_sym[nrle] = 18; S.rle_ext[nrle++] = (uint8_t)(r - 11); ++S.cl_freq[18];
                    run -= r;
                }
                if (run >= 3) {
                    S.rle_sym[nrle] = 17; S.rle_ext[nrle++] = (uint8_t)(run - 3); ++S.cl_freq[17];
                    run = 0;
                }
            } else {
                S.rle_sym[nrle] = (uint8_t)v; S.rle_ext[nrle++] = 0; ++S.cl_freq[v];
                --run;
                while (run >= 3) {
                    const int r = run < 6 ? run : 6;
                    S.rle_sym[nrle] = 16; S.rle_ext[nrle++] = (uint8_t)(r - 3); ++S.cl_freq[16];
                    run -= r;
                }
            }
            for (; run > 0; --run) {
                S.rle_sym[nrle] = (uint8_t)v; S.rle_ext[nrle++] = 0; ++S.cl_freq[v];
            }
        }
        S.bc[0] = (uint32_t)nlit; S.bc[1] = (uint32_t)ndist; S.bc[2] = (uint32_t)nrle;
    }
    limited = build_code(S, S.cl_freq, 19, 7, true, -1, S.cl_len, S.cl_code, L) || limited;
    if (L.lo == 0) {
        int ncode = 19;
        while (ncode > 4 && S.cl_len[code_length_order(ncode - 1)] == 0) --ncode;
        uint32_t bits = 17u + 3u * (uint32_t)ncode;
        for (int s = 0; s < 19; ++s) bits += S.cl_freq[s] * (uint32_t)(S.cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
        for (int s = 0; s < 286; ++s) bits += ll_freq[s] * (uint32_t)(S.ll_len[s] + length_extra_bits(s));
        for (int s = 0; s < 30; ++s) bits += d_freq[s] * (uint32_t)(S.d_len[s] + distance_extra_bits(s));
        S.bc[3] = (uint32_t)ncode;
        S.bc[4] = bits;
    }
    TT_PNG_SYNC();
    return limited;
}

// The block of S.tok[0, ntok) (the end-of-block token included, and counted in S.ll_freq), which covers bytes [from, to) of
// `in`.  Three ways to write it are sized exactly: its LZ77 tokens under their own codes; its bytes as literals only under
// theirs (matches flatten a skewed byte histogram: where the literal/length code of the tokens comes out longer than the
// plain Huffman code of the bytes, the matches do not pay); its bytes stored (behind a header of their own if no stored run
// is pending).  The smallest is taken, the tokens on a tie with the literals, stored on a tie with either (the literal form
// is not sized where a bound says it could win by less than 1 part in 32: below); a stored block is left to the pending
// stored run.  Returns true if the block was written.
TT_HD inline bool finish_block(State& S, Writer& W, Lanes L, const uint8_t* in, int stored_from, int from, int to, int ntok, Stats& stats) {
    TT_PNG_SYNC();
    TT_ENC_LANES(l) {
        for (int i = l; i < 288; i += kLanes) S.lit_freq[i] = i == (int)kEob ? 1u : 0u;
        if (l < 32) S.no_freq[l] = 0;
    }
    TT_PNG_SYNC();
    TT_ENC_LANES(l)
        for (int i = from + l; i < to; i += kLanes) TT_ENC_ADD(&S.lit_freq[in[i]], 1u);
    bool limited = plan_block(S, L, S.ll_freq, S.d_freq);
    const uint32_t token_bits = TT_PNG_UNIFORM(S.bc[4]);
    // Before the literal form is sized (three more codes, as long again as the block has taken so far): a lower bound of its
    // symbols' bits, the entropy of the byte counts with log2(2^e (1 + m)) >= e + m, in 1/256 bit, rounded down everywhere.
    // The literal form is sized only where the bound is more than 1/32 below the tokens' size: it cannot win where the bound
    // is not below, and a win of under 3 % (noisy camera rows, where it would be sized for most blocks and taken for few) is
    // not worth doubling the block's time.
    TT_PNG_SYNC();
    TT_ENC_LANES(l) {
        const uint64_t total = (uint64_t)(to - from) + 1;
        uint64_t sum = 0;
        for (int i = l; i < 257; i += kLanes) {
            const uint64_t f = S.lit_freq[i];
            if (!f) continue;
            const uint64_t q = (total << 8) / f;                  // >= 256
            const int e = 63 - __builtin_clzll(q);
            sum += f * (256ull * (uint64_t)(e - 8) + (((q - (1ull << e)) << 8) >> e));
        }
        S.key[l] = (uint32_t)sum;
        S.sorted[l] = (uint32_t)(sum >> 32);
    }
    TT_PNG_SYNC();
    uint64_t bound = 0;
    for (int l = 0; l < kLanes; ++l) bound += ((uint64_t)TT_PNG_UNIFORM(S.sorted[l]) << 32) | TT_PNG_UNIFORM(S.key[l]);
    bool literal = false;
    if ((bound >> 8) + (token_bits >> 5) < token_bits) {
        const bool literal_limited = plan_block(S, L, S.lit_freq, S.no_freq);
        literal = TT_PNG_UNIFORM(S.bc[4]) < token_bits;
        if (literal) {
            limited = literal_limited;
            ntok = to - from + 1;
        } else {
            limited = plan_block(S, L, S.ll_freq, S.d_freq);      // (its codes again: the literals' have replaced them)
        }
    }
    if (limited) ++stats.limited_blocks;
    const int nlit = (int)TT_PNG_UNIFORM(S.bc[0]), ndist = (int)TT_PNG_UNIFORM(S.bc[1]), nrle = (int)TT_PNG_UNIFORM(S.bc[2]);
    const int ncode = (int)TT_PNG_UNIFORM(S.bc[3]);
    const uint64_t dynamic_bits = TT_PNG_UNIFORM(S.bc[4]);
    const uint64_t stored_bits = 8ull * (uint64_t)(to - from) + (stored_from == from ? 40u : 0u);
    if (dynamic_bits >= stored_bits) return false;

    if (stored_from < from) emit_stored(S, W, L, in, stored_from, from, stats);
    reserve(S, W, L, 17 + 3 * 19 + 14 * 316);
    put(S, W, L, 4u, 3);                                          // BFINAL 0, BTYPE 10
    put(S, W, L, (uint32_t)(nlit - 257), 5);
    put(S, W, L, (uint32_t)(ndist - 1), 5);
    put(S, W, L, (uint32_t)(ncode - 4), 4);
    for (int i = 0; i < ncode; ++i) put(S, W, L, TT_PNG_UNIFORM((uint32_t)S.cl_len[code_length_order(i)]), 3);
    for (int i = 0; i < nrle; ++i) {
        const int s = (int)TT_PNG_UNIFORM((uint32_t)S.rle_sym[i]);
        put(S, W, L, TT_PNG_UNIFORM((uint32_t)S.cl_code[s]), (int)TT_PNG_UNIFORM((uint32_t)S.cl_len[s]));
        if (s >= 16) put(S, W, L, TT_PNG_UNIFORM((uint32_t)S.rle_ext[i]), s == 16 ? 2 : s == 17 ? 3 : 7);
    }
    for (int t0 = 0; t0 < ntok; t0 += kLanes) {
        reserve(S, W, L, 48 * kLanes);
        TT_PNG_SYNC();
        PerLane<uint32_t> nb;
        PerLane<uint64_t> val;
        TT_ENC_LANES(l) {
            uint64_t v = 0;
            int n = 0;
            if (t0 + l < ntok) {
                const uint32_t t = !literal ? S.tok[t0 + l] : t0 + l < to - from ? (uint32_t)in[from + t0 + l] : kEob;
                if (t >> 31) {
                    int ext, extra;
                    const int ls = length_symbol((int)(t & 255u) + kLenBase, ext, extra);
                    v = S.ll_code[ls];
                    n = S.ll_len[ls];
                    v |= (uint64_t)extra << n;
                    n += ext;
                    const int ds = distance_symbol((int)((t >> 8) & 32767u) + 1, ext, extra);
                    v |= (uint64_t)S.d_code[ds] << n;
                    n += S.d_len[ds];
                    v |= (uint64_t)extra << n;
                    n += ext;
                } else {
                    v = S.ll_code[t];
                    n = S.ll_len[t];
                }
            }
            val[l] = v;
            nb[l] = (uint32_t)n;
        }
        const uint32_t total = exclusive_scan(nb, L);
        TT_ENC_LANES(l) {
            or_bits(S, W.nbits + (int)nb[l], val[l], val[l] ? 48 : 0);      // (zero bits are there already)
        }
        W.nbits += (int)total;
    }
    TT_PNG_SYNC();
    ++stats.dynamic_blocks;
    return true;
}

// Bytes in[0, n), n >= 1 -> one segment at out[0, ...): non-final blocks, the last the empty stored block.  Returns its
// size, at most stored_only_bytes(n); nothing is stored at or beyond out[cap] (cap >= segment_slot_bytes(n) holds it all).
// out is 4-byte aligned.  Every argument is the same in every lane.  stats: counted per segment.
TT_HD inline long long deflate_segment(State& S, const uint8_t* in, int n, uint8_t* out, long long cap, Lanes L, Stats& stats) {
    stats.dynamic_blocks = stats.stored_blocks = stats.limited_blocks = 0;
    Writer W;
    W.out = out; W.cap = cap; W.base = 0; W.nbits = 0;
    TT_PNG_SYNC();
    TT_ENC_LANES(l) {
        for (int i = l; i < (1 << kHashBits); i += kLanes) S.hash[i] = 0;
        for (int i = l; i < kOutWords + 2; i += kLanes) S.obuf[i] = 0;
        for (int i = l; i < 288; i += kLanes) S.ll_freq[i] = 0;
        if (l < 32) S.d_freq[l] = 0;
    }
    TT_PNG_SYNC();
    int p = 0, ntok = 0, block_from = 0, stored_from = 0;
    while (p < n) {
        const int cnt = n - p < kLanes ? n - p : kLanes;
        PerLane<int> mlen, mdist, hashed;
        TT_ENC_LANES(l) {
            const int pos = p + l;
            int len = 0, dist = 0;
            hashed[l] = -1;
            if (l < cnt && pos + kMinMatch <= n) {
                const uint32_t h = hash4(in + pos);
                hashed[l] = (int)h;
                const uint32_t c = S.hash[h];
                if (c != 0u && pos - (int)(c - 1) <= kWindow) {
                    const int cand = (int)(c - 1);
                    const int max = n - pos < kMaxMatch ? n - pos : kMaxMatch;
                    const int m = match_length(in + cand, in + pos, max);
                    if (m >= kMinMatch && !(m == kMinMatch && pos - cand > kFar)) {
                        len = m;
                        dist = pos - cand;
                    }
                }
            }
            mlen[l] = len;
            mdist[l] = dist;
            S.mlen[l] = (uint16_t)len;
        }
        const uint64_t M = ballot(mlen, L);
        TT_PNG_SYNC();
        TT_ENC_LANES(l)
            if (hashed[l] >= 0) TT_ENC_MAX(&S.hash[hashed[l]], (uint32_t)(p + l + 1));
        // the greedy resolution, the same in every lane: T = the positions that start a token
        uint64_t T = 0;
        int q = 0;
        while (q < cnt) {
            const uint64_t rest = M >> q;
            if (!rest) {
                T |= bits_below(cnt) & ~bits_below(q);
                q = cnt;
                break;
            }
            const int m = q + __builtin_ctzll(rest);
            T |= bits_below(m + 1) & ~bits_below(q);
            q = m + (int)TT_PNG_UNIFORM((uint32_t)S.mlen[m]);
        }
        TT_ENC_LANES(l) {
            if ((T >> l) & 1u) {
                const int at = ntok + popcount64(T & bits_below(l));
                if (mlen[l] >= kMinMatch) {
                    int ext, extra;
                    S.tok[at] = 0x80000000u | ((uint32_t)(mdist[l] - 1) << 8) | (uint32_t)(mlen[l] - kLenBase);
                    TT_ENC_ADD(&S.ll_freq[length_symbol(mlen[l], ext, extra)], 1u);
                    TT_ENC_ADD(&S.d_freq[distance_symbol(mdist[l], ext, extra)], 1u);
                } else {
                    S.tok[at] = in[p + l];
                    TT_ENC_ADD(&S.ll_freq[in[p + l]], 1u);
                }
            }
        }
        ntok += popcount64(T);
        p += q;
        if (ntok + kLanes + 1 > kBlockTokens || p >= n) {
            TT_PNG_SYNC();
            if (L.lo == 0) {
                S.tok[ntok] = kEob;
                ++S.ll_freq[kEob];
            }
            if (finish_block(S, W, L, in, stored_from, block_from, p, ntok + 1, stats)) stored_from = p;
            block_from = p;
            ntok = 0;
            TT_PNG_SYNC();
            TT_ENC_LANES(l) {
                for (int i = l; i < 288; i += kLanes) S.ll_freq[i] = 0;
                if (l < 32) S.d_freq[l] = 0;
            }
        }
        TT_PNG_SYNC();
    }
    if (stored_from < n) emit_stored(S, W, L, in, stored_from, n, stats);
    emit_stored(S, W, L, in, n, n, stats);
    flush(S, W, L, true);
    if (W.base > stored_only_bytes(n)) {                          // (a dynamic block between stored runs cost the run its merge)
        TT_PNG_SYNC();
        W.base = 0;
        W.nbits = 0;
        stats.dynamic_blocks = stats.stored_blocks = 0;
        emit_stored(S, W, L, in, 0, n, stats);
        emit_stored(S, W, L, in, n, n, stats);
        flush(S, W, L, true);
    }
    return W.base;
}

// -------------------------------------------------------------------------------------------------------------- the file
// signature, IHDR, ttSG (png.py: version 1, R, ceil(H / R), n + 1 big-endian offsets into the IDAT payload, offsets[0] = 2),
// one IDAT with the whole zlib stream (78 01, the segments, 03 00, the Adler-32 of the filtered scanlines), IEND.
constexpr int kTtsgAt = 33;                                      // signature 8, IHDR 12 + 13

struct FileGeom {
    long long stride, expect;           // bytes of a filtered row, of all rows
    int rows, nseg;                     // rows of a full segment (R, at most H), segments
    long long idat_at;                  // of the IDAT chunk's length field
    long long n_full, n_last;           // filtered bytes of a full segment, of the last
};

TT_HD inline FileGeom file_geom(int H, int W, int C, int R) {
    FileGeom g;
    g.stride = 1 + (long long)W * C;
    g.expect = H * g.stride;
    g.rows = R < H ? R : H;
    g.nseg = (H + g.rows - 1) / g.rows;
    g.idat_at = kTtsgAt + 12 + 9 + 4 * ((long long)g.nseg + 1);
    g.n_full = g.rows * g.stride;
    g.n_last = (H - (g.nseg - 1) * g.rows) * g.stride;
    return g;
}

TT_HD inline int segment_rows(const FileGeom& g, int H, int seg) { return seg + 1 < g.nseg ? g.rows : H - (g.nseg - 1) * g.rows; }

// the file's size when its segments' sizes sum to `segments` bytes
TT_HD inline long long file_bytes(const FileGeom& g, long long segments) { return g.idat_at + 12 + 2 + segments + 6 + 12; }

// the largest file an image can become: every segment stored
TT_HD inline long long file_bound(const FileGeom& g, int H) {
    const long long full = stored_only_bytes(g.rows * g.stride), last = stored_only_bytes(segment_rows(g, H, g.nseg - 1) * g.stride);
    return file_bytes(g, (g.nseg - 1) * full + last);
}

TT_HD inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// Everything of the file but the segments, the Adler-32 and the CRC fields of IHDR, ttSG and IDAT (IEND's is a constant):
// serial.  seg_sizes[0, nseg): what deflate_segment returned; seg_at[0, nseg): where each segment goes in the file.  R is
// written to ttSG as given.  Returns the file's size.
TT_HD inline long long write_container(uint8_t* file, int H, int W, int C, int R, const FileGeom& g, const int32_t* seg_sizes, long long* seg_at) {
    const uint8_t head[16] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    for (int i = 0; i < 16; ++i) file[i] = head[i];
    put_be32(file + 16, (uint32_t)W);
    put_be32(file + 20, (uint32_t)H);
    file[24] = 8; file[25] = (uint8_t)(C == 3 ? 2 : 0); file[26] = 0; file[27] = 0; file[28] = 0;
    uint8_t* t = file + kTtsgAt;
    put_be32(t, (uint32_t)(9 + 4 * (g.nseg + 1)));
    t[4] = 't'; t[5] = 't'; t[6] = 'S'; t[7] = 'G';
    t[8] = 1;
    put_be32(t + 9, (uint32_t)R);
    put_be32(t + 13, (uint32_t)g.nseg);
    long long at = 2;
    for (int s = 0; s < g.nseg; ++s) {
        put_be32(t + 17 + 4 * (long long)s, (uint32_t)at);
        seg_at[s] = g.idat_at + 8 + at;
        at += seg_sizes[s];
    }
    put_be32(t + 17 + 4 * (long long)g.nseg, (uint32_t)at);
    uint8_t* d = file + g.idat_at;
    put_be32(d, (uint32_t)(at + 6));
    d[4] = 'I'; d[5] = 'D'; d[6] = 'A'; d[7] = 'T';
    d[8] = 0x78; d[9] = 0x01;
    d[8 + at] = 0x03; d[8 + at + 1] = 0x00;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    uint8_t* e = d + 8 + at + 6 + 4;
    for (int i = 0; i < 12; ++i) e[i] = iend[i];
    return file_bytes(g, at - 2);
}

// ------------------------------------------------------------------------------------------------- the slot table's format
// What file_slots.h asks of a format: the first pass is the filter, a row per unit; the parts are the segments.
struct SlotFormat {
    typedef tt_png_enc_image Image;
    typedef FileGeom Geom;
    TT_HD static Geom geom(const Image& im) { return file_geom(im.height, im.width, im.channels, im.rows_per_segment); }
    TT_HD static int units(const Image& im, const Geom&) { return im.height; }
    TT_HD static int parts(const Geom& g) { return g.nseg; }
    TT_HD static long long first_bytes(const Geom& g) { return g.expect; }
    TT_HD static long long slot_bytes(const Image&, const Geom& g, bool last) { return segment_slot_bytes(last ? g.n_last : g.n_full); }
    // 0 where the table is refused for its sizes
    static long long bound(const Image& im) {
        if ((im.channels != 1 && im.channels != 3) || im.height < 1 || im.width < 1 || im.rows_per_segment < 1) return 0;
        if (im.filter < TT_PNGE_FILTER_NONE || im.filter > TT_PNGE_FILTER_ADAPTIVE) return 0;
        const Geom g = geom(im);
        if (g.rows * g.stride > 2147483647LL - 64) return 0;
        const long long most = file_bound(g, im.height);
        if (most - g.idat_at - 24 > 2147483640LL) return 0;                        // the zlib stream: at most 2^31 - 8 bytes
        return most;
    }
};

}  // namespace tt_pngenc

// The bf16x3 convention, stated once: how an f32 operand becomes a bf16 (hi, lo) pair, where the pair lies in memory, and in which
// order the three bf16 MFMAs of a product are summed.  Every kernel that promises bit-equality with another one (pair-format
// producers against in-kernel splits, seg_chain against two conv launches, conv_x3_up2 against bilinear_up2_pair + conv, the patch
// and pipelined tiles against the 8-wave tiles, sp_conv_l2 against the run-staged kernel, the out_pair epilogue against
// weights.split_pairs_x3) keeps that promise by calling the functions below; the host-side statement of the same layout is
// weights.split_pairs_x3 / split_pairs_frag.
//
// SPLIT.  hi = rne_bf16(x), lo = rne_bf16(x - hi).  The subtraction is exact in f32 (the difference is at most half a bf16 ulp of x
// and a multiple of x's f32 ulp), so hi + lo carries 16 significant bits of x.  On the gfx950 converter a pair of elements takes
// 6 VALU: cvt_pk (both hi), shift and and (the two hi values widened back to f32), two subtractions, cvt_pk (both lo).  split_hi /
// split_lo are its two 3-VALU halves, for the kernels that place them between MFMAs by hand; split8 is a fragment's four pairs.
//
// PAIR FORMAT.  A row of C channels is C / 16 groups of kPairGroupBytes = 64 B: [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15], 16 B each: a
// 16 B chunk is one lane's MFMA fragment (8 bf16 of K), lane half h of a k-step reads hi chunk h and lo chunk h + 2.  The lo half of
// any hi element or chunk therefore lies kPairLo = 32 B further.  Groups are 64 B aligned and a hi offset inside a group is below 32,
// so bit 5 of a hi address is clear and `+ 32` and `^ 32u` name the same byte; the kernels that address LDS through an XOR swizzle of
// the 16 B chunk index write `^ 32u`, which commutes with the swizzle.  (The f16 h2 pair of conv_h2.hip / weights.split_pairs_h2
// shares the 64 B group shape; its split is its own and has one device-side consumer.)
//
// PRODUCT.  a * b ~ a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on v_mfma_f32_32x32x16_bf16 into f32 (a_lo*b_lo, below 2^-16 of the product,
// is dropped).  Two summation orders exist, and each bit-equality promise is between kernels of the same one:
//   * one accumulator, small terms first: c += al*bh, c += ah*bl, c += ah*bh.  The convolutions.  A wave there owns several
//     accumulator blocks and issues each term over all of them before the next term (consecutive MFMAs then write different
//     accumulators), which leaves this order per accumulator.
//   * two accumulators: c2 += al*bh, c += ah*bh, c2 += ah*bl, summed by the epilogue.  The decoder kernels (dec_chain.hip,
//     dec_spatial.hip), whose waves own one or two output blocks, too few to interleave: a back-to-back MFMA pair on one
//     accumulator waits for the first one's last pass.
#pragma once
#include "tt_common.h"

namespace tt {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Mfma;
template <> struct Mfma<float> {
    // one 16 B vector (4 floats) per lane = 4 MFMAs of K=2 (lanes 0-31: k, lanes 32-63: k+4)
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    }
};
template <> struct Mfma<uint16_t> {
    // one 16 B vector (8 bf16) per lane = 1 MFMA of K=16
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                    __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mfma<f16_t> {
    // one 16 B vector (8 halves) per lane = 1 MFMA of K=16, same rate as bf16
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// ---- split
// the two hi values of a packed pair, back in f32
__device__ __forceinline__ float hi0_f32(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ float hi1_f32(uint32_t h) { return __uint_as_float(h & 0xffff0000u); }

// first half of an element pair's split: h = both hi halves packed, t0 / t1 = the two hi values as f32
__device__ __forceinline__ void split_hi(float x0, float x1, uint32_t& h, float& t0, float& t1) {
    h = pack_bf16x2(x0, x1);
    t0 = hi0_f32(h);
    t1 = hi1_f32(h);
}
// second half: both lo halves packed
__device__ __forceinline__ uint32_t split_lo(float x0, float x1, float t0, float t1) { return pack_bf16x2(x0 - t0, x1 - t1); }

// eight f32 (a lane's share of a 16-wide k-step) -> their hi and lo fragments.  The two halves' operations with each subtraction
// behind its own widening, the order the compiler gets them in (split_hi; split_lo widens both first): conv_x3_up2.hip's
// production, scheduled beside another workgroup's MFMAs, comes out as measured only in this one.
__device__ __forceinline__ void split8(const float (&x)[8], uint4& hi, uint4& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
        l[e] = pack_bf16x2(x[2 * e] - hi0_f32(h[e]), x[2 * e + 1] - hi1_f32(h[e]));
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}
// ... from the two raw 16 B fragments that hold them (uint4, u32x4, float4: elements 0-3, 4-7)
__device__ __forceinline__ float frag_f32(float v) { return v; }
__device__ __forceinline__ float frag_f32(uint32_t bits) { return __uint_as_float(bits); }
template <typename V>
__device__ __forceinline__ void split8(const V& r0, const V& r1, uint4& hi, uint4& lo) {
    static_assert(sizeof(V) == 16, "a 16-byte fragment of four f32");
    const float x[8] = {frag_f32(r0.x), frag_f32(r0.y), frag_f32(r0.z), frag_f32(r0.w),
                        frag_f32(r1.x), frag_f32(r1.y), frag_f32(r1.z), frag_f32(r1.w)};
    split8(x, hi, lo);
}
// The same fragment through split_hi / split_lo, pair by pair: the prologue of the hand-pipelined kernels (conv_x3_pipe.hip), whose
// loop places these halves between MFMAs one at a time.  V: a 16-byte vector of four uint32 (u32x4, uint4).
template <typename V>
__device__ __forceinline__ void split8_halves(const V& r0, const V& r1, V& hi, V& lo) {
    static_assert(sizeof(V) == 16, "a 16-byte fragment of four f32");
    const float x[8] = {frag_f32(r0.x), frag_f32(r0.y), frag_f32(r0.z), frag_f32(r0.w),
                        frag_f32(r1.x), frag_f32(r1.y), frag_f32(r1.z), frag_f32(r1.w)};
    uint32_t h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t0, t1;
        split_hi(x[2 * e], x[2 * e + 1], h[e], t0, t1);
        l[e] = split_lo(x[2 * e], x[2 * e + 1], t0, t1);
    }
    hi = V{h[0], h[1], h[2], h[3]};
    lo = V{l[0], l[1], l[2], l[3]};
}

// ---- pair format
constexpr int kPairGroup = 16;        // channels of a group
constexpr int kPairGroupBytes = 64;    // [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15]
constexpr int kPairLo = 32;            // a lo half lies this many bytes after its hi half
static_assert(kPairGroupBytes == kPairGroup * 2 * (int)sizeof(uint16_t), "a group holds a bf16 hi and a bf16 lo per channel");
static_assert(kPairLo == kPairGroup * (int)sizeof(uint16_t) && 2 * kPairLo == kPairGroupBytes, "hi halves first, lo halves behind them");
static_assert((kPairLo & (kPairLo - 1)) == 0, "+ kPairLo == ^ kPairLo on a hi address needs a single bit");

// channel c's hi half inside the pair-format row at `row`, a byte pointer or (pair_at(0, c): the byte offset inside a row) an integer
template <typename B>
__device__ __forceinline__ B pair_at(B row, int c) {
    return row + (c >> 4) * kPairGroupBytes + ((c >> 3) & 1) * 16 + (c & 7) * 2;
}

// one f32 value as the (hi, lo) pair of channel c of a pair-format row (LDS or global)
__device__ __forceinline__ void pair_store(unsigned char* row, int c, float v) {
    const uint16_t hi = f32_to_bf16(v);
    const uint16_t lo = f32_to_bf16(v - bf16_to_f32(hi));
    unsigned char* p = pair_at(row, c);
    *reinterpret_cast<uint16_t*>(p) = hi;
    *reinterpret_cast<uint16_t*>(p + kPairLo) = lo;
}
__device__ __forceinline__ float pair_load(const unsigned char* row, int c) {
    const unsigned char* p = pair_at(row, c);
    return bf16_to_f32(*reinterpret_cast<const uint16_t*>(p)) + bf16_to_f32(*reinterpret_cast<const uint16_t*>(p + kPairLo));
}
// four consecutive channels c .. c + 3 (c % 4 == 0): two 8-byte stores
__device__ __forceinline__ void pair_store4(unsigned char* row, int c, const float4& v) {
    unsigned char* p = pair_at(row, c);
    const uint16_t h0 = f32_to_bf16(v.x), h1 = f32_to_bf16(v.y), h2 = f32_to_bf16(v.z), h3 = f32_to_bf16(v.w);
    const uint16_t l0 = f32_to_bf16(v.x - bf16_to_f32(h0)), l1 = f32_to_bf16(v.y - bf16_to_f32(h1));
    const uint16_t l2 = f32_to_bf16(v.z - bf16_to_f32(h2)), l3 = f32_to_bf16(v.w - bf16_to_f32(h3));
    *reinterpret_cast<uint2*>(p) = make_uint2((unsigned)h0 | ((unsigned)h1 << 16), (unsigned)h2 | ((unsigned)h3 << 16));
    *reinterpret_cast<uint2*>(p + kPairLo) = make_uint2((unsigned)l0 | ((unsigned)l1 << 16), (unsigned)l2 | ((unsigned)l3 << 16));
}
// the split halves of eight consecutive channels (o % 8 == 0) into a pair-format tensor in global memory whose element o -- 4 bytes
// per channel, the footprint of the f32 it replaces -- is `out + o`: two 16-byte stores
__device__ __forceinline__ void pair_store8(float* out, long long o, const uint4& hi, const uint4& lo) {
    float* g = out + (o & ~(long long)(kPairGroup - 1)) + ((o & 8) ? 4 : 0);
    *reinterpret_cast<uint4*>(g) = hi;
    *reinterpret_cast<uint4*>(g + kPairLo / 4) = lo;
}

// ---- product
// one accumulator, small terms first
__device__ __forceinline__ void mfma3(const uint4& ah, const uint4& al, const uint4& bh, const uint4& bl, f32x16& c) {
    Mfma<uint16_t>::run(al, bh, c);
    Mfma<uint16_t>::run(ah, bl, c);
    Mfma<uint16_t>::run(ah, bh, c);
}
// cross terms and main term on two accumulators, summed by the caller's epilogue
__device__ __forceinline__ void mfma3(const uint4& ah, const uint4& al, const uint4& bh, const uint4& bl, f32x16& c, f32x16& c2) {
    Mfma<uint16_t>::run(al, bh, c2);
    Mfma<uint16_t>::run(ah, bh, c);
    Mfma<uint16_t>::run(ah, bl, c2);
}

}  // namespace tt

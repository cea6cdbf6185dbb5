// Implicit-GEMM convolution, LDS-DMA pipelined kernel (gfx950 `global_load_lds_dwordx4`).
//
// Same math and epilogue as conv_igemm.hip; different data movement.  Carries every large dense layer of the
// camera trunk / SECOND / decoder value projections, the 7x7/2 stem in row-run form, and (GATHER) the sparse 3D
// convolutions of the LiDAR encoder:
//   * block tile 256 x {256, 128, 64, 32}, 4 or 8 waves with 64x64 or 128x64 register tiles (template parameters;
//     conv_choose.cpp states which shape gets which and why).
//   * global -> LDS by DMA (no staging VGPRs).  STAGES = 3: tile k+2 is issued right after the barrier that
//     publishes tile k, with a COUNTED `s_waitcnt vmcnt(N)` (never 0 in the main loop) and a raw `s_barrier`, so
//     two K tiles of loads overlap the MFMA phase (64 B rows).  STAGES = 2: one tile in flight, 128 B rows =
//     whole cache lines per DMA lane group (the faster choice wherever 2 x tile fits the LDS budget).
//   * K order: channel chunk outer, filter tap inner (dense); natural [tap][channel] order, 1-4 taps per 128 B
//     row, rulebook entries fetched one tile ahead (gather).
//   * the pieces shared with the kernels derived from this one are defined in conv_lds_dma.h: per DMA slot ONE precomputed
//     pointer (tap (0,0)) and ONE tap-validity bitmask, the XOR swizzle applied to the DMA SOURCE address, the zero page that
//     rows which are padding / beyond M / beyond K read instead of branching, the XCD-aware tile order.
// Requires: Cin % BK == 0 (dense: one tap per K tile) or power-of-two Cin >= 16 (gather); KH*KW <= 32; no split-K.
#include "conv_lds_dma.h"

namespace tt {

// Timing experiments only (tools/conv_microbench.py, TT_MB_ACT=97/98 on the 2-stage variants): skip the weight /
// activation DMA after the first K tile to see how much of the loop time is the L2->LDS stream.  0 in the product.
#ifndef TT_GLDS_DEBUG
#define TT_GLDS_DEBUG 0
#endif

// X3 (T = float, 128 B rows): "bf16x3" arithmetic on f32 storage.  Activations stay f32 in HBM / LDS and are split
// into a bf16 (hi, lo) pair per element when a wave loads its A fragment; the weights arrive pre-split (per 16
// K elements 64 B = [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15], thinktwice_amd/weights.py::split_pairs_x3, same
// footprint as f32).  Each product is three v_mfma_f32_32x32x16_bf16: a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with f32
// accumulation -- 16 mantissa bits per operand (relative error ~1e-5 per dot product instead of bf16's 4e-3) at
// 16/3 of the exact-f32 MFMA rate.  This is the precision mode whose outputs meet the 1e-3 tolerance.
// APAIR (X3 only): the ACTIVATIONS arrive pre-split too -- the tensor holds, per 16 channels, 64 B = [hi c0-7 | hi c8-15 | lo c0-7 |
// lo c8-15] in bf16 (the weights' pair format along the channel axis, same footprint as f32), written by the producer's epilogue
// (tt_conv_desc.out_pair) or by an elementwise producer (tt_bilinear_up2_pair).  The hi / lo values are the ones the split of bf16x3.h computes,
// so the sums are bit-identical; what disappears is the split itself: 6 VALU per element pair per USE (a 3 x 3 layer splits every
// input element 9 x per column tile) against once per element at the producer.  For tensors whose ONLY readers are bf16x3 convolutions.
template <typename T, int BN, int WAVES_M, int WAVES_N, int BKB, int STAGES = 3, bool GATHER = false, bool X3 = false, bool APAIR = false>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64,
                             ((256 / WAVES_M / 32) * (BN / WAVES_N / 32) >= 16)  ? 1      // 128x128 per wave: 512 regs
                             : ((256 / WAVES_M / 32) * (BN / WAVES_N / 32) >= 8) ? 2      // 128x64 per wave: 256 regs
                             : (WAVES_M * WAVES_N == 16 || BKB == 64)            ? 4
                                                                                 : 2)
void conv_igemm_glds_kernel(const ConvArgs p, const void* zero_page,
                                                              int tiles_m, int tiles_n) {
#if defined(__HIP_DEVICE_COMPILE__)   // amdgcn builtins / inline asm: keep the x86 host pass away from the body
    constexpr int BM = 256;
    constexpr int VEC = Elem<T>::kVec;
    constexpr int BK = BKB / (int)sizeof(T);          // BKB = K bytes per row per tile (64 or 128)
    constexpr int CPR = BKB / 16;                     // 16 B chunks per row
    // STAGES = 23: asymmetric ring -- THREE activation stages, TWO weight stages (x3 256x256 tile: 3 x 32 + 2 x 32 KiB =
    // the whole 160 KiB).  The weight tiles are L2-resident for every workgroup of the launch; the activation tiles are the
    // ones that miss (one tap in nine), so they get the second tile of lookahead.
    constexpr bool ASYM = STAGES == 23;
    constexpr int SA = ASYM ? 3 : STAGES, SB = ASYM ? 2 : STAGES;
    static_assert(STAGES == 2 || STAGES == 3 || ASYM, "2 or 3 LDS stages, or 23 = 3 activation + 2 weight stages");
    static_assert(!GATHER || STAGES == 2, "gather mode is written for the 2-stage pipeline");
    constexpr int A_BYTES = BM * BKB, B_BYTES = BN * BKB;
    constexpr int STAGE_BYTES = (BM + BN) * BKB;
    // byte offset of tile kt's activation / weight stage from the start of the dynamic LDS
    auto off_a = [](int kt) { return ASYM ? (kt % 3) * A_BYTES : (kt % SA) * STAGE_BYTES; };
    auto off_b = [](int kt) { return ASYM ? 3 * A_BYTES + (kt % 2) * B_BYTES : (kt % SB) * STAGE_BYTES + A_BYTES; };
    constexpr int NA_INSTR = BM * CPR / 64;           // 1 KiB wave-instructions in the A tile
    constexpr int NB_INSTR = BN * CPR / 64;
    constexpr int NW = WAVES_M * WAVES_N;             // waves per workgroup (8 or 16)
    constexpr int NIA = NA_INSTR / NW;                // A wave-instructions per wave per tile
    constexpr int NIB = (NB_INSTR + NW - 1) / NW;     // B  " (when NB_INSTR < NW some waves re-load a chunk
                                                      //       another wave also loads: same bytes, harmless,
                                                      //       and every wave keeps the same vmcnt arithmetic)
    constexpr int LPT = NIA + NIB;                    // DMA loads per thread per tile
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(!X3 || (sizeof(T) == 4 && BKB == 128), "x3: f32 storage, 128 B rows");
    static_assert(!APAIR || (X3 && !GATHER), "pre-split activations: dense bf16x3 only");
    static_assert(NW == 4 || NW == 8 || NW == 16, "4, 8 or 16 waves");
    static_assert(NA_INSTR % NW == 0 && NIA >= 1 && NIB >= 1, "tile too small for the wave count");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    int Mlim = p.M;
    if (GATHER && p.m_dev) {           // sparse conv: live output rows are only known on the device
        const int md = *p.m_dev;
        Mlim = md < Mlim ? md : Mlim;
    }
    // sparse launches cover the ALLOCATED rows: the tile order is dealt over the live row tiles only
    const int live_m = (GATHER && p.m_dev) ? (Mlim - p.m_begin + BM - 1) / BM : tiles_m;
    const int nblk = (live_m < tiles_m ? (live_m > 0 ? live_m : 0) : tiles_m) * tiles_n;
    if ((int)blockIdx.x >= nblk) return;               // block-uniform, before any barrier
    const int L = xcd_tile(nblk);
    const int tile_n = L % tiles_n, tile_m = L / tiles_n;
    const int m0 = p.m_begin + tile_m * BM, n0 = tile_n * BN;
    if (m0 >= Mlim) return;            // block-uniform, before any barrier
    long long* const tr = (p.trace && tid == 0 && blockIdx.y == 0) ? p.trace + (long long)blockIdx.x * 4 : nullptr;
    if (tr) tr[0] = (long long)wall_clock64();

    const T* __restrict__ in = reinterpret_cast<const T*>(p.in);
    const T* __restrict__ wgt = reinterpret_cast<const T*>(p.weight);
    const T* zp = reinterpret_cast<const T*>(zero_page);

    // ---- per-thread DMA slots: A slot j covers LDS chunk g = (wave + NW*j)*64 + lane of the A tile.  Dense: one pointer + one
    // tap mask (dense_slot).  GATHER: the chunk's element offset inside the K tile, the slot's rulebook row and whether it is live
    int a_c[NIA];
    long long a_base[NIA];
    bool a_ok[NIA];
    const T* a_ptr[NIA];
    unsigned a_mask[NIA];
#pragma unroll
    for (int j = 0; j < NIA; ++j) {
        const int g = (wave + NW * j) * 64 + lane;
        if constexpr (GATHER) {
            const int row = g / CPR, pos = g % CPR;
            a_c[j] = (pos ^ swz<BKB>(row)) * VEC;
            a_ok[j] = m0 + row < Mlim;
            const int mm = a_ok[j] ? m0 + row : 0;
            // with a tile plan the tile's slot `mm` stands for output row row_perm[mm]
            a_base[j] = (long long)((p.row_perm && a_ok[j]) ? p.row_perm[mm] : mm) * p.KW;
        } else {
            dense_slot<BKB>(p, in, g, m0, Mlim, a_ptr[j], a_mask[j]);
        }
    }
    int b_c[NIB];
    long long b_base[NIB];
    bool b_ok[NIB];
    const T* b_ptr[NIB];
#pragma unroll
    for (int j = 0; j < NIB; ++j) {
        const int g = ((wave + NW * j) % NB_INSTR) * 64 + lane;
        const int row = g / CPR, pos = g % CPR;
        b_c[j] = (pos ^ swz<BKB>(row)) * VEC;
        b_ok[j] = (n0 + row) < p.Cout;
        b_base[j] = (long long)(n0 + row) * p.K;
        b_ptr[j] = wgt + b_base[j] + b_c[j];
    }

    int nk = (p.K + BK - 1) / BK;

    // Dense: K order of conv_lds_dma.h (KWalk).  GATHER (sparse conv) walks K in natural [tap][channel] order; a K tile covers BK/Cin taps when Cin < BK
    // (each 16 B chunk of a row then comes from its own tap's input row) or a BK-channel slice of one tap.
    // Cin is a power of two there (dispatcher): tap / channel by shift and mask, not integer division.
    int g_cur[NIA];                                    // rulebook entries of the next tile to issue
    int g_t = 0;                                       // K tile of the next rulebook fetch
    const int cin_shift = 31 - __clz(p.Cin), cin_mask = p.Cin - 1;
    // Tile plan (tt_sp_tile_plan): the rows of this tile were sorted by tap mask, so the tile only walks the UNION of
    // their taps.  K tile t of the compact walk covers tap(s) "the (t*TPT + s)-th set bit of the union" (TPT taps per
    // 128 B row when Cin < BK) or one BK-channel slice of one tap (Cin >= BK).  Both walkers below (rulebook fetch, one
    // tile ahead; DMA issue) pop the same bit sequence; everything is wave-uniform scalar work.
    constexpr int TPTMAX = 4;
    const bool planned = GATHER && p.row_mask != nullptr;
    unsigned umask = 0;
    if (planned) {
        unsigned* uw = reinterpret_cast<unsigned*>(smem);
        if (tid == 0) *uw = 0u;
        __syncthreads();
        if (tid < BM && m0 + tid < Mlim) atomicOr(uw, p.row_mask[m0 + tid]);
        __syncthreads();
        umask = *uw;
        __syncthreads();                               // every wave has read it before the first DMA lands there
        umask = __builtin_amdgcn_readfirstlane(umask);
        const int nt = __popc(umask);
        nk = p.Cin >= BK ? nt * (p.Cin / BK) : (nt * p.Cin + BK - 1) / BK;
    }
    struct TapWalk {
        unsigned rem;
        int sub, cur;
    };
    TapWalk wf{umask, 0, -1}, wi{umask, 0, -1};
    auto next_taps = [&](TapWalk& w, int (&tp)[TPTMAX]) {
        if (p.Cin >= BK) {
            if (w.sub == 0) {
                w.cur = w.rem ? __builtin_ctz(w.rem) : -1;
                w.rem &= w.rem - 1;
            }
            tp[0] = w.cur;
            if (++w.sub == p.Cin / BK) w.sub = 0;
        } else {
            const int tpt = BK >> cin_shift;           // taps per K tile (<= TPTMAX, dispatcher)
#pragma unroll
            for (int i = 0; i < TPTMAX; ++i) {
                tp[i] = -1;
                if (i < tpt && w.rem) {
                    tp[i] = __builtin_ctz(w.rem);
                    w.rem &= w.rem - 1;
                }
            }
        }
    };
    auto pick = [&](const int (&tp)[TPTMAX], int slot) {    // tap of 16 B chunk `slot` (= element offset >> cin_shift)
        int t = tp[0];
#pragma unroll
        for (int i = 1; i < TPTMAX; ++i) t = (slot == i) ? tp[i] : t;
        return t;
    };
    auto fetch_rulebook = [&]() {
        if (planned) {
            int tp[TPTMAX];
            next_taps(wf, tp);
#pragma unroll
            for (int j = 0; j < NIA; ++j) {
                const int t = p.Cin >= BK ? tp[0] : pick(tp, a_c[j] >> cin_shift);
                g_cur[j] = (a_ok[j] && t >= 0) ? p.gather[a_base[j] + t] : -1;
            }
            ++g_t;
            return;
        }
#pragma unroll
        for (int j = 0; j < NIA; ++j) {
            const int k = g_t * BK + a_c[j];
            g_cur[j] = (a_ok[j] && k < p.K) ? p.gather[a_base[j] + (k >> cin_shift)] : -1;
        }
        ++g_t;
    };
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const unsigned lds_dma_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    KWalk wa{0, 0, 0}, wb{0, 0, 0};
    if (!GATHER && p.splits > 1) {
        // split-K (few rows, long K: gridDim.y K ranges): this workgroup owns K tiles [kt0, kt1) of the (channel chunk outer, tap
        // inner) walk -- both walkers start there, the ring and the loop below count from 0; the epilogue stores the raw partial
        // sums into slice blockIdx.y of the workspace (conv_epilogue's p.ws branch), splitk_finalize_kernel adds the slices
        const int per = (nk + p.splits - 1) / p.splits;
        const int kt0 = (int)blockIdx.y * per;
        int kt1 = kt0 + per;
        kt1 = kt1 < nk ? kt1 : nk;
        const int taps = p.KH * p.KW;
        const int chunk = kt0 / taps, tap = kt0 - chunk * taps;
        wa.ci = wb.ci = chunk * BK;
        wa.kh = wb.kh = tap / p.KW;
        wa.kw = wb.kw = tap - (tap / p.KW) * p.KW;
        nk = kt1 > kt0 ? kt1 - kt0 : 0;
    }
    auto issue_a = [&](int kt) {
        const unsigned st = lds_dma_base + (unsigned)off_a(kt);
        const int kh = wa.kh, kw = wa.kw, ci = wa.ci;
        const int k0 = kt * BK;                        // GATHER: position of this tile in the [KH][KW][Cin] weight row
        // wave-uniform (SALU): tap index and the element offset of tap (kh, kw), channel ci from tap (0, 0), channel 0
        const int tap = kh * p.KW + kw;
        const long long tap_off = ((long long)(kh * p.dil) * p.W + kw * p.dil) * p.in_cstride + ci;
        advance<BK>(wa, p);
        const bool dbg_skip_a = TT_GLDS_DEBUG && p.act == 98 && kt > 0;
#pragma unroll
        for (int j = 0; j < NIA; ++j) {
            if (dbg_skip_a) break;
            const T* src;
            if (GATHER) {
                // sparse conv: the activation row of (output row, tap) comes from the rulebook entry that was
                // fetched one iteration ago (g_cur), so the DMA does not sit behind a dependent index load
                const int gi = g_cur[j];
                const int kl = k0 + a_c[j];
                src = gi >= 0 ? in + (long long)gi * p.in_cstride + p.in_coff + (kl & cin_mask) : zp;
            } else {
                src = ((a_mask[j] >> tap) & 1u) ? a_ptr[j] + tap_off : zp;
            }
            dma_piece(src, st + (unsigned)(wave_s + NW * j) * 1024u);
        }
    };
    auto issue_b = [&](int kt) {
        const unsigned st = lds_dma_base + (unsigned)off_b(kt);
        const int k0 = GATHER ? kt * BK                // position of this tile in the [KH][KW][Cin] weight row
                              : (wb.kh * p.KW + wb.kw) * p.Cin + wb.ci;
        advance<BK>(wb, p);
        const bool dbg_skip_b = TT_GLDS_DEBUG && p.act == 97 && kt > 0;
        int tpi[TPTMAX];
        if (planned) next_taps(wi, tpi);
#pragma unroll
        for (int j = 0; j < NIB; ++j) {
            if (dbg_skip_b) break;
            // dense: K % BK == 0 (Cin % BK == 0); gather: the last K tile may be ragged (27 taps of 16/32 channels)
            bool ok = b_ok[j] && (!GATHER || (k0 + b_c[j] < p.K));
            const T* src = ok ? b_ptr[j] + k0 : zp;
            if (planned) {      // compact walk: weight row offset = tap * Cin + channel
                const int t = p.Cin >= BK ? tpi[0] : pick(tpi, b_c[j] >> cin_shift);
                ok = b_ok[j] && t >= 0;
                src = ok ? b_ptr[j] - b_c[j] + (long long)t * p.Cin + ((k0 + b_c[j]) & cin_mask) : zp;
            }
            dma_piece(src, st + (unsigned)((wave_s + NW * j) % NB_INSTR) * 1024u);
        }
    };
    auto issue_tile = [&](int kt) {
        issue_a(kt);
        issue_b(kt);
    };
    // what goes out right after the barrier of tile kt
    auto issue_ahead = [&](int kt) {
        if (ASYM) {
            if (kt + 1 < nk) issue_b(kt + 1);          // weights first: the counted wait at the next tile's top lets the
            if (kt + 2 < nk) issue_a(kt + 2);          // younger activation loads stay in flight
        } else if (kt + STAGES - 1 < nk) {
            issue_tile(kt + STAGES - 1);
        }
    };

    // The same DMA, one instruction at a time (dense bf16x3 body; conv_lds_dma.h "spread").  Order of issue is unchanged (weights
    // of tile kt+1, then activations of kt+2), so the counted waits at the top of the next tile still hold.
    auto a_begin = [&](int kt, bool on) { return dma_begin_a<BK>(p, wa, lds_dma_base + (unsigned)off_a(kt), on); };
    auto b_begin = [&](int kt, bool on) { return dma_begin_b<BK, 1>(p, wb, lds_dma_base + (unsigned)off_b(kt), on); };
    auto a_emit = [&](const DmaCtx& c, int j) { dma_emit_a(c, a_ptr[j], a_mask[j], zp, wave_s + NW * j); };
    auto b_emit = [&](const DmaCtx& c, int j) { dma_emit_b(c, b_ptr[j], b_ok[j], zp, (wave_s + NW * j) % NB_INSTR); };

    f32x16 acc[TM][TN];
    zero_acc(acc);

    if (GATHER && nk > 0) fetch_rulebook();
    if (nk > 0) issue_tile(0);
    if (GATHER && nk > 1) fetch_rulebook();            // for tile 1; lands while tile 0 streams in
    if (STAGES == 3 && nk > 1) issue_tile(1);
    if (ASYM && nk > 1) issue_a(1);

    // fragment addressing: row = tile row + (lane&31); 16 B chunk c16 = 2*kc + (lane>>5), swizzled -- conv_lds_dma.h's frag_off with the
    // row term and the swizzle term of a row kept apart (written through frag_off, the first tile's block of 20 of these kernels came
    // out of the compiler with other instruction counts; this form leaves every MFMA block as it was)
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned fa_off[TM], fb_off[TN], fa_s[TM], fb_s[TN];
    const unsigned hi = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 32 + (lane & 31);
        fa_off[i] = row * BKB;
        fa_s[i] = swz<BKB>(row);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 32 + (lane & 31);
        fb_off[j] = BM * BKB + row * BKB;
        fb_s[j] = swz<BKB>(row);
    }
    // X3: a k-step is 16 f32 = 64 B.  A: lane half h owns floats 8h..8h+7 = chunks 4kc+2h and 4kc+2h+1 (the second is
    // the first with address bit 4 flipped, the swizzle being an XOR); B: hi chunk 4kc+h, lo chunk 4kc+2+h (bit 5).
    constexpr int NKC_ = X3 ? BKB / 64 : BKB / 32;
    // spread DMA issue (below): 256-wide tiles only -- a 64 x 128 wave tile has 6 MFMAs (192 cycles) per sub-step to put one
    // 16-cycle DMA piece behind; the narrow tiles' 3-MFMA sub-steps do not cover the texture path's time for 8 waves' pieces
    // (measured +3 % on them)
    const bool spread = BN == 256;
    unsigned fa_pre[NKC_][TM], fb_pre[NKC_][TN];
#pragma unroll
    for (int kc = 0; kc < NKC_; ++kc) {
        const unsigned ca = X3 ? (APAIR ? 4u * kc + hi : 4u * kc + 2u * hi) : 2u * kc + hi;    // APAIR: hi chunk; lo chunk = ^ 32
        const unsigned cb = X3 ? 4u * kc + hi : 2u * kc + hi;
#pragma unroll
        for (int i = 0; i < TM; ++i) fa_pre[kc][i] = fa_off[i] + ((ca ^ fa_s[i]) << 4);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb_pre[kc][j] = fb_off[j] + ((cb ^ fb_s[j]) << 4);
    }

    for (int kt = 0; kt < nk; ++kt) {
        // tile kt has landed for THIS wave once at most one younger tile (LPT loads) is outstanding
        if (ASYM && kt + 1 < nk) wait_vmcnt<NIA>();                 // outstanding in issue order: A(kt) B(kt) A(kt+1)
        else if (STAGES == 3 && kt + 1 < nk) wait_vmcnt<LPT>();
        else wait_vmcnt<0>();
        asm volatile("s_barrier" ::: "memory");   // publishes tile kt; everyone is done reading tile kt-1
        if (tr && kt == 0) tr[1] = (long long)wall_clock64();

        // fragment offsets carry the activation / weight split of a symmetric stage (weights at + A_BYTES): the two bases
        // below make the same offsets address the asymmetric ring
        const unsigned sbase_a = lds_base + (unsigned)off_a(kt);
        const unsigned sbase_b = lds_base + (unsigned)(off_b(kt) - A_BYTES);
        const unsigned sbase = sbase_a;
        if constexpr (X3) {
            // bf16x3 body.  A k-step is 16 f32 of K: 2 reads per A fragment (raw f32), the split (6 VALU per element
            // pair, once per k-step, up front), then per output column block j: 2 reads (weights hi, lo) and 3 MFMAs per row
            // block.  The walk over (k-step, j) is software-pipelined inside the tile: the reads of sub-step s+1 are
            // issued before the MFMAs of sub-step s, into the registers sub-step s-1 has released (one B fragment pair
            // per buffer keeps the 64 x 128 wave tile inside 256 registers).
            constexpr int NS = NKC_ * TN;
            u32x4 ra0[TM], ra1[TM], bh[2], bl[2];
            uint4 ah[2][TM], al[2][TM];
            auto split_frag = [&](int i, uint4& hi_out, uint4& lo_out) {
                asm volatile("" : "+v"(ra0[i]));
                asm volatile("" : "+v"(ra1[i]));
                if (APAIR || (TT_GLDS_DEBUG && p.act == 96)) {   // pre-split activations: ra0 = hi, ra1 = lo (debug 96: raw bits)
                    hi_out = __builtin_bit_cast(uint4, ra0[i]);
                    lo_out = __builtin_bit_cast(uint4, ra1[i]);
                    return;
                }
                split8(ra0[i], ra1[i], hi_out, lo_out);
            };
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ra0[i] = lds_read(sbase + fa_pre[0][i]);
                ra1[i] = lds_read(sbase + (fa_pre[0][i] ^ (APAIR ? 32u : 16u)));
            }
            bh[0] = lds_read(sbase_b + fb_pre[0][0]);
            bl[0] = lds_read(sbase_b + (fb_pre[0][0] ^ 32u));
            constexpr bool SPREAD = !GATHER;
            constexpr int PER = (NIA + NIB + NS - 1) / NS;         // DMA pieces per sub-step
            DmaCtx ca{0u, 0, 0, false}, cb{0u, 0, 0, false};
            if constexpr (SPREAD) {
                if (spread) {
                    // first pieces issued: weights (ASYM: of tile kt+1; else of kt+STAGES-1, after its activations)
                    if (ASYM) {
                        cb = b_begin(kt + 1, kt + 1 < nk);
                        ca = a_begin(kt + 2, kt + 2 < nk);
                    } else {
                        ca = a_begin(kt + STAGES - 1, kt + STAGES - 1 < nk);
                        cb = b_begin(kt + STAGES - 1, kt + STAGES - 1 < nk);
                    }
                } else {
                    issue_ahead(kt);
                }
            } else {
                issue_ahead(kt);
                if (kt + 2 < nk) fetch_rulebook();
            }
#pragma unroll
            for (int ss = 0; ss < NS; ++ss) {
                const int kc = ss / TN, j = ss % TN, buf = ss & 1, ab = kc & 1;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                asm volatile("" : "+v"(bh[buf]));
                asm volatile("" : "+v"(bl[buf]));
                if constexpr (SPREAD) {
                    if (spread) {
                        // this sub-step's share of the next tile's DMA (no LDS read is in flight here: the compiler's
                        // lgkmcnt(0) in front of a global_load_lds costs nothing)
#pragma unroll
                        for (int q = ss * PER; q < (ss + 1) * PER && q < NIA + NIB; ++q) {
                            if (ASYM) {
                                if (q < NIB) { if (cb.on) b_emit(cb, q); }
                                else if (ca.on) a_emit(ca, q - NIB);
                            } else {
                                if (q < NIA) { if (ca.on) a_emit(ca, q); }
                                else if (cb.on) b_emit(cb, q - NIA);
                            }
                        }
                    }
                }
                if (j == 0) {    // the k-step's activation fragments: split up front
#pragma unroll
                    for (int i = 0; i < TM; ++i) split_frag(i, ah[ab][i], al[ab][i]);
                }
                // reads under this sub-step's MFMAs: the next sub-step's weight pair, and the next k-step's activations
                if (j == TN - 1 && kc + 1 < NKC_) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        ra0[i] = lds_read(sbase + fa_pre[kc + 1][i]);
                        ra1[i] = lds_read(sbase + (fa_pre[kc + 1][i] ^ (APAIR ? 32u : 16u)));
                    }
                }
                if (ss + 1 < NS) {
                    const int kc2 = (ss + 1) / TN, j2 = (ss + 1) % TN;
                    if (!(TT_GLDS_DEBUG && p.act == 95)) {   // debug 95: weight fragments read once per tile
                        bh[buf ^ 1] = lds_read(sbase_b + fb_pre[kc2][j2]);
                        bl[buf ^ 1] = lds_read(sbase_b + (fb_pre[kc2][j2] ^ 32u));
                    } else {
                        bh[buf ^ 1] = bh[buf];
                        bl[buf ^ 1] = bl[buf];
                    }
                }
                const uint4 bhv = __builtin_bit_cast(uint4, bh[buf]);
                const uint4 blv = __builtin_bit_cast(uint4, bl[buf]);
                // term-major order: consecutive MFMAs write different accumulators (a back-to-back pair on the same
                // accumulator waits for the first one's last pass); per accumulator the one-accumulator order of bf16x3.h
                if (!(TT_GLDS_DEBUG && p.act == 94)) {       // debug 94: one MFMA per fragment pair instead of three
#pragma unroll
                    for (int i = 0; i < TM; ++i) Mfma<uint16_t>::run(al[ab][i], bhv, acc[i][j]);
#pragma unroll
                    for (int i = 0; i < TM; ++i) Mfma<uint16_t>::run(ah[ab][i], blv, acc[i][j]);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) Mfma<uint16_t>::run(ah[ab][i], bhv, acc[i][j]);
            }
            continue;
        }
        constexpr int NKC = BKB / 32;
        u32x4 fa[2][TM], fb[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[0][i] = lds_read(sbase + fa_pre[0][i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[0][j] = lds_read(sbase_b + fb_pre[0][j]);
        // the next tile's DMA goes out AFTER the first fragment reads: its address arithmetic (~90 VALU/SALU) then
        // runs under the LDS latency instead of in front of it (every wave of the block is in this phase together,
        // so nothing else would cover that latency)
        issue_ahead(kt);
        if (GATHER && kt + 2 < nk) fetch_rulebook();   // for tile kt+2, consumed at the top of the next iteration
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            const int cur = kc & 1, nxt = cur ^ 1;
            // wait for the fragments of step kc; tie the wait to the registers the MFMAs read
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // volatile asms stay in order: these empty ones come after the wait, and the MFMAs below
            // consume their outputs, so no MFMA can be scheduled above the wait
#pragma unroll
            for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(fa[cur][i]));
#pragma unroll
            for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(fb[cur][j]));
            if (kc + 1 < NKC) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[nxt][i] = lds_read(sbase + fa_pre[kc + 1][i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[nxt][j] = lds_read(sbase_b + fb_pre[kc + 1][j]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const uint4 av = __builtin_bit_cast(uint4, fa[cur][i]);
                    const uint4 bv = __builtin_bit_cast(uint4, fb[cur][j]);
                    Mfma<T>::run(av, bv, acc[i][j]);
                }
        }
    }
    // Measured and NOT kept (profiles/r01_conv_microbench_tiles.txt): deferring each tile's last k-step past the next
    // barrier (to cover the prologue bubble) changed nothing, and skipping either DMA stream after the first tile
    // (TT_GLDS_DEBUG) did not shorten the loop either: at ~1.0 PF the loop is neither L2->LDS- nor bubble-bound.
    __syncthreads();   // all waves done with the last stage before the epilogue reuses LDS
    if (tr) tr[2] = (long long)wall_clock64();
    conv_epilogue<T, TM, TN, WTM, WTN>(p, acc, smem, wave, lane, wm, wn, m0, n0, Mlim);
    if (p.trace && blockIdx.y == 0) {                                               // block-uniform: every wave takes the barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                                            // (trace only) the slowest wave's epilogue
        if (tr) tr[3] = (long long)wall_clock64();
    }
#endif
}

template <typename T, int BN, int WAVES_M, int WAVES_N, int BKB, int STAGES = 3, bool GATHER = false, bool X3 = false, bool APAIR = false>
static int launch_glds(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    constexpr int BM = 256;
    constexpr int WTN = BN / WAVES_N;
    // rows [m_begin, M) by default; c.main_rows > 0 (tail split) restricts the launch to that many row tiles from m_begin
    int tiles_m = div_up(a.M - a.m_begin, BM);
    if (c.main_rows > 0 && c.main_rows < tiles_m) tiles_m = c.main_rows;
    const int tiles_n = div_up(a.Cout, BN);
    size_t smem = STAGES == 23 ? (size_t)(3 * BM + 2 * BN) * BKB : (size_t)STAGES * (BM + BN) * BKB;
    const size_t epi = (size_t)(WAVES_M * WAVES_N) * 32 * (WTN + 4) * 4;
    if (smem < epi) smem = epi;
    // split-K: a.ws / a.ws_slices are the caller's (ordered slices, c.slices non-empty ranges)
    return launch_lds_dma(conv_igemm_glds_kernel<T, BN, WAVES_M, WAVES_N, BKB, STAGES, GATHER, X3, APAIR>,
                          dim3((unsigned)(tiles_m * tiles_n), (unsigned)(c.splits > 1 ? c.slices : 1)), dim3(WAVES_M * WAVES_N * 64), smem,
                          smem, "conv_igemm_glds_kernel", a, st, tiles_m, tiles_n, c.splits);
}

// the tile variants this file instantiates: a choice naming one of them launches it
#define TT_GLDS_VARIANT(T, BN, WM, WN, BKB, ST, G, X3, AP)                                                                          \
    if (c.bn == BN && c.waves_m == WM && c.waves_n == WN && c.bkb == BKB && c.stages == ST && c.gather == G && c.x3 == X3 && c.apair == AP) \
        return launch_glds<T, BN, WM, WN, BKB, ST, G, X3, AP>(c, a, st);

// T16 = uint16_t (bf16) or f16_t (IEEE half): same tiles, same MFMA rate.
template <typename T16>
static int launch_glds16(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    TT_GLDS_VARIANT(T16, 32, 8, 1, 128, 2, true, false, false)
    TT_GLDS_VARIANT(T16, 64, 8, 1, 128, 2, true, false, false)
    TT_GLDS_VARIANT(T16, 128, 4, 2, 128, 2, true, false, false)
    TT_GLDS_VARIANT(T16, 256, 2, 4, 128, 2, false, false, false)
    TT_GLDS_VARIANT(T16, 256, 2, 4, 64, 3, false, false, false)
    TT_GLDS_VARIANT(T16, 128, 2, 2, 64, 3, false, false, false)
    TT_GLDS_VARIANT(T16, 128, 4, 2, 64, 3, false, false, false)
    TT_GLDS_VARIANT(T16, 64, 8, 1, 128, 2, false, false, false)
    TT_GLDS_VARIANT(T16, 64, 8, 1, 64, 3, false, false, false)
    return 0;
}

static int launch_glds32(const ConvChoice& c, ConvArgs& a, hipStream_t st) {
    TT_GLDS_VARIANT(float, 128, 4, 2, 64, 3, false, false, false)
    TT_GLDS_VARIANT(float, 64, 8, 1, 64, 3, false, false, false)
    // bf16x3 (a.weight = the pre-split weights): gathered, dense, dense with pre-split activations
    TT_GLDS_VARIANT(float, 32, 8, 1, 128, 2, true, true, false)
    TT_GLDS_VARIANT(float, 64, 8, 1, 128, 2, true, true, false)
    TT_GLDS_VARIANT(float, 128, 8, 1, 128, 2, true, true, false)
    TT_GLDS_VARIANT(float, 32, 8, 1, 128, 2, false, true, false)
    TT_GLDS_VARIANT(float, 64, 8, 1, 128, 2, false, true, false)
    TT_GLDS_VARIANT(float, 128, 8, 1, 128, 2, false, true, false)
    TT_GLDS_VARIANT(float, 256, 4, 2, 128, 23, false, true, false)
    TT_GLDS_VARIANT(float, 32, 8, 1, 128, 2, false, true, true)
    TT_GLDS_VARIANT(float, 64, 8, 1, 128, 2, false, true, true)
    TT_GLDS_VARIANT(float, 128, 8, 1, 128, 2, false, true, true)
    TT_GLDS_VARIANT(float, 256, 4, 2, 128, 23, false, true, true)
    return 0;
}
#undef TT_GLDS_VARIANT

// One launch of the LDS-DMA kernel (of a tail split: the main launch, or with a.m_begin set the tail).  Split-K (c.splits > 1) launches
// the tiles only; the caller runs splitk_finalize_kernel.  1, or < 0 on failure.
int launch_conv_glds(const ConvChoice& c, ConvArgs& a, int dtype, hipStream_t st) {
    const int r = dtype == TT_F32 ? launch_glds32(c, a, st) : dtype == TT_F16 ? launch_glds16<f16_t>(c, a, st) : launch_glds16<uint16_t>(c, a, st);
    TT_REQUIRE(r, "tt_conv2d_fwd: no conv_igemm_glds_kernel<%d, %d, %d, %d, %d, %d, %d, %d> for dtype %d", c.bn, c.waves_m, c.waves_n, c.bkb,
               c.stages, (int)c.gather, (int)c.x3, (int)c.apair, dtype);
    return r;
}

}  // namespace tt

// Row-batched MLP chains of the look-and-predict decoder in ONE launch (tt_mlp_chain).
//
// The reference decoder (thinktwice_decoder.py:26-260, multi_scale_deformable_attn_function.py:197-344) is a long
// sequence of nn.Linear layers over a few hundred to a few thousand rows: query_linear -> sampling_offsets /
// attention_weights, ffn.w_1 -> w_2 (+ residual), output_proj, mlp -> traj / ctrl offset heads, the coarse heads.
// Launched one kernel per layer they are ~5 us each of pure latency.  Here a workgroup owns 32 rows and walks the
// whole chain: intermediates never leave LDS, only the outputs a later kernel needs are written to HBM.
//
// Arithmetic: "bf16x3" on the bf16 MFMA (the exact-f32 MFMA is 16x slower): every f32 operand is a bf16 (hi, lo) pair,
// a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi accumulated in f32 (relative error ~1e-5 per dot product).  Weights arrive
// pre-split from the host in FRAGMENT-MAJOR order (weights.py::split_pairs_frag: per 32-column block and 16-wide K
// step one contiguous KiB of hi halves + one of lo halves, indexed by lane), so a wave's B operand is two fully
// coalesced 1 KiB loads; intermediates are split ONCE when a stage writes them to LDS ("pair format": per row, per 16
// K elements 64 B = [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15]), so a wave's A fragment is two ds_read_b128 with no
// conversion; the chain input is split when it is loaded from HBM.
//
// Layout of a stage: out[32 rows][N] = A[32][K] * W^T.  v_mfma_f32_32x32x16_bf16: lane l supplies row / column
// (l & 31) and the 8-element K chunk (l >> 5) of a 16-element K step.  The 8 waves of the workgroup take the 32-column
// blocks of N round-robin, up to 4 accumulator blocks per wave at a time, so one A fragment feeds up to 12 MFMAs.
// Weights stream from L2 straight into the B operand registers (each element is used once per workgroup: staging
// them through LDS would only add a round trip), double-buffered one K step ahead.
//
// Which of the two forms below a chain runs in, its grid and where its intermediates go: chain_choose.cpp.
#include <mutex>

#include "bounded_wait.h"
#include "chain_choose.h"
#include "conv_common.h"

namespace tt {

constexpr int kChainPF = 4;       // weight K-steps in flight per wave

struct ChainArgs {
    const float* x;
    long long R;
    int x_stride, nstages;
    int nbw;              // 32-column blocks per wave per pass (1..kChainNBW); 1 when N is split over gridDim.y
    ChainStage st[kChainMaxStages];
};

// (The operand split, the pair-format LDS buffers and the two-accumulator product of these kernels: bf16x3.h.)

__global__ __launch_bounds__(kChainWaves * 64) void mlp_chain_kernel(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r_ = lane & 31, h_ = lane >> 5;
    const long long m0 = (long long)blockIdx.x * 32;
    const long long m = m0 + r_;
    const bool row_ok = m < a.R;

    for (int s = 0; s < a.nstages; ++s) {
        const ChainStage& S = a.st[s];
        const int NB = (S.N + 31) >> 5;
        const int nsteps = S.Kp >> 4;
        const bool from_x = S.in_sel < 0;
        const unsigned char* abuf = from_x ? nullptr : smem + a.st[S.in_sel].lds_off;
        const int astride = from_x ? 0 : a.st[S.in_sel].lds_stride;
        const float* xrow = a.x + (row_ok ? m : 0) * a.x_stride;

        const int per_pass = kChainWaves * a.nbw;
        for (int base = per_pass * blockIdx.y; base < NB; base += per_pass * gridDim.y) {
            // launder the lane-derived indices: the row / column address arithmetic of the epilogue is invariant across
            // passes and stages and would otherwise be hoisted and kept live through the K loops (spills)
            int r = r_, h = h_;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(r), "+v"(h));
#endif
            // this pass: blocks nb0, nb0 + 8, ... (nbw of them, those < NB); gridDim.y > 1 splits a single wide stage
            const int nb0 = base + wave;
            const unsigned char* bptr[kChainNBW];
            bool live[kChainNBW];
#pragma unroll
            for (int q = 0; q < kChainNBW; ++q) {
                const int nb = nb0 + q * kChainWaves;
                live[q] = q < a.nbw && nb < NB;
                // fragment-major weights: block nb, step ks at ((nb * nsteps + ks) * 2 + plane) KiB, lane-contiguous
                bptr[q] = reinterpret_cast<const unsigned char*>(S.w) + (size_t)(live[q] ? nb : 0) * nsteps * 2048 +
                          (h * 32 + r) * 16;
            }
            f32x16 acc[kChainNBW], acc2[kChainNBW];
#pragma unroll
            for (int q = 0; q < kChainNBW; ++q)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[q][i] = acc2[q][i] = 0.f;

            // Weight ring of kChainPF K-steps; every load is UNCONDITIONAL (step clamped to the last one, dead blocks
            // re-read block 0, rows beyond R re-read row 0) so the compiler counts the outstanding loads statically
            // instead of draining them at every loop head.
            const int last = nsteps - 1;
            auto load_b = [&](int ks, uint4 (&bh)[kChainNBW], uint4 (&bl)[kChainNBW]) {
                const int kk = ks < last ? ks : last;
#pragma unroll
                for (int q = 0; q < kChainNBW; ++q) {
                    const unsigned char* p = bptr[q] + (size_t)kk * 2048;
                    bh[q] = *reinterpret_cast<const uint4*>(p);
                    bl[q] = *reinterpret_cast<const uint4*>(p + 1024);
                }
            };
            uint4 bh[kChainPF][kChainNBW], bl[kChainPF][kChainNBW];
#pragma unroll
            for (int p = 0; p < kChainPF; ++p) load_b(p, bh[p], bl[p]);
            if (from_x) {
                // A from HBM/L2 (f32 rows, x_stride >= Kp checked by the host): a ring of raw fragments, split on use
                const float* xa = xrow + h * 8;
                float4 ar0[kChainPF], ar1[kChainPF];
#pragma unroll
                for (int p = 0; p < kChainPF; ++p) {
                    const int kk = p < last ? p : last;
                    ar0[p] = *reinterpret_cast<const float4*>(xa + kk * 16);
                    ar1[p] = *reinterpret_cast<const float4*>(xa + kk * 16 + 4);
                }
#pragma unroll 1
                for (int ks = 0; ks < nsteps; ks += kChainPF) {
#pragma unroll
                    for (int p = 0; p < kChainPF; ++p) {
                        const int k = ks + p;
                        const float v[8] = {ar0[p].x, ar0[p].y, ar0[p].z, ar0[p].w, ar1[p].x, ar1[p].y, ar1[p].z, ar1[p].w};
                        uint4 ah, al;
                        split8(v, ah, al);
                        if (k < nsteps) {
#pragma unroll
                            for (int q = 0; q < kChainNBW; ++q)
                                if (live[q]) mfma3(ah, al, bh[p][q], bl[p][q], acc[q], acc2[q]);
                        }
                        const int kn = k + kChainPF < last ? k + kChainPF : last;
                        ar0[p] = *reinterpret_cast<const float4*>(xa + kn * 16);
                        ar1[p] = *reinterpret_cast<const float4*>(xa + kn * 16 + 4);
                        load_b(k + kChainPF, bh[p], bl[p]);
                    }
                }
            } else {
                const unsigned char* pa = abuf + (size_t)r * astride + h * 16;
#pragma unroll 1
                for (int ks = 0; ks < nsteps; ks += kChainPF) {
#pragma unroll
                    for (int p = 0; p < kChainPF; ++p) {
                        const int k = ks + p;
                        const int kk = k < last ? k : last;
                        const uint4 ah = *reinterpret_cast<const uint4*>(pa + kk * 64);
                        const uint4 al = *reinterpret_cast<const uint4*>(pa + kk * 64 + 32);
                        if (k < nsteps) {
#pragma unroll
                            for (int q = 0; q < kChainNBW; ++q)
                                if (live[q]) mfma3(ah, al, bh[p][q], bl[p][q], acc[q], acc2[q]);
                        }
                        load_b(k + kChainPF, bh[p], bl[p]);
                    }
                }
            }

            // epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
#pragma unroll
            for (int q = 0; q < kChainNBW; ++q) {
                if (!live[q]) continue;
                const int n = (nb0 + q * kChainWaves) * 32 + r;
                const bool n_ok = n < S.N;
                // the kept row is N rounded up to 16 columns wide (the consumer's Kp), the block to 32: with N % 32 in 1 .. 16 the
                // block's last 16 columns lie behind the row -- in the next row's first group (and, for row 31, behind the buffer)
                const bool n_kept = S.lds_off >= 0 && n < ((S.N + 15) & ~15);
                const float bias = (S.bias && n_ok) ? S.bias[n] : 0.f;
                float sw[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) sw[j] = (S.side && n_ok && j < S.side_k) ? S.side_w[n * S.side_k + j] : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
                    const long long mr = m0 + rr;
                    const bool ok = n_ok && mr < a.R;
                    float v = (acc[q][i] + acc2[q][i]) + bias;
                    if (S.side && ok) {
                        const float* sp = S.side + mr * S.side_stride;
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (j < S.side_k) v += sp[j] * sw[j];
                    }
                    if (S.res && ok) v += S.res[mr * S.res_stride + S.res_coff + n];
                    v = apply_act(v, S.act);
                    if (!ok) v = 0.f;
                    if (S.out && ok) S.out[mr * S.out_stride + S.out_coff + n] = v;
                    if (n_kept) pair_store(smem + S.lds_off + (size_t)rr * S.lds_stride, n, v);
                }
            }
        }
        __syncthreads();   // this stage's LDS output is complete (and its input buffer free) before the next stage
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The WIDE form (tt_mlp_chain_wide): few rows, so the time of a chain is the latency of streaming its weights -- one workgroup
// keeps ~128 KiB of loads in flight and gets ~45 GB/s out of the L2 (a 4.4 MB chain: 90-120 us; the batch-1 tick runs 38 of
// them back to back).  Here the COLUMNS of every stage are dealt over `G` co-resident workgroups per 32 rows (gridDim.y) and
// the eight waves of a workgroup split the K steps of a column block between them (partial tiles summed through LDS in wave
// order: deterministic).  Stage outputs a later stage reads go through an f32 scratch in global memory; between dependent
// stages the G workgroups of a row block meet at a ticket barrier (agent-scope release / acquire: the XCDs' L2s are not
// coherent with each other for ordinary stores).  The ticket counters live in a library-owned pool, are claimed round-robin per
// launch and reset themselves with the launch's last arrival.
constexpr int kWidePF = 8;               // K steps in flight per wave (8 x 4 KiB: weights + activation fragments)

struct WideStage {
    ChainStage s;
    const float* in;      // stage input: the chain input rows, or an earlier stage's scratch (fragment-major)
    int in_stride;        // row stride in floats; fragment-major: 16-column steps per row block
    int in_frag;
    float* keep;          // scratch of this stage's output (null: no later stage reads it), fragment-major
    int keep_stride;      // its steps per row block = N rounded up to 32, / 16
    int sync_before;      // the row block's workgroups meet before this stage
};

struct WideArgs {
    long long R;
    int nstages, nsync;
    int rb;               // 32-row blocks per workgroup (1, 2, 4 or 8); its eight waves = rb row blocks x 8 / rb K slices
    unsigned* tickets;    // one counter (64 B apart) per row group
    int* fault;           // HOST-mapped (pinned) word of this device, set with a system-scope store if a ticket wait gave up:
                          // the host reads it without a copy (tt_device_faults) and every later entry point refuses to run
    int max_spin;         // polls before a wait gives up (pair_wait_max_spin; tests force a time-out with 0)
    long long* trace;     // debug (tt_mlp_chain_wide_set_trace): 64 wall-clock stamps (10 ns ticks) per workgroup, or null
    WideStage st[kChainMaxStages];
};

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every outstanding global store (~1 us per
// stage here), which only the ticket barrier needs
__device__ __forceinline__ void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// Arrive + wait (bounded_wait.h).  Returns true if the wait GAVE UP: the caller poisons every value the workgroup writes from here
// on.  The workgroup still arrives at every later barrier, so the counter reaches its total and resets itself for the slot's next
// launch.
__device__ __forceinline__ bool ticket_barrier(unsigned* ctr, unsigned target, int* fault, int max_spin, int* gave_up) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        bounded_wait(ctr, target, fault, max_spin, gave_up);
    }
    __syncthreads();
    return *gave_up != 0;
}

// One stage of the wide chain with a ring of PF K steps per wave (PF = 2, 4, 8 by the stage's steps per wave: every ring slot
// is loaded unconditionally, and a workgroup's loads go through one L1 at 64 B / clock -- a ring deeper than the stage has
// steps would spend more time on duplicate loads than the stage's own weights take).
template <int PF>
__device__ __forceinline__ void wide_stage(const WideArgs& a, const WideStage& W, float (*part)[32][32], unsigned* ctr,
                                           unsigned& arrived, long long* tr, int& tri, int* gave_up, bool& poisoned) {
    const ChainStage& S = W.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = gridDim.y, g = blockIdx.y;
    const int RB = a.rb, KS = kChainWaves / RB;
    const int rb = wave & (RB - 1), ks = wave / RB;
    const long long m0g = (long long)blockIdx.x * RB * 32;       // first row of the workgroup
    const long long m0 = m0g + rb * 32;                          // first row of this wave's block
    auto stamp = [&]() {
        if (tr && tid == 0 && tri < 64) tr[tri++] = (long long)wall_clock64();
    };
    const int NB = (S.N + 31) >> 5;
    const int nsteps = S.Kp >> 4;
    const int last = nsteps - 1;
    const int mine = (nsteps - ks + KS - 1) / KS;                // K steps ks, ks + KS, ... (<= 0: none)
    int r = lane & 31, h = lane >> 5;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(r), "+v"(h));
#endif
    // The WEIGHT half of the first block's ring is issued before the barrier: it does not depend on the other workgroups.
    uint4 bh[PF], bl[PF];
    float4 a0[PF], a1[PF];
    const unsigned char* bp = reinterpret_cast<const unsigned char*>(S.w) + (size_t)(g < NB ? g : 0) * nsteps * 2048 +
                              (h * 32 + r) * 16;
    auto load_b = [&](int step, int p) {
        const int kk = step < last ? step : last;
        const unsigned char* q = bp + (size_t)kk * 2048;
        bh[p] = *reinterpret_cast<const uint4*>(q);
        bl[p] = *reinterpret_cast<const uint4*>(q + 1024);
    };
#pragma unroll
    for (int p = 0; p < PF; ++p) load_b(ks + KS * p, p);
    if (W.sync_before) {
        arrived += (unsigned)G;
        poisoned = ticket_barrier(ctr, arrived, a.fault, a.max_spin, gave_up) || poisoned;
    }
    stamp();
    // activation fragments: lanes of rows beyond R load nothing (a 1-row chain issues 2 of 64 lanes).  Row-major input (the
    // chain input): 32 B of row m0 + r per step; an earlier stage's scratch is FRAGMENT-MAJOR (per row block and step two
    // contiguous KiB indexed by lane), so those loads are fully coalesced.
    const bool row_live = m0 + r < a.R;
    const float* ap;
    int a_step, a_off1;
    if (W.in_frag) {
        ap = W.in + ((size_t)(m0 >> 5) * W.in_stride * 128 + (size_t)(h * 32 + r)) * 4;
        a_step = 512; a_off1 = 256;
    } else {
        ap = W.in + (row_live ? m0 + r : 0) * W.in_stride + h * 8;
        a_step = 16; a_off1 = 4;
    }
    auto load_a = [&](int step, int p) {
        const int kk = step < last ? step : last;
        if (row_live) {
            a0[p] = *reinterpret_cast<const float4*>(ap + (size_t)kk * a_step);
            a1[p] = *reinterpret_cast<const float4*>(ap + (size_t)kk * a_step + a_off1);
        } else {
            a0[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            a1[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    for (int nb = g; nb < NB; nb += G) {
        if (nb != g) {
            bp += (size_t)G * nsteps * 2048;
#pragma unroll
            for (int p = 0; p < PF; ++p) load_b(ks + KS * p, p);
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) load_a(ks + KS * p, p);
        // epilogue operands, loaded now so that their latency is not exposed after the K loop (first two row slots of the
        // thread: all of them when the workgroup has one row block)
        const int col = tid & 31, n = nb * 32 + col;
        const bool n_ok = n < S.N;
        const float bias = (S.bias && n_ok) ? S.bias[n] : 0.f;
        // (straight-line code: clamped addresses + selects under wave-uniform branches, not one branch per element)
        float sw[8], pre[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) sw[j] = 0.f;
        const int n_c = n_ok ? n : 0;
        if (S.side) {
            float wv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[j] = S.side_w[n_c * S.side_k + (j < S.side_k ? j : 0)];
#if defined(__HIP_DEVICE_COMPILE__)
            // all eight loads issued before the first select (the compiler otherwise sinks each into its own branch: 8 serial
            // round trips)
            asm volatile("" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]), "+v"(wv[3]), "+v"(wv[4]), "+v"(wv[5]), "+v"(wv[6]), "+v"(wv[7]));
#endif
#pragma unroll
            for (int j = 0; j < 8; ++j) sw[j] = (n_ok && j < S.side_k) ? wv[j] : 0.f;
        }
        constexpr int kPre = PF < 8 ? 2 : 0;                       // (the deep ring has no registers to spare, and its stages
                                                                  // are bound by their weight stream, not by this latency)
#pragma unroll
        for (int j = 0; j < kPre; ++j) {
            const long long mr = m0g + (tid >> 5) + 16 * j;
            const long long mr_c = mr < a.R ? mr : 0;
            float v = 0.f;
            if (S.res) v = S.res[mr_c * S.res_stride + S.res_coff + n_c];
            if (S.side) {
                const float* sp = S.side + mr_c * S.side_stride;
                float sv[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) sv[jj] = sp[jj < S.side_k ? jj : 0];
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]), "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7]));
#endif
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) v += sv[jj] * sw[jj];
            }
            pre[j] = v;                                           // used only where (mr < R && n < N)
        }

        f32x16 acc, acc2;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = acc2[i] = 0.f;
#pragma unroll 1
        for (int i = 0; i < mine; i += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const float v[8] = {a0[p].x, a0[p].y, a0[p].z, a0[p].w, a1[p].x, a1[p].y, a1[p].z, a1[p].w};
                uint4 ah, al;
                split8(v, ah, al);
                if (i + p < mine) mfma3(ah, al, bh[p], bl[p], acc, acc2);
                if (i + PF < mine) {                 // wave-uniform: the last ring round reloads nothing
                    const int nxt = ks + KS * (i + p + PF);
                    load_b(nxt, p);
                    load_a(nxt, p);
                }
            }
        }
        // this wave's partial tile.  C/D map: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int i = 0; i < 16; ++i) part[wave][(i & 3) + 8 * (i >> 2) + 4 * h][r] = acc[i] + acc2[i];
        lds_barrier();
        if (nb == g) stamp();
        // epilogue: thread -> column `col` of rows (tid >> 5) + 16 j of the workgroup's RB * 32 rows; the K slices of a row
        // block are summed in slice order
        for (int j = 0; j < 2 * RB; ++j) {
            const int rg = (tid >> 5) + 16 * j;                   // row within the workgroup
            const int b = rg >> 5, rr = rg & 31;
            const long long mr = m0g + rg;
            const bool ok = n_ok && mr < a.R;
            float v = part[b][rr][col];
            for (int q = 1; q < KS; ++q) v += part[q * RB + b][rr][col];
            v += bias;
            if (j < kPre) {
                v += j == 0 ? pre[0] : pre[1];
            } else {
                const long long mr_c = ok ? mr : 0;
                float t = 0.f;
                if (S.res) t = S.res[mr_c * S.res_stride + S.res_coff + n_c];
                if (S.side) {
                    const float* sp = S.side + mr_c * S.side_stride;
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) t += sp[jj < S.side_k ? jj : 0] * sw[jj];
                }
                v += t;
            }
            v = apply_act(v, S.act);
            if (poisoned) v = __builtin_nanf("");                 // a barrier of this workgroup timed out: never a plausible number
            if (!ok) v = 0.f;
            if (S.out && ok) S.out[mr * S.out_stride + S.out_coff + n] = v;
            if (W.keep && mr < a.R)                              // fragment-major scratch (see load_a); padding columns = 0
                W.keep[((((size_t)(mr >> 5) * W.keep_stride + (n >> 4)) * 2 + ((n >> 2) & 1)) * 64 + ((n >> 3) & 1) * 32 + rr) * 4 +
                       (n & 3)] = v;
        }
        lds_barrier();      // `part` is free again; the global stores are NOT waited for here (the next ticket barrier does)
    }
    stamp();
}

__global__ __launch_bounds__(kChainWaves * 64) void mlp_chain_wide_kernel(const WideArgs a) {
    __shared__ float part[kChainWaves][32][32];
    __shared__ int gave_up;
    const int tid = threadIdx.x;
    const int G = gridDim.y, g = blockIdx.y;
    unsigned* ctr = a.tickets + (size_t)blockIdx.x * 16;
    unsigned arrived = 0;
    bool poisoned = false;
    if (tid == 0) gave_up = 0;                                   // (published by the first ticket barrier's __syncthreads)
    long long* tr = a.trace ? a.trace + ((size_t)blockIdx.x * G + g) * 64 : nullptr;
    int tri = 0;
    if (tr && tid == 0) tr[tri++] = (long long)wall_clock64();
    const int KS = kChainWaves / a.rb;
    for (int s = 0; s < a.nstages; ++s) {
        const WideStage& W = a.st[s];
        if (tr && tid == 0 && tri < 64) tr[tri++] = (long long)wall_clock64();
        const int per_wave = ((W.s.Kp >> 4) + KS - 1) / KS;      // K steps of the busiest wave (uniform over the workgroup)
        if (per_wave <= 2) wide_stage<2>(a, W, part, ctr, arrived, tr, tri, &gave_up, poisoned);
        else if (per_wave <= 4) wide_stage<4>(a, W, part, ctr, arrived, tr, tri, &gave_up, poisoned);
        else wide_stage<8>(a, W, part, ctr, arrived, tr, tri, &gave_up, poisoned);
    }
    // the launch's last arrival puts the ticket back to zero for the next launch that claims this slot
    __syncthreads();
    if (tid == 0) {
        const unsigned total = (unsigned)(a.nsync + 1) * (unsigned)G;
        const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1 == total) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_mlp_chain(const float* x, long long R, int x_stride, int nstages, const tt_chain_stage* st,
                            int n_split, void* stream) {
    if (int rc = chain_validate("tt_mlp_chain", x, R, x_stride, nstages, st)) return rc;
    ChainChoice c;
    if (int rc = chain_choose(R, nstages, st, n_split, 0, CHAIN_ROWS, -1, &c)) return rc;
    ChainArgs a;
    a.x = x; a.R = R; a.x_stride = x_stride; a.nstages = nstages;
    a.nbw = c.nbw;
    for (int s = 0; s < nstages; ++s) {
        a.st[s] = chain_stage(st[s]);
        a.st[s].lds_off = c.lds_off[s];
        a.st[s].lds_stride = c.lds_stride[s];
    }
    if (lds_opt_in(reinterpret_cast<const void*>(mlp_chain_kernel), 160 * 1024, "mlp_chain_kernel")) return -1;
    hipLaunchKernelGGL(mlp_chain_kernel, dim3((unsigned)c.row_groups, (unsigned)c.n_split), dim3(kChainWaves * 64), c.lds_total,
                       (hipStream_t)stream, a);
    return check_launch("tt_mlp_chain");
}

// ---- tt_mlp_chain_wide
// Host state of the wide form, PER DEVICE and behind one mutex (the library may be driven from several host threads / devices):
//  * the ticket pool: kEagerSlots counters claimed round-robin by plain launches (a collision needs > kEagerSlots row groups in
//    flight at once), and kCapturedSlots claimed PERMANENTLY by launches recorded into a HIP graph (a captured launch replays
//    with the slot baked into its arguments, so no later launch may be handed the same counter);
//  * the co-residency capacity: hipOccupancyMaxActiveBlocksPerMultiprocessor x the device's CU count.  A launch may use at most
//    capacity / kWideConcurrent workgroups (the decoder runs two chains at a time, on its main and its branch stream), so the
//    spinning workgroups of concurrent launches can never fill the chip and keep their own peers out.  hipLaunchCooperativeKernel
//    would give the same guarantee per launch, but it goes through the device's single cooperative queue (the two streams'
//    chains would serialise) and is not recordable into a HIP graph; the occupancy bound + bounded spin + loud fault is the
//    form that keeps both.
// (The fault word a barrier that gives up sets, and the bound on its wait: common.cpp.)
namespace {
constexpr int kEagerSlots = 4096;        // 64 B each; a launch claims one per row group
constexpr int kCapturedSlots = 12288;
constexpr int kWideConcurrent = 2;
struct WidePool {
    unsigned* tickets = nullptr;         // kEagerSlots + kCapturedSlots counters, 64 B apart, device memory
    unsigned next_eager = 0, next_captured = 0;
    int capacity = 0;                    // co-resident workgroups of mlp_chain_wide_kernel on this device
};
WidePool g_pools[kMaxDevices];
std::mutex g_wide_mutex;
long long* g_trace = nullptr;            // tt_mlp_chain_wide_set_trace

// (g_wide_mutex held)
WidePool* wide_pool(int dev) {
    WidePool& P = g_pools[dev];
    if (P.tickets) return &P;
    if (!tt::device_fault_word()) {
        tt::set_error("tt_mlp_chain_wide: cannot allocate the host-mapped fault word");
        return nullptr;
    }
    int occ = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tt::mlp_chain_wide_kernel, kChainWaves * 64, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || occ < 1 || cus < 1) {
        (void)hipGetLastError();
        tt::set_error("tt_mlp_chain_wide: cannot query the kernel's occupancy on device %d", dev);
        return nullptr;
    }
    void* p = nullptr;
    const size_t bytes = (size_t)(kEagerSlots + kCapturedSlots) * 64;
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) {
        (void)hipGetLastError();
        tt::set_error("tt_mlp_chain_wide: cannot allocate the ticket pool");
        return nullptr;
    }
    P.capacity = occ * cus;
    P.tickets = static_cast<unsigned*>(p);
    return &P;
}
}  // namespace

// Workgroups one launch may use on the current device (co-resident capacity / kWideConcurrent), or < 0 on error.
extern "C" int tt_mlp_chain_wide_max_workgroups(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -2;
    std::lock_guard<std::mutex> lock(g_wide_mutex);
    WidePool* P = wide_pool(dev);
    return P ? P->capacity / kWideConcurrent : -2;
}

extern "C" int tt_mlp_chain_wide_set_trace(void* stamps_or_null) {
    g_trace = static_cast<long long*>(stamps_or_null);
    return 0;
}

extern "C" int tt_mlp_chain_wide(const float* x, long long R, int x_stride, int nstages, const tt_chain_stage* st,
                                 int n_groups, void* workspace, long long workspace_bytes, void* stream) {
    // host-side argument checks first (no device is touched until they pass)
    if (int rc = chain_validate("tt_mlp_chain_wide", x, R, x_stride, nstages, st)) return rc;
    ChainChoice c;
    if (int rc = chain_choose(R, nstages, st, 1, n_groups, CHAIN_WIDE_AS_GIVEN, -1, &c)) return rc;
    TT_REQUIRE(workspace && workspace_bytes >= c.workspace_bytes && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "tt_mlp_chain_wide: workspace of %lld B needed (%lld given)", c.workspace_bytes, workspace_bytes);
    if (int rc = tt::refuse_after_fault("tt_mlp_chain_wide")) return rc;
    int dev = 0;
    TT_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices, "tt_mlp_chain_wide: no current device");
    std::lock_guard<std::mutex> lock(g_wide_mutex);     // pool creation + slot claim (+ the launch: slots stay in claim order)
    WidePool* P = wide_pool(dev);
    if (!P) return -2;
    if (int rc = chain_wide_fits(c, P->capacity / kWideConcurrent)) return rc;
    WideArgs a;
    a.R = R; a.nstages = nstages; a.nsync = c.nsync; a.rb = c.rb;
    for (int s = 0; s < nstages; ++s) {
        WideStage& W = a.st[s];
        W.s = chain_stage(st[s]);
        W.keep = c.keep_off[s] < 0 ? nullptr : reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + c.keep_off[s]);
        W.keep_stride = c.keep_stride[s];
        W.sync_before = c.sync_before[s];
        const int in = st[s].in_sel;
        if (in < 0) {
            W.in = x; W.in_stride = x_stride; W.in_frag = 0;
        } else {
            W.in = a.st[in].keep; W.in_stride = a.st[in].keep_stride; W.in_frag = 1;
        }
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusNone;
    }
    const unsigned row_groups = (unsigned)c.row_groups;
    if (cap == hipStreamCaptureStatusActive) {          // replayed with these arguments: the slots are this launch's for good
        if (P->next_captured + row_groups > (unsigned)kCapturedSlots) {
            // a process that keeps re-capturing graphs: captured launches own their slots for good.  Distinct code: the caller
            // records the one-workgroup-per-row-block chain (tt_mlp_chain) instead (ops.mlp_chain does)
            tt::set_error("tt_mlp_chain_wide: the %d ticket slots reserved for graph-captured launches are used up", kCapturedSlots);
            return -4;
        }
        a.tickets = P->tickets + (size_t)(kEagerSlots + P->next_captured) * 16;
        P->next_captured += row_groups;
    } else {
        if (P->next_eager + row_groups > (unsigned)kEagerSlots) P->next_eager = 0;
        a.tickets = P->tickets + (size_t)P->next_eager * 16;
        P->next_eager += row_groups;
    }
    a.fault = tt::device_fault_word();
    a.max_spin = tt::pair_wait_max_spin();
    a.trace = g_trace;
    hipLaunchKernelGGL(mlp_chain_wide_kernel, dim3(row_groups, (unsigned)c.n_groups), dim3(kChainWaves * 64), 0,
                       (hipStream_t)stream, a);
    return check_launch("tt_mlp_chain_wide");
}

// One K step of the hand-pipelined bf16x3 kernels: the TN groups of MG MFMAs and everything that runs in the gaps behind them.
// This is TEXT, included by conv_x3_pipe.hip inside the K step loop of each of its two kernels (TT_X3_RUN3 = 0: per-tap activation
// tiles, conv_x3_pipe_kernel; 1: run-staged activations, conv_x3_run3_kernel), so that the schedule -- MFMA term order, the bh / bl
// refill, the barrier slot, the read and wait slots, the split-slot layouts, the weight walker's gaps and the weight-stage swap -- is
// stated once.  It is not a function: either kernel's instruction stream moves when its body is reached through a call, even a
// force-inlined one (profiles/x3_pipe_one_body.txt), and what a form does differently is chosen by the preprocessor, so that each
// kernel sees exactly its own statements.
//
// The including K step has defined: kc (this K step's index in its tile), kn (the next one's), srcA / srcB (the stages the next K
// step's operands lie in), dma(q) (issue piece q of this K step's DMA stream), the fragment registers ah / al / bh / bl / ra0 / ra1,
// the accumulators, fb_pre, the walkers and the stage addresses; TT_X3_RUN3 = 1 also t (the tile's kw), nkw / ntap (kw and tap of
// the K step being prepared), a_count (the run pieces this tile issues), f_mask, fa_run and zaddr; TT_X3_RUN3 = 0 fa_pre.
uint32_t sh[4], sl[4];
float st0 = 0.f, st1 = 0.f;
// split stage s = 2 * pair + half of the fragment in ra0 / ra1
auto split_stage = [&](int s) {
    // pinned on both sides: the stage's 3 VALU cannot start before this point (input pin) nor end after it
    const int e = s >> 1;
    asm volatile("" : "+v"(ra0), "+v"(ra1));
    const float x0 = __uint_as_float(e == 0 ? ra0.x : e == 1 ? ra0.z : e == 2 ? ra1.x : ra1.z);
    const float x1 = __uint_as_float(e == 0 ? ra0.y : e == 1 ? ra0.w : e == 2 ? ra1.y : ra1.w);
    if (TT_PIPE_DEBUG & 2) {
        if ((s & 1) == 0) sh[e] = __float_as_uint(x0);
        else sl[e] = __float_as_uint(x1);
        return;
    }
    if ((s & 1) == 0) {
        split_hi(x0, x1, sh[e], st0, st1);
        asm volatile("" : "+v"(sh[e]), "+v"(st0), "+v"(st1));
    } else {
        asm volatile("" : "+v"(st0), "+v"(st1));
        sl[e] = split_lo(x0, x1, st0, st1);
        asm volatile("" : "+v"(sl[e]));
    }
};
#pragma unroll
for (int g = 0; g < TN; ++g) {
    const int rb = g / NGR;                             // row block whose next fragment this group works on
    const bool barw = (kc == 1 && rb == 0);             // window that carries the tile barrier
    const bool bar = barw && (g % NGR) == 0;            // ... and the group inside it
    const bool last = g == TN - 1;
    // window slots: reads @1, wait @4, eight split stages from @4 on; barrier window: barrier @3, reads @4, wait @7
    constexpr int R0 = 1, W0 = 4, RB = 4, WB = 7;
#pragma unroll
    for (int m = 0; m < MG; ++m) {
        const int term = m / TM, i = m % TM;
        if (term == 0) TT_MFMA(acc[i][g], al[kc][i], bh[g]);
        else if (term == 1) TT_MFMA(acc[i][g], ah[kc][i], bl[g]);
        else TT_MFMA(acc[i][g], ah[kc][i], bh[g]);
        // ---- the gap behind MFMA m
        const int ws = (g % NGR) * MG + m;              // slot inside the row-block window
        if (m == 0 && !(TT_PIPE_DEBUG & 8)) {
            // hi half of the column block the previous group finished with.  g = 0: column TN-1 of THIS K step
            // (its registers were busy until the previous K step's last MFMA); else column g-1 of the next one
            if (g == 0) bh[TN - 1] = lds_read(sB_cur + fb_pre[kc][TN - 1]);
            else bh[g - 1] = lds_read(srcB + fb_pre[kn][g - 1]);
        }
        if (bar && m == 3) {
            // The next tile's operands have landed for this wave; only the activation pieces issued with THIS tile stay in flight
            // (s_waitcnt takes an immediate).  Every fragment read of this tile is complete: publish the next tile, free this
            // one's stages.
#if TT_X3_RUN3
            // its weights, and -- third tile of a run -- the next run (issued with the first two tiles: 5 + 4 pieces)
            if (TT_PIPE_DEBUG & 16) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else if (t == 0) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else if (t == 1) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
            // the NIA = 8 youngest loads are the activations of the tile two ahead
            if (TT_PIPE_DEBUG & 16) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
        }
        if (ws == (barw ? RB : R0) && !(TT_PIPE_DEBUG & 8)) {
            // the next K step's activation fragment of row block rb (pair format: straight into ah / al, whose last readers,
            // the previous K step's MFMAs, were issued long ago)
#if TT_X3_RUN3
            // padding: a lane whose (row, tap) is outside the image reads the zero row
            const unsigned a0 = ((f_mask[rb] >> ntap) & 1u) ? srcA + fa_run[nkw][kn][rb] : zaddr;
            if constexpr (APAIR) {
                ah[kn][rb] = lds_read(a0);
                al[kn][rb] = lds_read(a0 ^ 32u);
            } else {
                ra0 = lds_read(a0);
                ra1 = lds_read(a0 ^ 16u);
            }
#else
            if constexpr (APAIR) {
                ah[kn][rb] = lds_read(srcA + fa_pre[kn][rb]);
                al[kn][rb] = lds_read(srcA + (fa_pre[kn][rb] ^ 32u));
            } else {
                ra0 = lds_read(srcA + fa_pre[kn][rb]);
                ra1 = lds_read(srcA + (fa_pre[kn][rb] ^ 16u));
            }
#endif
        }
        // DMA: gaps 2 and 3 of a group, behind the fragment reads; in the barrier group gaps 4 and 5, behind the barrier (the
        // weight stage it frees)
        {
            const int s0 = bar ? 4 : 2;
#if TT_X3_RUN3
            // weights: one piece per group; run pieces: spread from group 0 on, two per group only where the count needs it
            // (TN = 4, five pieces)
            if (kc == 1) {
                if (m == s0) dma(g);
            } else if (a_count > 0) {
                const int per = (a_count + TN - 1) / TN;
                const int q0 = g * per;
                if (m == s0 && q0 < a_count) dma(q0);
                if (per == 2 && m == s0 + 1 && q0 + 1 < a_count) dma(q0 + 1);
            }
#else
            constexpr int DPG = 2;                      // slots per group (a weight step uses one)
            const int npieces = kc == 0 ? DPA : DPB;
            if (m == s0) dma(npieces * g);
            if (m == s0 + 1 && npieces == DPG) dma(npieces * g + 1);
#endif
        }
        if (ws == (barw ? WB : W0)) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (APAIR) asm volatile("" : "+v"(ah[kn][rb]), "+v"(al[kn][rb]));
            else asm volatile("" : "+v"(ra0), "+v"(ra1));
            if (g == 0) asm volatile("" : "+v"(bh[TN - 1]));     // the gap-0 read of this K step has landed too
        }
        if (m == 2 * TM - 1 && !(TT_PIPE_DEBUG & 8)) bl[g] = lds_read(srcB + (fb_pre[kn][g] ^ 32u));   // lo half: free now
        if constexpr (!APAIR) {
            // the eight 3-VALU split stages, spread over what is left of the window
            const int first = barw ? WB : W0;
            const int avail = WIN - first;
            int lastslot;
            if (avail >= 16) {                           // every other gap
                if (ws >= first && ((ws - first) & 1) == 0 && (ws - first) / 2 < 8) split_stage((ws - first) / 2);
                lastslot = first + 14;
            } else if (avail >= 8) {                     // every gap
                if (ws >= first && ws - first < 8) split_stage(ws - first);
                lastslot = first + 7;
            } else {                                     // two stages per gap
                if (ws >= first && ws - first < 4) {
                    split_stage(2 * (ws - first));
                    split_stage(2 * (ws - first) + 1);
                }
                lastslot = first + 3;
            }
            if (ws == lastslot) {
                ah[kn][rb] = u32x4{sh[0], sh[1], sh[2], sh[3]};
                al[kn][rb] = u32x4{sl[0], sl[1], sl[2], sl[3]};
                asm volatile("" : "+v"(ah[kn][rb]), "+v"(al[kn][rb]));
            }
        }
        // the walker of the DMA stream this K step has just finished issuing, and the tile's stage rotation
#if TT_X3_RUN3
        // the run walker after the run's last piece went out (second tile): a dozen SALU once per run, not pinned
        if (last && kc == 0 && t == 1 && m == MG - 2) run_walk();
#else
        if (last && kc == 0) {
            if (m == MG - 3) {
                asm volatile("" : "+s"(a_kw));
                a_walk1();
                asm volatile("" : "+s"(a_kw), "+s"(a_d));
            }
            if (m == MG - 2) {
                asm volatile("" : "+s"(a_tap), "+s"(a_d), "+s"(a_off));
                a_walk2();
                asm volatile("" : "+s"(a_tap), "+s"(a_off));
            }
            if (m == MG - 1) {
                asm volatile("" : "+s"(a_rem), "+s"(a_st));
                a_walk3();
                asm volatile("" : "+s"(a_rem), "+s"(a_st));
            }
        }
#endif
        if (last && kc == 1) {
            if (m == MG - 3) {
                asm volatile("" : "+s"(b_tap), "+s"(b_off));
                b_walk1();
                asm volatile("" : "+s"(b_tap), "+s"(b_off));
            }
            if (m == MG - 2) {
                asm volatile("" : "+s"(b_rem), "+s"(b_st));
                b_walk2();
                asm volatile("" : "+s"(b_rem), "+s"(b_st));
            }
            if (m == MG - 1) {
                // (the run buffers swap behind the run's third tile, in the kernel)
#if TT_X3_RUN3
                asm volatile("" : "+s"(sB_cur), "+s"(sB_nxt));
#else
                asm volatile("" : "+s"(sA_cur), "+s"(sA_nxt), "+s"(sB_cur), "+s"(sB_nxt));
                sA_cur = sA_nxt;
                sA_nxt = sA_nxt == ldsA + 2u * A_BYTES ? ldsA : sA_nxt + A_BYTES;
#endif
                const unsigned tb = sB_cur;
                sB_cur = sB_nxt;
                sB_nxt = tb;
#if TT_X3_RUN3
                asm volatile("" : "+s"(sB_cur), "+s"(sB_nxt));
#else
                asm volatile("" : "+s"(sA_cur), "+s"(sA_nxt), "+s"(sB_cur), "+s"(sB_nxt));
#endif
            }
        }
    }
}

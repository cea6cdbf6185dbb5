// The dispatch of the decoder's row chains, stated once: from a chain's rows, stages and hints to the form (tt_mlp_chain, a
// workgroup per 32 rows with the intermediates in LDS, or tt_mlp_chain_wide, the columns of every stage over co-resident
// workgroups that meet at ticket barriers), the grid, and the placement of every kept stage output.  Plain host arithmetic (no HIP
// call), so tt_mlp_chain_plan answers without a device and the rules are testable on any machine (tests/test_chain_choice.py).
// The launchers in dec_chain.hip only map a choice onto their kernel's arguments; a rule that is not here does not exist.
//
// The wide form guards a kernel whose workgroups spin on each other: a grid this file lets through must be co-resident, or the
// launch ends in a barrier time-out.  The form also decides the order of the K sum, i.e. the bits of the output: no number here
// moves without a new record in tests/chain_choice_cases.json.
#include "chain_choose.h"

namespace tt {

namespace {

constexpr int kWideMaxRowBlocks = 16;       // AUTO: beyond 512 rows the rows alone fill enough workgroups
constexpr int kWideRoom = 128;              // workgroups the choice gives one launch: co-resident with room to spare (half of the
                                            // CUs of an MI355X, the other half for the chain on the decoder's other stream)
constexpr int kWideDefaultGroups = 16;      // column groups without a hint: the widest stage's blocks, at most this
constexpr int kWideMaxGroups = 64;          // column groups per row group the kernel's ticket arithmetic is checked for
constexpr size_t kLdsBudget = 160 * 1024;   // LDS of a CU: the row form's intermediates of 32 rows

long long keep_cols(int N) { return (N + 31) / 32 * 32; }

// 32-row blocks per workgroup of the wide form: with several row blocks the waves of a workgroup share the weight stream (same K
// slice, different rows) instead of every row block streaming all the weights through its own workgroup
int wide_rb(long long row_blocks) { return row_blocks <= 1 ? 1 : (row_blocks == 2 ? 2 : 4); }
long long wide_row_groups(long long row_blocks) {
    const int rb = wide_rb(row_blocks);
    return (row_blocks + rb - 1) / rb;
}

// Wide form: one fragment-major f32 scratch per stage output a later stage reads (rows padded to the workgroups' row blocks, columns
// to 32, each rounded to 256 B), and a barrier in front of every stage that reads an output not yet known complete.
void wide_layout(long long R, int nstages, const tt_chain_stage* st, ChainChoice* c) {
    const long long row_blocks = (R + 31) / 32;
    c->rb = wide_rb(row_blocks);
    c->row_groups = wide_row_groups(row_blocks);
    c->n_split = 1;
    const long long rows = c->row_groups * c->rb * 32;
    long long off = 0;
    int synced_upto = -1;                 // stages <= this index are complete on every workgroup of the row block
    for (int s = 0; s < nstages; ++s) {
        bool kept = false;
        for (int t = s + 1; t < nstages; ++t) kept = kept || st[t].in_sel == s;
        c->keep_off[s] = -1;
        if (kept) {
            c->keep_off[s] = off;
            c->keep_stride[s] = (int)keep_cols(st[s].N) / 16;
            off += (rows * keep_cols(st[s].N) * 4 + 255) / 256 * 256;
        }
        // (the consumer's padded K, a multiple of 16, lies inside the producer's 32-column blocks: finite (zero) padding)
        c->sync_before[s] = st[s].in_sel >= 0 && st[s].in_sel > synced_upto;
        if (c->sync_before[s]) { synced_upto = s - 1; ++c->nsync; }
    }
    c->workspace_bytes = off < 256 ? 256 : off;
}

// Row form: an output is kept while a LATER stage reads it; buffers are placed first-fit over the live ranges
int rows_layout(long long R, int nstages, const tt_chain_stage* st, int n_split, ChainChoice* c) {
    TT_REQUIRE(n_split >= 1 && (n_split == 1 || nstages == 1), "tt_mlp_chain: n_split > 1 needs a single stage");
    c->rb = 1;
    c->row_groups = (R + 31) / 32;
    c->n_groups = 1;
    c->n_split = n_split;
    c->nbw = n_split > 1 ? 1 : kChainNBW;         // a split stage has few blocks per workgroup: one per wave and pass
    int last_use[kChainMaxStages];
    for (int s = 0; s < nstages; ++s) last_use[s] = -1;
    for (int s = 0; s < nstages; ++s)
        if (st[s].in_sel >= 0) last_use[st[s].in_sel] = s;
    size_t off[kChainMaxStages], len[kChainMaxStages];
    size_t total = 0;
    for (int s = 0; s < nstages; ++s) {
        const tt_chain_stage& d = st[s];
        c->lds_off[s] = -1; c->lds_stride[s] = 0;
        off[s] = 0; len[s] = 0;
        if (last_use[s] >= 0) {
            const int np = (d.N + 15) / 16 * 16;          // the consumer's Kp
            c->lds_stride[s] = np * 4 + 16;
            len[s] = (size_t)32 * c->lds_stride[s];
            // Two-ended placement against the buffers still live at stage s (those read at or after s): a buffer goes
            // to the END of the 160 KiB window when its input sits in the lower half, else to the start -- a chain then
            // ping-pongs between the two ends and a long-lived buffer in the middle never splits the free space.
            auto clashes = [&](size_t pos) -> int {
                for (int t = 0; t < s; ++t)
                    if (len[t] != 0 && last_use[t] >= s && pos < off[t] + len[t] && off[t] < pos + len[s]) return t;
                return -1;
            };
            const bool in_low = d.in_sel < 0 || off[d.in_sel] + len[d.in_sel] / 2 < kLdsBudget / 2;
            bool placed = false;
            size_t pos = 0;
            for (int attempt = 0; attempt < 2 && !placed; ++attempt) {
                const bool top = (attempt == 0) ? (d.in_sel >= 0 && in_low) : !(d.in_sel >= 0 && in_low);
                if (top) {
                    if (len[s] > kLdsBudget) break;
                    long long p = (long long)((kLdsBudget - len[s]) / 16 * 16);
                    int t;
                    while (p >= 0 && (t = clashes((size_t)p)) >= 0) p = ((long long)off[t] - (long long)len[s]) / 16 * 16;
                    if (p >= 0 && clashes((size_t)p) < 0) { pos = (size_t)p; placed = true; }
                } else {
                    size_t p = 0;
                    int t;
                    while ((t = clashes(p)) >= 0) p = (off[t] + len[t] + 15) / 16 * 16;
                    if (p + len[s] <= kLdsBudget) { pos = p; placed = true; }
                }
            }
            TT_REQUIRE(placed, "tt_mlp_chain: intermediates of stage %d do not fit in 160 KiB of LDS", s);
            off[s] = pos;
            c->lds_off[s] = (int)pos;
            if (pos + len[s] > total) total = pos + len[s];
        }
    }
    for (int s = 0; s < nstages; ++s)
        if (st[s].in_sel >= 0)
            TT_REQUIRE(c->lds_stride[st[s].in_sel] == st[s].Kp * 4 + 16, "tt_mlp_chain: stage %d Kp mismatch", s);
    TT_REQUIRE(total <= kLdsBudget, "tt_mlp_chain: intermediates need %zu B of LDS (> 160 KiB)", total);
    c->lds_total = total < 16 ? 16 : total;
    return 0;
}

}  // namespace

int chain_validate(const char* who, const void* x, long long R, int x_stride, int nstages, const tt_chain_stage* st) {
    TT_REQUIRE(x && st && R > 0 && nstages >= 1 && nstages <= kChainMaxStages, "%s: bad arguments", who);
    TT_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && x_stride % 4 == 0, "%s: x must be 16 B aligned rows", who);
    for (int s = 0; s < nstages; ++s) {
        const tt_chain_stage& d = st[s];
        TT_REQUIRE(d.in_sel < s, "%s: stage %d reads stage %d", who, s, d.in_sel);
        TT_REQUIRE(d.w && d.K > 0 && d.N > 0 && d.Kp % 16 == 0 && d.Kp >= d.K && d.K % 4 == 0, "%s: stage %d: K=%d Kp=%d N=%d", who, s,
                   d.K, d.Kp, d.N);
        TT_REQUIRE((reinterpret_cast<uintptr_t>(d.w) & 15) == 0, "%s: stage %d weights unaligned", who, s);
        TT_REQUIRE(d.side_k >= 0 && d.side_k <= 8 && (!d.side || d.side_w), "%s: stage %d side input", who, s);
        TT_REQUIRE(d.in_sel >= 0 || x_stride >= d.Kp, "%s: stage %d: x rows (stride %d) must cover the padded K = %d (finite padding)",
                   who, s, x_stride, d.Kp);
        TT_REQUIRE(d.in_sel < 0 || st[d.in_sel].N == d.K, "%s: stage %d: K=%d but stage %d has N=%d", who, s, d.K, d.in_sel,
                   d.in_sel >= 0 ? st[d.in_sel].N : 0);
    }
    return 0;
}

ChainStage chain_stage(const tt_chain_stage& d) {
    ChainStage S;
    S.w = d.w; S.bias = d.bias; S.res = d.res; S.side = d.side; S.side_w = d.side_w; S.out = d.out;
    S.K = d.K; S.Kp = d.Kp; S.N = d.N; S.act = d.act; S.in_sel = d.in_sel;
    S.res_stride = d.res_stride; S.res_coff = d.res_coff; S.side_stride = d.side_stride; S.side_k = d.side_k;
    S.out_stride = d.out_stride; S.out_coff = d.out_coff;
    S.lds_off = -1; S.lds_stride = 0;
    return S;
}

bool chain_is_wide(long long R, int force, int max_workgroups) {
    static const bool on = env_flag("TT_CHAIN_WIDE", true);      // A/B knob: 0 = AUTO always takes the row form
    if (force != CHAIN_AUTO) return force != CHAIN_ROWS;
    const long long row_blocks = (R + 31) / 32;
    if (!on || row_blocks > kWideMaxRowBlocks) return false;
    // a small / partitioned device that cannot hold one workgroup per row group: the row form needs no co-residency
    return wide_row_groups(row_blocks) <= (max_workgroups < kWideRoom ? max_workgroups : kWideRoom);
}

int chain_wide_fits(const ChainChoice& c, int max_workgroups) {
    // the ticket barrier needs every workgroup of the launch running: beyond what the device holds beside a second launch the
    // first arrivals would spin until they give up
    TT_REQUIRE(c.row_groups * c.n_groups <= max_workgroups, "tt_mlp_chain_wide: %lld row groups x %d column groups: at most %d "
               "workgroups per launch can be guaranteed co-resident on this device", c.row_groups, c.n_groups, max_workgroups);
    return 0;
}

int chain_choose(long long R, int nstages, const tt_chain_stage* st, int n_split, int groups_hint, int force, int max_workgroups,
                 ChainChoice* out) {
    ChainChoice& c = *out;
    c = ChainChoice{};
    c.wide = chain_is_wide(R, force, max_workgroups);
    if (!c.wide) return rows_layout(R, nstages, st, n_split, &c);
    wide_layout(R, nstages, st, &c);
    if (force == CHAIN_WIDE_AS_GIVEN) {
        TT_REQUIRE(groups_hint >= 1 && groups_hint <= kWideMaxGroups, "tt_mlp_chain_wide: %d column groups: 1 - 64 workgroups per row "
                   "group can be co-resident", groups_hint);
        c.n_groups = groups_hint;
        if (max_workgroups >= 0)
            if (int rc = chain_wide_fits(c, max_workgroups)) return rc;
    } else {
        const int room = max_workgroups < kWideRoom ? max_workgroups : kWideRoom;
        TT_REQUIRE(c.row_groups <= room, "tt_mlp_chain_wide: %lld row groups cannot be co-resident on this device (%d)", c.row_groups,
                   room);          // (AUTO has taken the row form)
        int g = groups_hint;
        if (g <= 0) {
            for (int s = 0; s < nstages; ++s) g = g > (st[s].N + 31) / 32 ? g : (st[s].N + 31) / 32;
            if (g > kWideDefaultGroups) g = kWideDefaultGroups;
        }
        if (g > room / c.row_groups) g = (int)(room / c.row_groups);
        c.n_groups = g > kWideMaxGroups ? kWideMaxGroups : g;
    }
    if (c.n_groups == 1) {                 // one workgroup per row group: nobody to wait for
        for (int s = 0; s < nstages; ++s) c.sync_before[s] = 0;
        c.nsync = 0;
    }
    return 0;
}

}  // namespace tt

// (the wide placement alone, of stages nobody has validated: it reads N and in_sel and follows no index)
extern "C" long long tt_mlp_chain_wide_workspace_bytes(long long R, int nstages, const tt_chain_stage* st) {
    if (!st || R <= 0 || nstages < 1 || nstages > tt::kChainMaxStages) return -1;
    tt::ChainChoice c{};
    tt::wide_layout(R, nstages, st, &c);
    return c.workspace_bytes;
}

extern "C" int tt_mlp_chain_plan(long long R, int x_stride, int nstages, const tt_chain_stage* st, int n_split, int groups, int force,
                                 int max_workgroups, tt_chain_choice* out) {
    using namespace tt;
    TT_REQUIRE(out && force >= CHAIN_AUTO && force <= CHAIN_WIDE_AS_GIVEN && (max_workgroups >= 0 || force == CHAIN_ROWS),
               "tt_mlp_chain_plan: bad arguments");
    const char* who = chain_is_wide(R, force, max_workgroups) ? "tt_mlp_chain_wide" : "tt_mlp_chain";
    alignas(16) static const char no_input[16] = {};       // a plan has no input pointer: validated as an aligned one
    if (int rc = chain_validate(who, no_input, R, x_stride, nstages, st)) return rc;
    ChainChoice c;
    if (int rc = chain_choose(R, nstages, st, n_split, groups, force, max_workgroups, &c)) return rc;
    out->wide = c.wide;
    out->row_groups = c.row_groups;
    out->n_groups = c.n_groups;
    out->n_split = c.n_split;
    out->workspace_bytes = c.workspace_bytes;       // (0 for the row form, as dynamic_lds is for the wide form)
    out->dynamic_lds = (long long)c.lds_total;
    return 0;
}

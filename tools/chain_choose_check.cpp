// Stand-alone host program over csrc/chain_choose.cpp, for a sanitizer build: reads the sweep's case list from stdin
// (tools/chain_choice_sweep.py --cases: one call per line, refusals included), runs tt_mlp_chain_plan and prints every answer.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       thinktwice_amd/csrc/chain_choose.cpp tools/chain_choose_check.cpp -o tools/chain_choose_check
//   python tools/chain_choice_sweep.py --cases | tools/chain_choose_check
//
// Touches no device and loads nothing of the library but the chooser.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../thinktwice_amd/csrc/chain_choose.h"

namespace tt {                                    // common.cpp's, without the rest of the library
static char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
bool env_flag(const char* name, bool dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) != 0 : dflt;
}
}  // namespace tt

int main() {
    char line[1024];
    int n = 0;
    while (fgets(line, sizeof line, stdin)) {
        // R x_stride n_split groups force max_workgroups nstages, then K Kp N in_sel side_k per stage
        long long R;
        int x_stride, n_split, groups, force, max_wg, nstages, used = 0;
        if (sscanf(line, "%lld %d %d %d %d %d %d%n", &R, &x_stride, &n_split, &groups, &force, &max_wg, &nstages, &used) != 7) return 2;
        if (nstages < 1 || nstages > tt::kChainMaxStages) return 2;
        // exactly nstages elements on the heap: a read past the list is a sanitizer report
        std::vector<tt_chain_stage> st((size_t)nstages);
        const char* p = line + used;
        for (int s = 0; s < nstages; ++s) {
            int adv = 0;
            tt_chain_stage& d = st[(size_t)s];
            memset(&d, 0, sizeof d);
            if (sscanf(p, "%d %d %d %d %d%n", &d.K, &d.Kp, &d.N, &d.in_sel, &d.side_k, &adv) != 5) return 2;
            p += adv;
            d.w = reinterpret_cast<const void*>(0x100000);
            if (d.side_k) {
                d.side = reinterpret_cast<const float*>(0x4000000);
                d.side_w = reinterpret_cast<const float*>(0x200000);
            }
        }
        tt_chain_choice c;
        memset(&c, 0, sizeof c);
        const int rc = tt_mlp_chain_plan(R, x_stride, nstages, st.data(), n_split, groups, force, max_wg, &c);
        if (rc)
            printf("rc %d: %s\n", rc, tt::g_err);
        else
            printf("%s grid %lld x %d ws %lld lds %lld | query %lld\n", c.wide ? "tt_mlp_chain_wide" : "tt_mlp_chain", c.row_groups,
                   c.wide ? c.n_groups : c.n_split, c.workspace_bytes, c.dynamic_lds,
                   tt_mlp_chain_wide_workspace_bytes(R, nstages, st.data()));
        ++n;
    }
    printf("%d calls\n", n);
    return n ? 0 : 1;
}

// Stand-alone host program over csrc/voxel_pool_choose.cpp, for a sanitizer build: reads the sweep's case list from stdin
// (tools/voxel_pool_choice_sweep.py --cases: one call per line, refusals included), runs the choosers and prints every label.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       thinktwice_amd/csrc/voxel_pool_choose.cpp tools/voxel_pool_choose_check.cpp -o tools/voxel_pool_choose_check
//   python tools/voxel_pool_choice_sweep.py --cases | tools/voxel_pool_choose_check
//
// Touches no device and loads nothing of the library but the chooser.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../thinktwice_amd/csrc/voxel_pool_choose.h"

namespace tt {
bool env_flag(const char* name, bool dflt) {      // common.cpp's, without the rest of the library
    const char* v = getenv(name);
    return v ? atoi(v) != 0 : dflt;
}
}  // namespace tt

int main() {
    char line[512], label[512], tight[24];
    int n = 0;
    while (fgets(line, sizeof line, stdin)) {
        long long a[12];
        char kind[16], type[32] = "";
        if (sscanf(line, "%15s", kind) != 1) continue;
        if (!strcmp(kind, "pool")) {
            // pool B Np C X Y feats out ws ws_bytes ws_entry lds_granted
            if (sscanf(line, "%*s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7,
                       a + 8, a + 9, a + 10) != 11)
                return 2;
            tt::VoxelPoolCall k;
            k.B = (int)a[0]; k.Np = (int)a[1]; k.C = (int)a[2]; k.X = (int)a[3]; k.Y = (int)a[4];
            k.geom = (const void*)0x1000; k.feats = (const void*)a[5]; k.out = (const void*)a[6]; k.ws = (const void*)a[7];
            k.ws_bytes = a[8]; k.ws_entry = a[9] != 0; k.lds_granted = a[10] != 0;
            const tt::VoxelPoolChoice c = tt::voxel_pool_choose(k);
            tt::vp_label(c.launch, c.nlaunch, c.nv, c.rf, nullptr, c.ws_bytes, label, sizeof label);
            tt::vp_label(c.launch, c.nlaunch, c.nv, c.rf, nullptr, c.ws_bytes, tight, sizeof tight);      // a label buffer that is too short
            printf("%s | query %lld plan %zu planned %lld\n", label, tt::voxel_pool_workspace_bytes(k.B, k.Np, k.C, k.X, k.Y),
                   tt::vp_static_plan_layout(k.B, k.Np, k.X, k.Y).end, tt::vp_static_plan_layout(k.B, k.Np, k.X, k.Y).partial_bytes(k.C));
        } else if (!strcmp(kind, "lift")) {
            // lift B ncam D fH fW C X Y has_ws type
            if (sscanf(line, "%*s %lld %lld %lld %lld %lld %lld %lld %lld %lld %31[^\n]", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8,
                       type) != 10)
                return 2;
            const tt::LiftSplatChoice c = tt::lift_splat_choose((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6],
                                                                (int)a[7], a[8] != 0);
            tt::vp_label(c.launch, c.nlaunch, 0, 0, type, c.arm == tt::LS_STRIP_CELLS ? c.ws_bytes : 0, label, sizeof label);
            tt::vp_label(c.launch, c.nlaunch, 0, 0, type, c.ws_bytes, tight, sizeof tight);
            printf("%s | query %lld\n", label, c.ws_bytes);
        } else {
            return 2;
        }
        ++n;
    }
    printf("%d calls\n", n);
    return n ? 0 : 1;
}

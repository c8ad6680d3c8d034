// TEST INFRASTRUCTURE ONLY: the group observation's kernels (emloco_amd/csrc/crowd_people_kernels.hip) on the CPU with the launch
// shapes of crowd_capi.hip, all arrays on the host.  Built into its own library by tests/emu_crowd_people.py together with
// emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/crowd_people_kernels.hip"

static const char *g_why = "";

extern "C" const char *emu_crowd_people_error(void) { return g_why; }

// `grid` > 0: that many workgroups stride over the rows (the result does not depend on it)
extern "C" int emu_crowd_people(const EmlocoCrowdPeople *pp, const int32_t *env_ids, int n, int grid) {
    const char *why = emloco::crowd_people_refusal(pp, n);
    g_why = why ? why : "";
    if (why) return -1;
    const EmlocoCrowdPeople p = *pp;
    const int rows = env_ids ? n : p.n_env;
    if (rows == 0) return 0;
    emu::launch((unsigned)((p.n_env + 255) / 256), 256, [&] { emloco::crowd_people_roots_kernel(p); });
    const int blocks = (rows + emloco::kPeopleWaves - 1) / emloco::kPeopleWaves;
    const unsigned g = (unsigned)(grid > 0 && grid < blocks ? grid : blocks);
    emu::launch(g, emloco::kPeopleThreads, [&] { emloco::crowd_people_kernel(p, env_ids, rows); });
    blockIdx.x = 0;
    return 0;
}

// TEST INFRASTRUCTURE ONLY: the crowd spawn's kernels (emloco_amd/csrc/crowd_spawn_kernels.hip) on the CPU with the launch shapes of
// crowd_capi.hip, all arrays on the host.  Built into its own library by tests/emu_crowd_spawn.py together with emu_runtime.cpp.
#include "hip/hip_runtime.h"
// lock-step fibers run one at a time: a plain read-modify-write is atomic
static inline unsigned atomicMin(unsigned *p, unsigned v) { const unsigned o = *p; *p = v < o ? v : o; return o; }
#include "../../emloco_amd/csrc/crowd_spawn_kernels.hip"

static const char *g_why = "";

extern "C" const char *emu_crowd_spawn_error(void) { return g_why; }

extern "C" int emu_crowd_spawn(const EmlocoCrowdSpawn *sp, const int32_t *env_ids, int n, const float *u) {
    const char *why = emloco::crowd_spawn_refusal(sp, env_ids, n, u);
    g_why = why ? why : "";
    if (why) return -1;
    const EmlocoCrowdSpawn s = *sp;
    const int rows = env_ids ? n : s.n_env;
    if (rows == 0) return 0;
    emu::launch((unsigned)((rows + emloco::kSpawnMarkThreads - 1) / emloco::kSpawnMarkThreads), emloco::kSpawnMarkThreads,
                [&] { emloco::crowd_spawn_mark_kernel(s, env_ids, rows); });
    emu::launch((unsigned)(s.n_env / s.group_size), (unsigned)(s.tries * 64), [&] { emloco::crowd_spawn_place_kernel(s, u, rows); });
    blockIdx.x = 0;
    return 0;
}

// TEST INFRASTRUCTURE ONLY: the crowd sensor's kernels (emloco_amd/csrc/crowd_kernels.hip) on the CPU with the launch shapes of
// crowd_capi.hip, all arrays on the host.  Built into its own library by tests/emu_crowd.py together with emu_runtime.cpp.
#include "hip/hip_runtime.h"
// lock-step fibers run one at a time: a plain read-modify-write is atomic (the shared header has only atomicAdd(int *))
static inline unsigned atomicMax(unsigned *p, unsigned v) { const unsigned o = *p; if (v > o) *p = v; return o; }
#include "../../emloco_amd/csrc/crowd_kernels.hip"

static const char *g_crowd_why = "";

extern "C" const char *emu_crowd_error(void) { return g_crowd_why; }

// `grid` > 0: that many workgroups stride over the envs (the result does not depend on it)
extern "C" int emu_crowd_sensor(const EmlocoCrowdBufs *bufs, const int32_t *env_ids, int n, int grid) {
    const char *why = emloco::crowd_refusal(bufs, n);
    g_crowd_why = why ? why : "";
    if (why) return -1;
    const EmlocoCrowdBufs c = *bufs;
    const int rows = env_ids ? n : c.n_env;
    if (rows == 0) return 0;
    if (c.stamps) emu::launch((unsigned)(grid > 0 && grid < c.n_env ? grid : c.n_env), emloco::kCrowdThreads, [&] { emloco::crowd_stamp_kernel(c); });
    emu::launch((unsigned)(grid > 0 && grid < rows ? grid : rows), emloco::kCrowdThreads, [&] { emloco::crowd_gather_kernel(c, env_ids, rows); });
    blockIdx.x = 0;
    return 0;
}

// TEST INFRASTRUCTURE ONLY: runs traj_densify_kernel of emloco_amd/csrc/traj_kernels.hip on the CPU through tests/emu/hip/
// (tests/test_traj_densify_cpu.py compiles it with emu/emu_runtime.cpp).  Arguments as emloco_traj_densify (include/emloco_task.h), all
// arrays on the host; validation and packing are the product's own (emloco::densify_pack), the launch is the emulator's.
#include <stdint.h>
#include "hip/hip_runtime.h"
#include "../emloco_amd/csrc/traj_kernels.hip"

using namespace emloco;

static const char *g_why = "";

extern "C" const char *emu_traj_densify_error(void) { return g_why; }

extern "C" int emu_traj_densify(const float *knot_t, int n_knots, const float *way, int64_t n_traj, const float *query_t, int n_query,
                                float *out, uint8_t *valid, int flags) {
    DensifyArgs a;
    const char *why = densify_pack(knot_t, n_knots, (long long)n_traj, query_t, n_query, flags, &a);
    g_why = why ? why : "";
    if (why) return -1;
    if (n_traj == 0) return 0;
    if (!way || !out) return -1;
    emu::launch((unsigned)((n_traj + DENSIFY_TPB - 1) / DENSIFY_TPB), DENSIFY_THREADS, [&] { traj_densify_kernel(a, way, out, valid); });
    blockIdx.x = 0;
    return 0;
}

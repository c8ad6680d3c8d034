// TEST INFRASTRUCTURE ONLY: the get-up kernels (emloco_amd/csrc/getup_kernels.hip) on the CPU with the launch shapes of
// getup_capi.hip, all arrays on the host.  Built into its own library by tests/emu_getup.py together with emu_runtime.cpp.
#include <cstring>
#include "hip/hip_runtime.h"
// lock-step fibers run one at a time: a plain read-modify-write is atomic (the 64-bit form the statistics use)
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
#include "../../emloco_amd/csrc/getup_kernels.hip"

static unsigned list_grid(int n) { return (unsigned)(n < 256 ? n : 256); }

extern "C" int emu_getup_split(const EmlocoGetupBufs *g, const int32_t *ids, int n, const float *rnd, uint64_t seed, float recovery_prob,
                               float fall_prob, int recovery_steps, uint32_t slot_key, int32_t *normal, int32_t *fall, int32_t *recover,
                               int32_t *fall_slot) {
    emloco::GetupSplitArgs a;
    a.ids = ids; a.n = n;
    a.rnd = rnd; a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
    a.recovery_prob = recovery_prob; a.fall_prob = fall_prob; a.recovery_steps = recovery_steps; a.slot_key = slot_key;
    a.normal = normal; a.fall = fall; a.recover = recover; a.fall_slot = fall_slot;
    const EmlocoGetupBufs gb = *g;
    emu::launch(1, GETUP_SPLIT_THREADS, [&] { emloco::getup_split_kernel(gb, a); });
    return 0;
}

extern "C" int emu_getup_flags(const EmlocoGetupBufs *g) {
    const EmlocoGetupBufs gb = *g;
    emu::launch((unsigned)((gb.n_env + GETUP_FLAGS_THREADS - 1) / GETUP_FLAGS_THREADS), GETUP_FLAGS_THREADS, [&] { emloco::getup_flags_kernel(gb); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_getup_amp_default(float *amp_obs_buf, int amp_ring, const int32_t *ids, int n) {
    if (n < 1) return 0;
    emu::launch(list_grid(n), 64, [&] { emloco::getup_amp_default_kernel(amp_obs_buf, amp_ring, ids, n); });
    blockIdx.x = 0;
    return 0;
}

// the pool copy of emloco_getup_apply (the kinematics and the trajectory behind it are the reset chain's, run by emu_task.cpp)
extern "C" int emu_getup_copy(const EmlocoGetupBufs *g, float *root, float *dof, float *lambda_ws, const int32_t *fall, const int32_t *fall_slot, int n) {
    if (n < 1) return 0;
    EmlocoSimDev d; memset(&d, 0, sizeof(d));
    d.n_env = g->n_env; d.root_state = root; d.dof_state = dof; d.lambda_ws = lambda_ws;
    const EmlocoGetupBufs gb = *g;
    emu::launch(list_grid(n), 64, [&] { emloco::getup_copy_kernel(gb, d, fall, fall_slot, n); });
    blockIdx.x = 0;
    return 0;
}

// getup_capi.hip -- C ABI (include/emloco_task.h) over the get-up task's reset kernels.
#include <hip/hip_runtime.h>
#include "getup_kernels.hip"
#include "sim_state.h"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
// the structure's own buffers, which every entry point that takes it needs
bool getup_incomplete(const EmlocoGetupBufs *g) {
    return g->n_env < 1 || g->n_pool < 1 || !g->pool_root || !g->pool_dof || !g->pool_taken || !g->assign || !g->recovery_counter ||
           !g->progress_buf || !g->reset_buf || !g->terminate_buf || !g->split_ws;
}
}  // namespace

extern "C" {

int emloco_getup_split(const EmlocoGetupBufs *g, const int32_t *dev_env_ids, int n, const float *dev_rnd, uint64_t seed,
                       float recovery_prob, float fall_prob, int recovery_steps, uint32_t slot_key, int32_t *dev_normal,
                       int32_t *dev_fall, int32_t *dev_recover, int32_t *dev_fall_slot, void *stream) {
    const char *who = "emloco_getup_split";
    if (!g || !dev_env_ids || !dev_normal || !dev_fall || !dev_recover || !dev_fall_slot) return capi_fail(EMLOCO_E_ARG, who, "null argument");
    if (getup_incomplete(g)) return capi_fail(EMLOCO_E_ARG, who, "missing buffers");
    if (n < 0 || n > g->n_env) return capi_fail(EMLOCO_E_ARG, who, "bad env count");
    if (recovery_steps < 0) return capi_fail(EMLOCO_E_ARG, who, "negative recovery_steps");
    emloco::GetupSplitArgs a;
    a.ids = dev_env_ids; a.n = n;
    a.rnd = dev_rnd; a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
    a.recovery_prob = recovery_prob; a.fall_prob = fall_prob; a.recovery_steps = recovery_steps; a.slot_key = slot_key;
    a.normal = dev_normal; a.fall = dev_fall; a.recover = dev_recover; a.fall_slot = dev_fall_slot;
    hipLaunchKernelGGL(emloco::getup_split_kernel, dim3(1), dim3(GETUP_SPLIT_THREADS), 0, (hipStream_t)stream, *g, a);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_getup_apply(EmlocoSim *sim, const EmlocoResetBufs *b, const EmlocoGetupBufs *g, const int32_t *dev_fall,
                       const int32_t *dev_fall_slot, const int32_t *dev_recover, int n, const float *dev_rnd_fall,
                       const float *dev_rnd_recover, uint64_t seed, float *dev_rnd_ws, void *stream) {
    const char *who = "emloco_getup_apply";
    if (!sim || !b || !g || !dev_fall || !dev_fall_slot || !dev_recover) return capi_fail(EMLOCO_E_ARG, who, "null argument");
    if (!sim->prepared) return capi_fail(EMLOCO_E_STATE, who, "sim not prepared");
    if (n < 0 || n > sim->n_env || g->n_env != sim->n_env) return capi_fail(EMLOCO_E_ARG, who, "bad env count");
    if ((dev_rnd_fall == nullptr) != (dev_rnd_recover == nullptr)) return capi_fail(EMLOCO_E_ARG, who, "the two lists' random rows go together");
    if (!dev_rnd_fall && !dev_rnd_ws) return capi_fail(EMLOCO_E_ARG, who, "neither random rows nor a workspace for them");
    if (getup_incomplete(g)) return capi_fail(EMLOCO_E_ARG, who, "missing get-up buffers");
    if (!b->traj_verts || !b->inverted || !b->progress_buf || !b->reset_buf || !b->terminate_buf || !b->waypoint_traj || !b->init_pose ||
        !b->init_vel)
        return capi_fail(EMLOCO_E_ARG, who, "missing reset buffers");
    if ((b->flags & EMLOCO_RESET_REAL_PATH) && b->n_real > 0 && !b->real_traj) return capi_fail(EMLOCO_E_ARG, who, "real_path without data");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned half = list_grid(n);
    EmlocoResetBufs keyed = *b;
    if (!dev_rnd_fall) {
        hipLaunchKernelGGL(emloco::getup_fill_rnd_kernel, dim3(2 * half), dim3(64), 0, st, dev_fall, dev_recover, n, (int)half,
                           (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), dev_rnd_ws);
        EMLOCO_HIPCHK(hipGetLastError());
        dev_rnd_fall = dev_rnd_ws;
        dev_rnd_recover = dev_rnd_ws + (size_t)n * EMLOCO_RESET_RND;
        keyed.real_pick = nullptr;              // a fresh real-path permutation per call, as emloco_task_reset_seeded
        keyed.real_pick_key = (uint32_t)((seed * 0xD6E8FEB86659FD93ull) >> 32);
    }
    hipLaunchKernelGGL(emloco::getup_copy_kernel, dim3(half), dim3(64), 0, st, *g, sim->dev, dev_fall, dev_fall_slot, n);
    EMLOCO_HIPCHK(hipGetLastError());
    const int rc = emloco_sim_fk_indexed(sim, dev_fall, n, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(emloco::getup_finish_kernel, dim3(2 * half), dim3(64), 0, st, keyed, sim->dev, dev_fall, dev_recover, n, (int)half,
                       dev_rnd_fall, dev_rnd_recover);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_getup_amp_default(const EmlocoTaskBufs *bufs, const int32_t *dev_env_ids, int n, void *stream) {
    const char *who = "emloco_getup_amp_default";
    if (!bufs || !dev_env_ids) return capi_fail(EMLOCO_E_ARG, who, "null argument");
    if (n < 0 || n > bufs->n_env) return capi_fail(EMLOCO_E_ARG, who, "bad env count");
    if (!bufs->amp_obs_buf || bufs->amp_ring < 0 || bufs->amp_ring > EMLOCO_AMP_STEPS) return capi_fail(EMLOCO_E_ARG, who, "missing AMP buffer");
    if (n == 0) return 0;
    hipLaunchKernelGGL(emloco::getup_amp_default_kernel, dim3(list_grid(n)), dim3(64), 0, (hipStream_t)stream, bufs->amp_obs_buf,
                       bufs->amp_ring, dev_env_ids, n);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_getup_flags(const EmlocoGetupBufs *g, void *stream) {
    const char *who = "emloco_getup_flags";
    if (!g) return capi_fail(EMLOCO_E_ARG, who, "null argument");
    if (getup_incomplete(g)) return capi_fail(EMLOCO_E_ARG, who, "missing buffers");
    const unsigned grid = (unsigned)((g->n_env + GETUP_FLAGS_THREADS - 1) / GETUP_FLAGS_THREADS);
    hipLaunchKernelGGL(emloco::getup_flags_kernel, dim3(grid), dim3(GETUP_FLAGS_THREADS), 0, (hipStream_t)stream, *g);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"

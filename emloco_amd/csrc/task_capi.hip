// task_capi.hip -- C ABI (include/emloco_task.h) over the fused post-physics kernels.
#include <hip/hip_runtime.h>
#include "task_kernels.hip"
#include "reset_kernels.hip"
#include "chain_kernels.hip"
#include "traj_kernels.hip"
#include "episode_stats_kernels.hip"
#include "sim_state.h"
#include "../../include/emloco_predictor.h"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
hipEvent_t g_ev0 = nullptr, g_ev1 = nullptr;
bool g_timing = false, g_pending = false;
float g_last_ms = -1.0f;
long long *g_chain_prof = nullptr;
// an AMP row holds 12 root values, 6 per subset joint, the subset's velocities, 12 key-body values and 11 betas: 35 + 3 n_sub values,
// which must fit EMLOCO_AMP_ROW (a wider row would run into the next row and past the last one)
bool bad_dof_subset(int n_sub) { return n_sub < 0 || n_sub % 3 != 0 || 35 + 3 * n_sub > EMLOCO_AMP_ROW; }
// the buffers every reset needs (emloco_task_reset, emloco_task_reset_seeded, emloco_task_reset_obs)
bool reset_bufs_complete(const EmlocoResetBufs *b) {
    return b->gts && b->grs && b->lrs && b->gvs && b->gavs && b->dvs && b->motion_len && b->motion_dt && b->motion_nframes &&
           b->motion_start && b->n_motions >= 1 && b->heightfield && b->betas && b->key_bodies && b->dof_subset && b->traj_verts &&
           b->inverted && b->progress_buf && b->reset_buf && b->terminate_buf && b->waypoint_traj && b->init_pose && b->init_vel &&
           b->amp_obs_buf && b->motion_ids && b->motion_times && b->ground_h;
}
}  // namespace

extern "C" {

int emloco_task_enable_timing(int on) {
    if (on && !g_ev0) {
        EMLOCO_HIPCHK(hipEventCreate(&g_ev0));
        EMLOCO_HIPCHK(hipEventCreate(&g_ev1));
    }
    g_timing = on != 0;
    return 0;
}

float emloco_task_last_ms(void) {
    if (g_pending) {
        if (hipEventSynchronize(g_ev1) == hipSuccess) {
            float ms = -1.0f;
            if (hipEventElapsedTime(&ms, g_ev0, g_ev1) == hipSuccess) g_last_ms = ms;
        }
        g_pending = false;
    }
    return g_last_ms;
}

int emloco_task_post_physics(const EmlocoTaskBufs *b, int mode, const int32_t *dev_env_ids, int n, void *stream) {
    if (!b) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: null buffers");
    if (b->n_env < 1 || b->hf_rows < 2 || b->hf_cols < 2) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: bad sizes");
    if (!b->rb_state || !b->progress_buf || !b->traj_verts) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: missing tensors");
    if ((mode & EMLOCO_POST_OBS) && (!b->obs_buf || !b->flip_obs_buf || !b->heightfield || !b->betas || !b->left_to_right))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: observation buffers missing");
    if ((mode & EMLOCO_POST_REWARD) && (!b->rew_buf || !b->reward_raw || !b->dof_force || !b->dof_state))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: reward buffers missing");
    if ((mode & EMLOCO_POST_SKIP_DONE) && !b->reset_buf) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: SKIP_DONE needs reset_buf");
    if ((mode & EMLOCO_POST_RESET) && (!b->reset_buf || !b->terminate_buf || !b->contact_force || !b->contact_body_mask))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: reset buffers missing");
    if ((mode & (EMLOCO_POST_AMP_ROW | EMLOCO_POST_AMP_SHIFT)) && (!b->amp_obs_buf || !b->dof_subset || !b->key_bodies || bad_dof_subset(b->n_dof_subset)))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: AMP buffers missing");
    const int count = dev_env_ids ? n : b->n_env;
    if (count < 0 || count > b->n_env) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics: bad env count");
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (g_timing) EMLOCO_HIPCHK(hipEventRecord(g_ev0, st));
    hipLaunchKernelGGL(emloco::post_physics_kernel, dim3((unsigned)count), dim3(64), 0, st, *b, mode, dev_env_ids, count);
    EMLOCO_HIPCHK(hipGetLastError());
    if (g_timing) { EMLOCO_HIPCHK(hipEventRecord(g_ev1, st)); g_pending = true; }
    return 0;
}

int emloco_task_post_physics_returns(const EmlocoTaskBufs *b, int mode, const void *step_, const uint8_t *dev_inverted, void *stream) {
    const EmlocoLocoValStep *step = (const EmlocoLocoValStep *)step_;
    if (!b || !step) return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: null argument");
    if (!(mode & EMLOCO_POST_REWARD) || !(mode & EMLOCO_POST_RESET) || (mode & EMLOCO_POST_SKIP_DONE))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: the return bookkeeping follows the reward and the reset flag of the same launch, for every env");
    if (step->n_env != b->n_env || !step->current_rewards || !step->current_lengths || !step->current_combined_rewards || !step->discount_coefs ||
        !step->waypoint_traj || !step->init_pose || !step->init_vel || !step->traj13 || !step->pose || !step->vel || !step->target || !step->weight)
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: LocoVal step buffers missing or for another env count");
    if ((step->staged_reward == nullptr) != (step->staged_done == nullptr))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: staged_reward and staged_done go together");
    if (b->n_env < 1 || b->hf_rows < 2 || b->hf_cols < 2 || !b->rb_state || !b->progress_buf || !b->traj_verts || !b->rew_buf || !b->reward_raw ||
        !b->dof_force || !b->dof_state || !b->reset_buf || !b->terminate_buf || !b->contact_force || !b->contact_body_mask)
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: task buffers missing");
    if ((mode & EMLOCO_POST_OBS) && (!b->obs_buf || !b->flip_obs_buf || !b->heightfield || !b->betas || !b->left_to_right))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: observation buffers missing");
    if ((mode & (EMLOCO_POST_AMP_ROW | EMLOCO_POST_AMP_SHIFT)) && (!b->amp_obs_buf || !b->dof_subset || !b->key_bodies || !b->betas || bad_dof_subset(b->n_dof_subset)))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_post_physics_returns: AMP buffers missing");
    hipStream_t st = (hipStream_t)stream;
    if (g_timing) EMLOCO_HIPCHK(hipEventRecord(g_ev0, st));
    hipLaunchKernelGGL(emloco::post_physics_returns_kernel, dim3((unsigned)b->n_env), dim3(64), 0, st, *b, mode, *step, dev_inverted);
    EMLOCO_HIPCHK(hipGetLastError());
    if (g_timing) { EMLOCO_HIPCHK(hipEventRecord(g_ev1, st)); g_pending = true; }
    return 0;
}

int emloco_task_amp_rows(int n, const float *root_pos, const float *root_rot, const float *root_vel,
                         const float *root_ang_vel, const float *dof_pos, const float *dof_vel,
                         const float *key_pos, const float *betas, const int32_t *dof_subset,
                         int n_dof_subset, float *out, void *stream) {
    if (n < 0 || !root_pos || !root_rot || !root_vel || !root_ang_vel || !dof_pos || !dof_vel || !key_pos || !betas || !dof_subset || !out)
        return capi_fail(EMLOCO_E_ARG, "emloco_task_amp_rows: bad argument");
    if (bad_dof_subset(n_dof_subset)) return capi_fail(EMLOCO_E_ARG, "emloco_task_amp_rows: dof subset must be a multiple of 3 in [0, 57] (a row of 35 + 3 n values within 206)");
    if (n == 0) return 0;
    hipLaunchKernelGGL(emloco::amp_rows_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, n, root_pos, root_rot,
                       root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, betas, dof_subset, n_dof_subset, out);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

// what emloco_task_reset refuses, ahead of every launch (emloco_task_reset_seeded checks the same before it fills the random rows);
// `who` names the entry point in the message.  0: go on, 1: nothing to do (n == 0), else the error code
static int reset_refused(const char *who, const EmlocoSim *sim, const EmlocoResetBufs *b, const int32_t *dev_env_ids, int n, const float *dev_rnd) {
    if (!sim || !b || !dev_env_ids || !dev_rnd) return capi_fail(EMLOCO_E_ARG, who, "null argument");
    if (!sim->prepared) return capi_fail(EMLOCO_E_STATE, who, "sim not prepared");
    if (n < 0 || n > sim->n_env) return capi_fail(EMLOCO_E_ARG, who, "bad env count");
    if (n == 0) return 1;
    if (!reset_bufs_complete(b)) return capi_fail(EMLOCO_E_ARG, who, "missing buffers");
    if (!(b->flags & EMLOCO_RESET_FIXED_LOCATION) && (!b->valid_x || !b->valid_y || b->n_valid < 1)) return capi_fail(EMLOCO_E_ARG, who, "no valid locations");
    if ((b->flags & EMLOCO_RESET_REAL_PATH) && b->n_real > 0 && !b->real_traj) return capi_fail(EMLOCO_E_ARG, who, "real_path without data");
    return 0;
}

int emloco_task_reset(EmlocoSim *sim, const EmlocoResetBufs *b, const int32_t *dev_env_ids, int n, const float *dev_rnd, void *stream) {
    const int refused = reset_refused("emloco_task_reset", sim, b, dev_env_ids, n, dev_rnd);
    if (refused) return refused == 1 ? 0 : refused;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = list_grid(n);
    hipLaunchKernelGGL(emloco::reset_sample_kernel, dim3(grid), dim3(64), 0, st, *b, sim->dev, dev_env_ids, n, dev_rnd);
    EMLOCO_HIPCHK(hipGetLastError());
    const int rc = emloco_sim_fk_indexed(sim, dev_env_ids, n, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(emloco::reset_finish_kernel, dim3(grid), dim3(64), 0, st, *b, sim->dev, dev_env_ids, n, dev_rnd);
    EMLOCO_HIPCHK(hipGetLastError());
    if (b->flags & EMLOCO_RESET_NO_AMP_HISTORY) return 0;
    hipLaunchKernelGGL(emloco::reset_amp_history_kernel, dim3(grid, EMLOCO_AMP_STEPS - 1), dim3(64), 0, st, *b, dev_env_ids, n);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_reset_amp_history(const EmlocoResetBufs *b, const int32_t *dev_env_ids, int n, void *stream) {
    if (!b || !dev_env_ids) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_amp_history: null argument");
    if (n < 0) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_amp_history: bad env count");
    if (n == 0) return 0;
    if (!b->gts || !b->grs || !b->lrs || !b->gvs || !b->gavs || !b->dvs || !b->motion_len || !b->motion_dt || !b->motion_nframes ||
        !b->motion_start || !b->betas || !b->key_bodies || !b->dof_subset || !b->amp_obs_buf || !b->motion_ids || !b->motion_times)
        return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_amp_history: missing buffers");
    const unsigned grid = list_grid(n);
    hipLaunchKernelGGL(emloco::reset_amp_history_kernel, dim3(grid, EMLOCO_AMP_STEPS - 1), dim3(64), 0, (hipStream_t)stream, *b, dev_env_ids, n);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_reset_seeded(EmlocoSim *sim, const EmlocoResetBufs *b, const int32_t *dev_env_ids, int n, uint64_t seed,
                             float *dev_rnd_ws, void *stream) {
    // everything emloco_task_reset refuses is refused here, before the random rows are written
    const int refused = reset_refused("emloco_task_reset_seeded", sim, b, dev_env_ids, n, dev_rnd_ws);
    if (refused) return refused == 1 ? 0 : refused;
    const unsigned grid = list_grid(n);
    hipLaunchKernelGGL(emloco::reset_fill_rnd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, dev_env_ids, n,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), dev_rnd_ws);
    EMLOCO_HIPCHK(hipGetLastError());
    EmlocoResetBufs keyed = *b;                 // a fresh real-path permutation per call (reset_kernels.hip: real_pick_perm)
    keyed.real_pick = nullptr;
    keyed.real_pick_key = (uint32_t)((seed * 0xD6E8FEB86659FD93ull) >> 32);
    return emloco_task_reset(sim, &keyed, dev_env_ids, n, dev_rnd_ws, stream);
}

int emloco_task_traj_reset(const EmlocoResetBufs *b, const int32_t *dev_env_ids, int n, const float *dev_rnd,
                           const float *dev_init_pos, const float *dev_root_vel, void *stream) {
    if (!b || !dev_env_ids || !dev_rnd || !dev_init_pos || !dev_root_vel) return capi_fail(EMLOCO_E_ARG, "emloco_task_traj_reset: null argument");
    if (n < 0) return capi_fail(EMLOCO_E_ARG, "emloco_task_traj_reset: bad env count");
    if (n == 0) return 0;
    if (!b->traj_verts || !b->inverted) return capi_fail(EMLOCO_E_ARG, "emloco_task_traj_reset: missing buffers");
    if ((b->flags & EMLOCO_RESET_REAL_PATH) && b->n_real > 0 && !b->real_traj) return capi_fail(EMLOCO_E_ARG, "emloco_task_traj_reset: real_path without data");
    const unsigned grid = list_grid(n);
    hipLaunchKernelGGL(emloco::traj_reset_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, *b, dev_env_ids, n, dev_rnd,
                       dev_init_pos, dev_root_vel);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_get_heights(const int16_t *dev_heightfield, int rows, int cols, float hscale, float vscale, const float *dev_pose7,
                            int n, int grid, float *dev_heights, int64_t *dev_px, int64_t *dev_py, void *stream) {
    if (!dev_heightfield || !dev_pose7 || rows < 2 || cols < 2 || n < 0) return capi_fail(EMLOCO_E_ARG, "emloco_task_get_heights: bad argument");
    if ((dev_px == nullptr) != (dev_py == nullptr)) return capi_fail(EMLOCO_E_ARG, "emloco_task_get_heights: px and py go together");
    if (n == 0) return 0;
    hipLaunchKernelGGL(emloco::get_heights_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, dev_heightfield, rows, cols,
                       hscale, vscale, dev_pose7, n, grid, dev_heights, dev_px, dev_py);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_compact_done_snapshot(const int64_t *dev_flags, int n, int32_t *dev_ids, int64_t *dev_snapshot, void *stream) {
    if (!dev_flags || !dev_ids || n < 1) return capi_fail(EMLOCO_E_ARG, "emloco_task_compact_done: bad argument (ids holds n + 1 entries)");
    hipLaunchKernelGGL(emloco::compact_flags_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dev_flags, n, dev_ids, dev_snapshot);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_compact_done(const int64_t *dev_flags, int n, int32_t *dev_ids, void *stream) {
    return emloco_task_compact_done_snapshot(dev_flags, n, dev_ids, nullptr, stream);
}

int emloco_task_pd_targets_copy(int n_env, const float *actions, const float *offset, const float *scale,
                                const uint8_t *zero_mask, float *pd_targets, float *actions_copy, void *stream) {
    if (n_env < 1 || !actions || !offset || !scale || !zero_mask || !pd_targets) return capi_fail(EMLOCO_E_ARG, "emloco_task_pd_targets: bad argument");
    if (actions_copy == actions) actions_copy = nullptr;
    const int total = n_env * 69;
    hipLaunchKernelGGL(emloco::pd_targets_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       total, actions, offset, scale, zero_mask, pd_targets, actions_copy);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_pd_targets(int n_env, const float *actions, const float *offset, const float *scale,
                           const uint8_t *zero_mask, float *pd_targets, void *stream) {
    return emloco_task_pd_targets_copy(n_env, actions, offset, scale, zero_mask, pd_targets, nullptr, stream);
}

int emloco_task_compact_done_order(EmlocoSim *sim, const int64_t *dev_flags, int n, int32_t *dev_ids, int64_t *dev_snapshot, void *stream) {
    if (!dev_flags || !dev_ids || n < 1) return capi_fail(EMLOCO_E_ARG, "emloco_task_compact_done_order: bad argument (ids holds n + 1 entries)");
    const bool sort = sim && sim->prepared && sim->cost_order && sim->d_ticks.p && sim->d_order.p;
    hipLaunchKernelGGL(emloco::compact_order_kernel, dim3(sort ? 2 : 1), dim3(1024), 0, (hipStream_t)stream, dev_flags, n, dev_ids, dev_snapshot,
                       sort ? sim->d_ticks.p : nullptr, sort ? sim->n_env : 0, sort ? sim->d_order.p : nullptr, sort ? sim->d_order_ws.p : nullptr);
    EMLOCO_HIPCHK(hipGetLastError());
    if (sort) sim->order_ready = true;
    return 0;
}

int emloco_task_reset_obs_pooled(EmlocoSim *sim, const EmlocoResetBufs *rb, const EmlocoTaskBufs *pb, int live_mode, const int64_t *dev_skip,
                                 const int32_t *dev_env_ids, int n, uint64_t seed, float *dev_rnd_ws, const float *dev_rnd,
                                 const EmlocoResetPool *pool, void *stream);

// internal diagnostic (not in the header): the first call allocates 16 wall-clock stamps (100 MHz) that every later
// emloco_task_reset_obs launch overwrites -- [0..5] reset slot 0: start, random row, sample, kinematics, finish, observations;
// [6, 7] last AMP history row of entry 0; [8, 9] / [10, 11] the observation workgroups of env 0 / the last env -- and copies them out
int emloco_task_chain_profile(long long *host16) {
    if (!g_chain_prof) { EMLOCO_HIPCHK(hipMalloc((void **)&g_chain_prof, 16 * sizeof(long long))); EMLOCO_HIPCHK(hipMemset(g_chain_prof, 0, 16 * sizeof(long long))); }
    EMLOCO_HIPCHK(hipDeviceSynchronize());
    if (host16) EMLOCO_HIPCHK(hipMemcpy(host16, g_chain_prof, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

#ifdef EMLOCO_POST_PROFILE
// internal diagnostic (builds with -DEMLOCO_POST_PROFILE only): 8 wall-clock stamps of the last env's post-physics workgroup
int emloco_task_post_profile(long long *host8) {
    static long long *buf = nullptr;
    if (!buf) {
        EMLOCO_HIPCHK(hipMalloc((void **)&buf, 8 * sizeof(long long)));
        EMLOCO_HIPCHK(hipMemset(buf, 0, 8 * sizeof(long long)));
        EMLOCO_HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(emloco::g_post_prof), &buf, sizeof(buf)));
    }
    EMLOCO_HIPCHK(hipDeviceSynchronize());
    if (host8) EMLOCO_HIPCHK(hipMemcpy(host8, buf, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}
#endif

int emloco_task_reset_obs(EmlocoSim *sim, const EmlocoResetBufs *rb, const EmlocoTaskBufs *pb, int live_mode, const int64_t *dev_skip,
                          const int32_t *dev_env_ids, int n, uint64_t seed, float *dev_rnd_ws, const float *dev_rnd, void *stream) {
    return emloco_task_reset_obs_pooled(sim, rb, pb, live_mode, dev_skip, dev_env_ids, n, seed, dev_rnd_ws, dev_rnd, nullptr, stream);
}

int emloco_task_reset_obs_pooled(EmlocoSim *sim, const EmlocoResetBufs *rb, const EmlocoTaskBufs *pb, int live_mode, const int64_t *dev_skip,
                                 const int32_t *dev_env_ids, int n, uint64_t seed, float *dev_rnd_ws, const float *dev_rnd,
                                 const EmlocoResetPool *pool, void *stream) {
    if (!sim || !rb || !pb || !dev_env_ids) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: null argument");
    if (const char *why = emloco::chain_pool_error(pool)) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs", why);
    if (!sim->prepared) return capi_fail(EMLOCO_E_STATE, "emloco_task_reset_obs: sim not prepared");
    if (n < 0 || n > sim->n_env) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: bad env count");
    if (!dev_rnd && !dev_rnd_ws) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: neither random rows nor a workspace for them");
    if (live_mode && !dev_skip) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: the live envs' role needs the flag snapshot");
    if (live_mode & ~(EMLOCO_POST_OBS | EMLOCO_POST_AMP_SHIFT | EMLOCO_POST_AMP_ROW | EMLOCO_POST_SKIP_DONE))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: the live envs' role builds observations / AMP rows only (progress, reward and flags belong to the flags launch)");
    if (pb->n_env != sim->n_env) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: task buffers and simulator disagree on the env count");
    const EmlocoResetBufs *b = rb;
    if (!reset_bufs_complete(b)) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: missing reset buffers");
    if (!(b->flags & EMLOCO_RESET_FIXED_LOCATION) && (!b->valid_x || !b->valid_y || b->n_valid < 1))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: no valid locations");
    if ((b->flags & EMLOCO_RESET_REAL_PATH) && b->n_real > 0 && !b->real_traj) return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: real_path without data");
    if (!pb->rb_state || !pb->progress_buf || !pb->traj_verts || !pb->obs_buf || !pb->flip_obs_buf || !pb->heightfield || !pb->betas ||
        !pb->left_to_right || !pb->amp_obs_buf || !pb->dof_subset || !pb->key_bodies || !pb->dof_state || bad_dof_subset(pb->n_dof_subset))
        return capi_fail(EMLOCO_E_ARG, "emloco_task_reset_obs: missing observation buffers");
    emloco::ChainArgs a;
    EmlocoResetBufs keyed;
    const unsigned grid = emloco::chain_pack(*rb, pb->n_env, live_mode, dev_skip, dev_env_ids, n, seed, dev_rnd_ws, dev_rnd, pool, g_chain_prof, &a, &keyed);
    if (grid == 0) return 0;
    hipLaunchKernelGGL(emloco::reset_obs_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, *pb, keyed, sim->dev, a);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_traj_densify(const float *knot_t, int n_knots, const float *dev_way, int64_t n_traj, const float *query_t, int n_query,
                        float *dev_out, uint8_t *dev_valid, int flags, void *stream) {
    static_assert(EMLOCO_DENSIFY_ORIGIN == emloco::DENSIFY_FLAG_ORIGIN && EMLOCO_DENSIFY_MAX_KNOTS == emloco::DENSIFY_MAX_KNOTS &&
                  EMLOCO_DENSIFY_MAX_QUERY == emloco::DENSIFY_MAX_QUERY, "include/emloco_task.h and traj_kernels.hip disagree");
    emloco::DensifyArgs a;
    const char *why = emloco::densify_pack(knot_t, n_knots, (long long)n_traj, query_t, n_query, flags, &a);
    if (why) return capi_fail(EMLOCO_E_ARG, "emloco_traj_densify", why);
    if (n_traj == 0) return 0;
    if (!dev_way || !dev_out) return capi_fail(EMLOCO_E_ARG, "emloco_traj_densify: null waypoints or output");
    const unsigned grid = (unsigned)((n_traj + emloco::DENSIFY_TPB - 1) / emloco::DENSIFY_TPB);
    hipLaunchKernelGGL(emloco::traj_densify_kernel, dim3(grid), dim3(emloco::DENSIFY_THREADS), 0, (hipStream_t)stream, a, dev_way, dev_out, dev_valid);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_episode_stats_step(int n_envs, const float *dev_rew_buf, const float *dev_reward_raw, const int64_t *dev_reset_buf,
                              const int64_t *dev_terminate_buf, const int64_t *dev_progress_buf, const float *dev_rb_state,
                              const float *dev_traj_verts, const uint8_t *dev_inverted, float inversion_scale, float dt, float traj_dur,
                              float fail_dist, float *dev_running, double *dev_totals, float *dev_game_out, void *stream) {
    static_assert(EMLOCO_EPM_TIMEOUT == EMLOCO_EPM_GAMES + EMLOCO_EPISODE_TIMEOUT && EMLOCO_EPM_FAR == EMLOCO_EPM_GAMES + EMLOCO_EPISODE_FAR &&
                  EMLOCO_EPM_FALLEN == EMLOCO_EPM_GAMES + EMLOCO_EPISODE_FALLEN, "the cause counters follow the game counter");
    if (!dev_rew_buf || !dev_reward_raw || !dev_reset_buf || !dev_terminate_buf || !dev_progress_buf || !dev_rb_state || !dev_traj_verts ||
        !dev_running || !dev_totals)
        return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_step: null buffer");
    if (n_envs <= 0) return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_step: bad env count");
    const auto positive = [](float x) { return x > 0.0f && x <= 3.402823466e38f; };
    if (!positive(fail_dist) || !positive(dt) || !positive(traj_dur))
        return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_step: fail_dist, dt and traj_dur must be positive and finite");
    if (dev_inverted && !(fabsf(inversion_scale) <= 3.402823466e38f)) return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_step: bad inversion scale");
    emloco::EpisodeStatsArgs a;
    a.n_env = n_envs;
    a.rew_buf = dev_rew_buf; a.reward_raw = dev_reward_raw;
    a.reset_buf = dev_reset_buf; a.terminate_buf = dev_terminate_buf; a.progress_buf = dev_progress_buf;
    a.rb_state = dev_rb_state; a.traj_verts = dev_traj_verts;
    a.inverted = dev_inverted; a.neg_scale = -inversion_scale;
    a.dt = dt; a.traj_dur = traj_dur; a.fail_dist = fail_dist;
    a.running = dev_running; a.totals = dev_totals; a.game_out = dev_game_out;
    const unsigned grid = (unsigned)((n_envs + emloco::kStatsWaves - 1) / emloco::kStatsWaves);
    hipLaunchKernelGGL(emloco::episode_stats_step_kernel, dim3(grid), dim3(64 * emloco::kStatsWaves), 0, (hipStream_t)stream, a);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_episode_stats_reduce(int n_envs, double *dev_totals, double *dev_moments, void *stream) {
    if (!dev_totals || !dev_moments) return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_reduce: null buffer");
    if (n_envs <= 0) return capi_fail(EMLOCO_E_ARG, "emloco_episode_stats_reduce: bad env count");
    hipLaunchKernelGGL(emloco::episode_stats_reduce_kernel, dim3(1), dim3(emloco::kStatsReduceThreads), 0, (hipStream_t)stream, n_envs,
                       dev_totals, dev_moments);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"

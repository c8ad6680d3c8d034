// episode_stats_kernels.hip -- the game statistics of a training run, kept on the device (include/emloco_task.h:
// emloco_episode_stats_step / emloco_episode_stats_reduce).  Included by task_capi.hip, which is built without fused-multiply-add
// contraction: the float32 running sums are plain adds in step order, the numpy restatement with the tests gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "task_device.h"

namespace emloco {

// the maximum over a wave on the DPP crossbar, as wave_sum (dev_math.h): the four permutations leave a 16-lane row's maximum in every
// lane of the row, the four row maxima are folded in a fixed order.  No NaN may come in (the caller replaces it): plain compares.
__device__ __forceinline__ float fmax_plain(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float wave_max(float v) {
    v = fmax_plain(v, dpp_mov<0x140>(v));   // row_mirror
    v = fmax_plain(v, dpp_mov<0x141>(v));   // row_half_mirror
    v = fmax_plain(v, dpp_mov<0xB1>(v));    // quad_perm [1,0,3,2]
    v = fmax_plain(v, dpp_mov<0x4E>(v));    // quad_perm [2,3,0,1]
    return fmax_plain(fmax_plain(fmax_plain(lane_bcast(v, 0), lane_bcast(v, 16)), lane_bcast(v, 32)), lane_bcast(v, 48));
}

struct EpisodeStatsArgs {
    int n_env;
    const float *rew_buf, *reward_raw;
    const int64_t *reset_buf, *terminate_buf, *progress_buf;
    const float *rb_state, *traj_verts;
    const uint8_t *inverted;                 // or NULL
    float neg_scale;                         // -inversion_penalty_scale
    float dt, traj_dur, fail_dist;
    float *running;                          // [E][EMLOCO_EPISODE_RUNNING]
    double *totals;                          // [E][EMLOCO_EPISODE_MOMENTS]
    float *game_out;                         // [E][EMLOCO_EPISODE_GAME_OUT] or NULL
};

constexpr int kStatsWaves = 4;               // envs per workgroup: one 64-lane wave each

// One wave per env, kStatsWaves envs per workgroup.  Lanes 0..23 scan the env's bodies, lane 0 keeps the books.  Every value the kernel
// writes belongs to its env alone: no atomics, the same result on every run.
__global__ void __launch_bounds__(64 * kStatsWaves)
episode_stats_step_kernel(EpisodeStatsArgs a) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x * kStatsWaves + (threadIdx.x >> 6);
    if (env >= a.n_env) return;              // wave-uniform
    float v2 = 0.0f, w2 = 0.0f;
    bool bad = false;
    if (lane < TNB) {
        const float *s = a.rb_state + ((long)env * TNB + lane) * 13;
        float x[13];
        for (int k = 0; k < 13; ++k) x[k] = s[k];
        for (int k = 0; k < 13; ++k) bad |= !(fabsf(x[k]) <= 3.402823466e38f);      // NaN and +-Inf
        v2 = (x[7] * x[7] + x[8] * x[8]) + x[9] * x[9];
        w2 = (x[10] * x[10] + x[11] * x[11]) + x[12] * x[12];
        v2 = v2 == v2 ? v2 : 0.0f;           // a NaN speed counts as a non-finite step, not as a maximum
        w2 = w2 == w2 ? w2 : 0.0f;
    }
    v2 = wave_max(v2);
    w2 = wave_max(w2);
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane != 0) return;

    float *run = a.running + (long)env * EMLOCO_EPISODE_RUNNING;
    double *tot = a.totals + (long)env * EMLOCO_EPISODE_MOMENTS;
    float r = a.rew_buf[env];
    if (a.inverted && a.inverted[env]) r *= a.neg_scale;         // amp_continuous_value.py:63-64
    const float ret = run[0] + r;
    const float loc = run[1] + a.reward_raw[(long)env * 2];
    const float pw = run[2] + a.reward_raw[(long)env * 2 + 1];
    const float len = run[3] + 1.0f;
    if ((double)v2 > tot[EMLOCO_EPM_MAX_SPEED2]) tot[EMLOCO_EPM_MAX_SPEED2] = (double)v2;
    if ((double)w2 > tot[EMLOCO_EPM_MAX_ANG_SPEED2]) tot[EMLOCO_EPM_MAX_ANG_SPEED2] = (double)w2;
    if (any_bad) tot[EMLOCO_EPM_NONFINITE_STEPS] += 1.0;
    const bool done = a.reset_buf[env] != 0;
    int cause = EMLOCO_EPISODE_RUNS;
    float tar[3] = {0.0f, 0.0f, 0.0f}, d2 = 0.0f;
    if (done || a.game_out) {
        // the post-physics kernel's target (task_device.h: post_physics_env, sample 0) and its distance test, term by term
        calc_pos(a.traj_verts + (long)env * EMLOCO_TRAJ_VERTS * 3, (float)a.progress_buf[env] * a.dt, a.traj_dur, tar);
        const float *root = a.rb_state + (long)env * TNB * 13;
        const float dx = tar[0] - root[0], dy = tar[1] - root[1];
        d2 = dx * dx + dy * dy;
    }
    if (done) {
        const bool far = d2 > a.fail_dist * a.fail_dist;
        cause = far ? EMLOCO_EPISODE_FAR : (a.terminate_buf[env] != 0 ? EMLOCO_EPISODE_FALLEN : EMLOCO_EPISODE_TIMEOUT);
        const double games = tot[EMLOCO_EPM_GAMES];
        const double dl = (double)len, dr = (double)ret;
        tot[EMLOCO_EPM_GAMES] = games + 1.0;
        tot[EMLOCO_EPM_GAMES + cause] += 1.0;                     // TIMEOUT / FAR / FALLEN follow GAMES
        tot[EMLOCO_EPM_SUM_LEN] += dl;
        tot[EMLOCO_EPM_SUM_LEN2] += dl * dl;
        const double mn = tot[EMLOCO_EPM_MIN_LEN], mx = tot[EMLOCO_EPM_MAX_LEN];
        tot[EMLOCO_EPM_MIN_LEN] = (games == 0.0 || dl < mn) ? dl : mn;          // (cleared totals hold 0, not a length)
        tot[EMLOCO_EPM_MAX_LEN] = dl > mx ? dl : mx;
        tot[EMLOCO_EPM_SUM_RET] += dr;
        tot[EMLOCO_EPM_SUM_RET2] += dr * dr;
        tot[EMLOCO_EPM_SUM_LOC] += (double)loc;
        tot[EMLOCO_EPM_SUM_POW] += (double)pw;
    }
    if (a.game_out) {
        float *g = a.game_out + (long)env * EMLOCO_EPISODE_GAME_OUT;
        g[0] = done ? ret : 0.0f; g[1] = done ? loc : 0.0f; g[2] = done ? pw : 0.0f; g[3] = done ? len : 0.0f;
        g[4] = (float)cause; g[5] = tar[0]; g[6] = tar[1]; g[7] = d2;
    }
    // the running values start over with the game
    run[0] = done ? 0.0f : ret;
    run[1] = done ? 0.0f : loc;
    run[2] = done ? 0.0f : pw;
    run[3] = done ? 0.0f : len;
}

constexpr int kStatsReduceThreads = 256;

__device__ __forceinline__ bool epm_is_min(int k) { return k == EMLOCO_EPM_MIN_LEN; }
__device__ __forceinline__ bool epm_is_max(int k) { return k == EMLOCO_EPM_MAX_LEN || k == EMLOCO_EPM_MAX_SPEED2 || k == EMLOCO_EPM_MAX_ANG_SPEED2; }
__device__ __forceinline__ double epm_fold(int k, double x, double y) {
    if (epm_is_min(k)) return y < x ? y : x;
    if (epm_is_max(k)) return y > x ? y : x;
    return x + y;
}

// One workgroup: thread t folds the contiguous envs [t c, (t + 1) c) in ascending order, then a pairwise tree in LDS in a fixed order
// -- the same moments on every run -- and clears the totals it has read.  The minimum length only looks at envs that finished a game
// (+inf stands for "none" inside the tree; a vector without games carries 0).
__global__ void __launch_bounds__(kStatsReduceThreads)
episode_stats_reduce_kernel(int n_env, double *totals, double *moments) {
    __shared__ double sm[EMLOCO_EPISODE_MOMENTS][kStatsReduceThreads];
    const int tid = threadIdx.x;
    const int c = (n_env + kStatsReduceThreads - 1) / kStatsReduceThreads;
    const long lo = (long)tid * c, hi = (lo + c < n_env) ? lo + c : n_env;
    double m[EMLOCO_EPISODE_MOMENTS];
    for (int k = 0; k < EMLOCO_EPISODE_MOMENTS; ++k) m[k] = 0.0;
    m[EMLOCO_EPM_MIN_LEN] = __builtin_inf();
    for (long e = lo; e < hi; ++e) {
        double *tot = totals + e * EMLOCO_EPISODE_MOMENTS;
        const bool played = tot[EMLOCO_EPM_GAMES] > 0.0;
        for (int k = 0; k < EMLOCO_EPISODE_MOMENTS; ++k) {
            const double x = tot[k];
            if (!epm_is_min(k) || played) m[k] = epm_fold(k, m[k], x);
            tot[k] = 0.0;
        }
    }
    for (int k = 0; k < EMLOCO_EPISODE_MOMENTS; ++k) sm[k][tid] = m[k];
    __syncthreads();
    for (int off = kStatsReduceThreads / 2; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < EMLOCO_EPISODE_MOMENTS; ++k) sm[k][tid] = epm_fold(k, sm[k][tid], sm[k][tid + off]);
        __syncthreads();
    }
    if (tid < EMLOCO_EPISODE_MOMENTS) {
        double v = sm[tid][0];
        if (epm_is_min(tid) && !(sm[EMLOCO_EPM_GAMES][0] > 0.0)) v = 0.0;
        moments[tid] = v;
    }
}

}  // namespace emloco

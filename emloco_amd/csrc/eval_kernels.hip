// eval_kernels.hip -- the LocoVal evaluation (`run.py --test`): the per-game bookkeeping of AMPPlayerContinuousValue.run
// (pacer/pacer/learning/amp_value_players.py:35-272, the plot_val_reward branch of the shipped player config) for a batch of envs.
// Entry points and record layout: include/emloco_predictor.h (EmlocoLocoValEval).  Built without multiply-add contraction
// (build.py, like the task unit): every accumulation follows the reference's torch / Python expression operation by operation, in the
// reference's dtypes (fp32 tensors, Python floats = double), so a game's record is the reference's numbers bit for bit
// (tests/golden/locoval_player.npz).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/emloco_predictor.h"
#include "locoval_returns_device.h"
#include "task_device.h"          // calc_pos: the target of the reward, for the path tracking

namespace emloco {

constexpr float kEvalMinReward = -10.0f, kEvalMaxReward = 100.0f;     // amp_value_players.py:55-56 (Python ints)
constexpr int kEvalReduceThreads = 256;

// One wave per env.  Lane 0 advances the env's game (the accumulation is a handful of scalar operations); at the game's first step
// the whole wave copies the LocoVal inputs in origin-relative form through the helper the training rollout uses
// (locoval_stage_env, locoval_returns_device.h: vec_task_wrappers.py:50-66, first 13 waypoints).
__global__ void __launch_bounds__(256)
locoval_eval_step_kernel(EmlocoLocoValEval s, const float *reward_raw, const float *disc, const int64_t *dones, const int64_t *terminate,
                         const uint8_t *inverted) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= s.n_env) return;
    // step index inside the game (0 at the first step after the game's reset); every lane reads it before lane 0 advances it below
    // (the exchange orders the reads ahead of that write for the CPU emulation of the kernel as well)
    const int n = __shfl(s.steps[e], 0);
    if (n == 0) {                               // :128-134 on the state after this step: the inputs the task captured at the reset
        EmlocoLocoValStep io = {};
        io.n_env = s.n_env;
        io.waypoint_traj = s.waypoint_traj; io.init_pose = s.init_pose; io.init_vel = s.init_vel;
        io.traj13 = s.traj13; io.pose = s.pose; io.vel = s.vel;
        locoval_stage_env(io, e, lane);
    }
    if (lane != 0) return;
    s.row_mask[e] = n == 0 ? 1.0f : 0.0f;
    // :144 -- the coefficient advances BEFORE the accumulation: the first reward already carries gamma.  A Python float (double).
    const double coef = s.coef[e] * s.gamma;
    const float coef32 = (float)coef;           // torch casts the Python scalar to the fp32 tensor's type
    const float r_loc = reward_raw[2 * (long)e], r_pow = reward_raw[2 * (long)e + 1];     // :138-139 (fp32)
    // :143-149 -- the style reward arrives as `.item()` of an fp32 tensor: promoted to double, and accumulated in double
    const double d = disc ? (double)disc[e] : 0.0;
    const float c_loc = s.c_loc[e] + (r_loc * 0.5f) * coef32;                            // :150 (fp32)
    const float c_pow = s.c_pow[e] + (r_pow * 0.5f) * coef32;                            // :151 (fp32)
    const double c_disc = s.c_disc[e] + (d * 0.25) * coef;                               // :149 (double)
    // :152 in this expression order; `disc_reward * 0.25` is computed in double and then cast to fp32 by the tensor add.  The
    // inversion penalty of :127 multiplies `r`, which this branch never adds to cr: the evaluation target ignores the inversion
    // (the training target of play_steps does not).
    const float cr = s.cr[e] + ((r_loc + r_pow) * 0.5f + (float)(d * 0.25)) * coef32;
    s.coef[e] = coef;
    s.c_loc[e] = c_loc;
    s.c_pow[e] = c_pow;
    s.c_disc[e] = c_disc;
    s.cr[e] = cr;
    s.steps[e] = n + 1;
    if (n == s.step_to_pred) {                  // :177-184
        s.tp_cr[e] = cr;
        s.tp_loc[e] = c_loc;
        s.tp_pow[e] = c_pow;
        s.tp_disc[e] = c_disc;
    }
    s.done[e] = dones[e] != 0 ? 1 : 0;
    s.terminated[e] = (terminate && terminate[e] != 0) ? 1 : 0;
    s.inverted[e] = (inverted && inverted[e]) ? 1 : 0;
}

// One env after the forward has evaluated the rows of this step's first steps: a game that ended this step is recorded at
// records[k][e][games[e]] for each of the n_nets networks (value_of(k): network k's value plane; the planes differ in `value` and `sq_err`
// alone) while the env's quota is not met (each env owns its slots: no append, no atomics on the records, the same records whatever the
// schedule), then the per-game state starts over -- once, however many networks.  A game that ends at its first step records the
// prediction made at that very step.
template <class VALUES>
__device__ __forceinline__ void locoval_eval_finish_env(const EmlocoLocoValEval &s, int e, int n_nets, VALUES value_of, EmlocoLocoValRecord *records) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    if (!s.done[e]) return;
    const int g = s.games[e];
    if (g < s.games_per_env) {
        const int steps = s.steps[e];
        // :187-193 -- a game that ends before step_to_pred takes its values at the end; otherwise the capture of :177-184 stands
        const bool at_end = steps - 1 < s.step_to_pred;
        const float cr = s.cr[e];
        const float tp_cr = at_end ? cr : s.tp_cr[e];
        EmlocoLocoValRecord r;
        r.disc_to_pred = at_end ? s.c_disc[e] : s.tp_disc[e];
        r.cr_to_pred = tp_cr;                   // :208 -- `rewards` holds the UNnormalised return
        r.loc_to_pred = at_end ? s.c_loc[e] : s.tp_loc[e];
        r.pow_to_pred = at_end ? s.c_pow[e] : s.tp_pow[e];
        // :195, fp32, a true division (the reference on the CPU; torch on a GPU would multiply by the fp32 reciprocal of 110)
        r.norm = (tp_cr - kEvalMinReward) / (kEvalMaxReward - kEvalMinReward);
        r.cr_end = cr;                          // :203
        r.steps = steps;                        // :204
        r.terminated = s.terminated[e];
        r.inverted = s.inverted[e];
        const long plane = (long)s.n_env * s.games_per_env;
        for (int k = 0; k < n_nets; ++k) {
            r.value = value_of(k)[e];
            const float diff = r.value - r.norm;
            r.sq_err = diff * diff;             // :196, MSELoss of one element
            records[k * plane + (long)e * s.games_per_env + g] = r;
        }
        s.games[e] = g + 1;
        if (g + 1 == s.games_per_env) atomicAdd(s.n_full, 1);     // an integer count: its final value does not depend on the order
    }
    // :199-202 and the next game's :72,87-95: cr, steps, the coefficient and the parts start over
    s.coef[e] = 1.0;
    s.c_disc[e] = 0.0;
    s.cr[e] = 0.0f;
    s.c_loc[e] = 0.0f;
    s.c_pow[e] = 0.0f;
    s.steps[e] = 0;
}

// One thread per env, after emloco_locoval_fwd_rows: the single network's records [n_env][games_per_env]
__global__ void __launch_bounds__(256)
locoval_eval_finish_kernel(EmlocoLocoValEval s, const float *value, EmlocoLocoValRecord *records) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n_env) return;
    locoval_eval_finish_env(s, e, 1, [=](int) { return value; }, records);
}

// One thread per env, after emloco_locoval_eval_fwd_multi: records [n_nets][n_env][games_per_env]
__global__ void __launch_bounds__(256)
locoval_eval_finish_multi_kernel(EmlocoLocoValEval s, EmlocoLocoValNets t, EmlocoLocoValRecord *records) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n_env) return;
    locoval_eval_finish_env(s, e, t.n_nets, [&](int k) { return (const float *)t.net[k].value; }, records);
}

// One workgroup: thread t sums the contiguous slots [t c, (t + 1) c) of records (env-major, game-minor; only the recorded games), then a
// pairwise tree in LDS in a fixed order -- the same moments on every run.
__global__ void __launch_bounds__(kEvalReduceThreads)
locoval_eval_reduce_kernel(int n_env, int games_per_env, const EmlocoLocoValRecord *records, const int32_t *games, double *moments) {
    __shared__ double sm[EMLOCO_EVAL_MOMENTS][kEvalReduceThreads];
    const int tid = threadIdx.x;
    const long total = (long)n_env * games_per_env;
    const long c = (total + kEvalReduceThreads - 1) / kEvalReduceThreads;
    const long lo = tid * c, hi = (lo + c < total) ? lo + c : total;
    double m[EMLOCO_EVAL_MOMENTS];
    for (int k = 0; k < EMLOCO_EVAL_MOMENTS; ++k) m[k] = 0.0;
    for (long i = lo; i < hi; ++i) {
        const long e = i / games_per_env;
        const int g = (int)(i - e * games_per_env);
        if (g >= games[e]) continue;
        const EmlocoLocoValRecord r = records[i];
        const double v = r.value;
        const double y[4] = {(double)r.cr_to_pred, (double)r.loc_to_pred, (double)r.pow_to_pred, r.disc_to_pred};
        m[0] += 1.0;
        m[1] += v;
        m[2] += v * v;
        for (int k = 0; k < 4; ++k) {
            m[3 + 3 * k] += y[k];
            m[4 + 3 * k] += y[k] * y[k];
            m[5 + 3 * k] += v * y[k];
        }
        m[15] += r.sq_err;
        m[16] += r.cr_end;
        m[17] += r.steps;
        m[18] += r.terminated ? 1.0 : 0.0;
        m[19] += r.inverted ? 1.0 : 0.0;
    }
    for (int k = 0; k < EMLOCO_EVAL_MOMENTS; ++k) sm[k][tid] = m[k];
    __syncthreads();
    for (int off = kEvalReduceThreads / 2; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < EMLOCO_EVAL_MOMENTS; ++k) sm[k][tid] += sm[k][tid + off];
        __syncthreads();
    }
    if (tid < EMLOCO_EVAL_MOMENTS) moments[tid] = sm[tid][0];
}

// ---------------------------------------------------------------------------------------------------------------- path tracking
// (`--eval_tracks`; include/emloco_predictor.h: EmlocoLocoValTrack).  One thread per env, between locoval_eval_step_kernel and the finish
// kernels: s.done[e] is this step's flag, s.steps[e] the game's step count including this step, s.games[e] the slot of the game in
// progress.  One calc_pos, two vertex reads and a dozen flops per env; the sums are doubles added in step order, nothing is atomic.
__global__ void __launch_bounds__(256)
locoval_eval_track_kernel(EmlocoLocoValEval s, EmlocoLocoValTrack t, EmlocoLocoValTrackRecord *records, float *samples) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n_env) return;
    const float *verts = t.traj_verts + (long)e * EMLOCO_TRAJ_VERTS * 3;
    const int64_t prog = t.progress_buf[e];
    float tar[3];
    calc_pos(verts, (float)prog * t.dt, t.traj_dur, tar);        // task_device.h:181-183, sample 0: the reward's target
    const float *root = t.root_pos + (long)e * t.root_stride;
    const float rx = root[0], ry = root[1];
    const float dx = tar[0] - rx, dy = tar[1] - ry;               // task_device.h:279-280
    const float dev = sqrtf(dx * dx + dy * dy);
    if (t.dev_now) t.dev_now[e] = dev;
    const int g = s.games[e];
    if (g >= s.games_per_env) return;                             // the quota is met: the env keeps stepping and records nothing
    const int n = s.steps[e];                                     // >= 1: this step is the game's n-th
    const bool first = n <= 1;
    double sum_dev = first ? 0.0 : t.sum_dev[e];
    double sum_sample = first ? 0.0 : t.sum_sample_dev[e];
    double path_len = first ? 0.0 : t.path_len[e];
    float max_dev = first ? 0.0f : t.max_dev[e];
    float last_sample = first ? 0.0f : t.last_sample_dev[e];
    int n_samples = first ? 0 : t.n_samples[e];
    sum_dev += (double)dev;
    max_dev = dev > max_dev ? dev : max_dev;
    if (!first) {                                                 // prev_xy is the root of this game's step before
        const float sx = rx - t.prev_xy[2 * (long)e], sy = ry - t.prev_xy[2 * (long)e + 1];
        path_len += (double)sqrtf(sx * sx + sy * sy);
    }
    const long slot = (long)e * s.games_per_env + g;
    if (prog % t.stride == 0 && n_samples < EMLOCO_TRACK_SAMPLES) {
        float *o = samples + (slot * EMLOCO_TRACK_SAMPLES + n_samples) * 4;
        o[0] = rx - verts[0];
        o[1] = ry - verts[1];
        o[2] = tar[0] - verts[0];
        o[3] = tar[1] - verts[1];
        sum_sample += (double)dev;
        last_sample = dev;
        n_samples += 1;
    }
    const bool done = s.done[e] != 0;
    if (done) {
        EmlocoLocoValTrackRecord r;
        r.ade = n_samples > 0 ? (float)(sum_sample / (double)n_samples) : 0.0f;
        r.fde = n_samples > 0 ? last_sample : 0.0f;
        r.mean_dev = (float)(sum_dev / (double)(n > 1 ? n : 1));
        r.max_dev = max_dev;
        r.final_dev = dev;
        r.path_len = (float)path_len;
        r.n_samples = n_samples;
        r._pad = 0;
        records[slot] = r;
    }
    // the accumulators start over with the game
    t.sum_dev[e] = done ? 0.0 : sum_dev;
    t.sum_sample_dev[e] = done ? 0.0 : sum_sample;
    t.path_len[e] = done ? 0.0 : path_len;
    t.max_dev[e] = done ? 0.0f : max_dev;
    t.last_sample_dev[e] = done ? 0.0f : last_sample;
    t.n_samples[e] = done ? 0 : n_samples;
    t.prev_xy[2 * (long)e] = rx;
    t.prev_xy[2 * (long)e + 1] = ry;
}

// One workgroup, as locoval_eval_reduce_kernel: thread t sums a contiguous run of slots (the recorded games only), then a pairwise tree in
// LDS in a fixed order.
__global__ void __launch_bounds__(kEvalReduceThreads)
locoval_track_reduce_kernel(int n_env, int games_per_env, const EmlocoLocoValTrackRecord *records, const int32_t *games, float fail_dist,
                            double *moments) {
    __shared__ double sm[EMLOCO_TRACK_MOMENTS][kEvalReduceThreads];
    const int tid = threadIdx.x;
    const long total = (long)n_env * games_per_env;
    const long c = (total + kEvalReduceThreads - 1) / kEvalReduceThreads;
    const long lo = tid * c, hi = (lo + c < total) ? lo + c : total;
    double m[EMLOCO_TRACK_MOMENTS];
    for (int k = 0; k < EMLOCO_TRACK_MOMENTS; ++k) m[k] = 0.0;
    for (long i = lo; i < hi; ++i) {
        const long e = i / games_per_env;
        const int g = (int)(i - e * games_per_env);
        if (g >= games[e]) continue;
        const EmlocoLocoValTrackRecord r = records[i];
        const double ade = r.ade, fde = r.fde, md = r.mean_dev;
        m[0] += 1.0;
        if (r.n_samples > 0) {
            m[1] += 1.0;
            m[2] += ade;
            m[3] += ade * ade;
            m[4] += fde;
            m[5] += fde * fde;
        }
        m[6] += md;
        m[7] += md * md;
        m[8] += r.final_dev;
        m[9] += r.path_len;
        m[10] += r.n_samples;
        m[11] += r.max_dev > fail_dist ? 1.0 : 0.0;
    }
    for (int k = 0; k < EMLOCO_TRACK_MOMENTS; ++k) sm[k][tid] = m[k];
    __syncthreads();
    for (int off = kEvalReduceThreads / 2; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < EMLOCO_TRACK_MOMENTS; ++k) sm[k][tid] += sm[k][tid + off];
        __syncthreads();
    }
    if (tid < EMLOCO_TRACK_MOMENTS) moments[tid] = sm[tid][0];
}

}  // namespace emloco

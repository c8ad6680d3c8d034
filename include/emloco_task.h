/*
 * emloco_task.h -- C ABI of libemloco_hip.so, part 2: the fused post-physics task kernels.
 *
 * One launch replaces the ~100 small torch kernels of the reference's post_physics_step
 * (pacer/pacer/env/tasks/humanoid.py:1211-1232, humanoid_amp.py:139-157):
 *   progress += 1                        humanoid.py:1213
 *   self observations (368)              humanoid.py:1625-1687 (compute_humanoid_observations_smpl_max)
 *   mirrored observations                humanoid.py:1066-1108, humanoid_pedestrain_terrain.py:455-491
 *   trajectory samples + location obs    humanoid_traj.py:208-224, traj_generator.py:278-296,
 *                                        humanoid_pedestrain_terrain.py:1549-1577
 *   height-map observations (32x32)      humanoid_pedestrain_terrain.py:394-442,732-815,1212-1288
 *   reward                               humanoid_pedestrain_terrain.py:907-930,1581-1592
 *   reset / terminate masks (int64)      humanoid_pedestrain_terrain.py:883-905,1468-1530
 *   AMP history shift + new AMP row      humanoid_amp.py:585-657,917-971
 * Buffers are caller-owned device memory (the task object allocates them, base_task.py:96-111).
 * Every entry point returns 0 or a negative EMLOCO_E_* code (emloco_sim.h); emloco_last_error() then has the text, for every entry
 * point of this header: per thread, meaningful only directly after the failing call; nothing is printed.
 */
#ifndef EMLOCO_TASK_H
#define EMLOCO_TASK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMLOCO_SELF_OBS 368
#define EMLOCO_TRAJ_SAMPLES 15
#define EMLOCO_TRAJ_VERTS 101
#define EMLOCO_HEIGHT_POINTS 1024
#define EMLOCO_TASK_OBS (2 * EMLOCO_TRAJ_SAMPLES + EMLOCO_HEIGHT_POINTS)
#define EMLOCO_OBS (EMLOCO_SELF_OBS + EMLOCO_TASK_OBS)
#define EMLOCO_AMP_ROW 206
#define EMLOCO_AMP_STEPS 15

/* what one launch computes (bit-or) */
enum {
    EMLOCO_POST_ADVANCE = 1,    /* progress_buf += 1 */
    EMLOCO_POST_OBS = 2,        /* obs_buf and flip_obs_buf */
    EMLOCO_POST_REWARD = 4,     /* rew_buf, reward_raw */
    EMLOCO_POST_RESET = 8,      /* reset_buf, terminate_buf */
    EMLOCO_POST_AMP_SHIFT = 16, /* history shift of amp_obs_buf */
    EMLOCO_POST_AMP_ROW = 32,   /* newest AMP row */
    EMLOCO_POST_STEP = 63,      /* everything post_physics_step does */
    EMLOCO_POST_SKIP_DONE = 64, /* leave the envs whose reset_buf is set alone (their observation rows are rebuilt by the reset
                                 * path): lets the observation launch of a step run beside that step's resets on another stream */
    EMLOCO_POST_AMP_DONE_ONLY = 128 /* AMP_SHIFT / AMP_ROW act on the envs whose reset flag is set after this launch only: the
                                 * terminal AMP observations of the finished envs (amp_continuous_value.py:90-96 scores them) are
                                 * written by the flags launch, BEFORE the reset path overwrites those envs' state; the side
                                 * launch (SKIP_DONE) writes the live envs' rows */
};

typedef struct {
    int32_t n_env;
    int32_t hf_rows, hf_cols;       /* height map shape (first index = x) */
    int32_t head_body;              /* sensor frame body (terrain_obs_root "head" -> 13) */
    int32_t n_dof_subset;           /* 57; a multiple of 3, at most 57 (an AMP row is 35 + 3 n_dof_subset values, EMLOCO_AMP_ROW at most) */
    float dt;                       /* control dt = controlFrequencyInv * sim.dt */
    float traj_dur;                 /* num_verts * vertex dt (traj_generator.py:270-273) */
    float sample_dt;                /* trajSampleTimestep */
    float hscale, vscale;           /* 0.1, 0.005 */
    float power_coef;               /* power_coefficient */
    float fail_dist;                /* 4.0 (humanoid_traj.py:30) */
    float max_episode_length;       /* episodeLength */
    /* simulator tensors (device) */
    const float *rb_state;          /* [E][24][13] */
    const float *dof_state;         /* [E][69][2] */
    const float *dof_force;         /* [E][69] */
    const float *contact_force;     /* [E][24][3] */
    /* task data (device) */
    const float *betas;             /* [E][17] humanoid_betas */
    const float *traj_verts;        /* [E][101][3] */
    const int16_t *heightfield;     /* [hf_rows][hf_cols] */
    const int32_t *left_to_right;   /* [24] */
    const uint8_t *contact_body_mask; /* [24] 1 = foot body excluded from the fall test */
    const int32_t *key_bodies;      /* [4] */
    const int32_t *dof_subset;      /* [n_dof_subset] */
    /* task buffers (device, in/out) */
    int64_t *progress_buf;          /* [E] */
    int64_t *reset_buf;             /* [E] */
    int64_t *terminate_buf;         /* [E] */
    float *obs_buf;                 /* [E][1422] */
    float *flip_obs_buf;            /* [E][1422] */
    float *rew_buf;                 /* [E] */
    float *reward_raw;              /* [E][2] */
    float *amp_obs_buf;             /* [E][15][206], index 0 = newest */
    /* 0: amp_obs_buf is the reference's layout (humanoid_amp.py:585-594): EMLOCO_POST_AMP_SHIFT moves rows 0..13 to 1..14 every step
     * -- 23 KB of the ~38 KB an env-step moves.  1 + h: amp_obs_buf is a RING: the row the reference calls k lives in physical row
     * (h + k) % 15, EMLOCO_POST_AMP_SHIFT is a no-op and EMLOCO_POST_AMP_ROW writes physical row h.  The caller moves h back by one
     * (h <- (h + 14) % 15) once per step, ahead of that step's launches, and hands the same value to EmlocoResetBufs.amp_ring. */
    int32_t amp_ring;
} EmlocoTaskBufs;
#define EMLOCO_AMP_PHYS_ROW(amp_ring, k) ((amp_ring) ? ((amp_ring) - 1 + (k)) % EMLOCO_AMP_STEPS : (k))

/* post_physics_step for all envs (dev_env_ids == NULL) or for the listed envs
 * (_compute_observations(env_ids) on reset, humanoid.py:459-465). */
int emloco_task_post_physics(const EmlocoTaskBufs *bufs, int mode, const int32_t *dev_env_ids, int n, void *stream);

/* emloco_task_post_physics for all envs with the LocoVal return bookkeeping of amp_continuous_value.py:63-64,93-129 behind it in the
 * SAME launch: what emloco_locoval_returns (include/emloco_predictor.h) does with rewards = rew_buf, dones = reset_buf and no AMP
 * reward, for each env right after its reward and reset flag exist.  `mode` must hold EMLOCO_POST_REWARD | EMLOCO_POST_RESET.
 * `step` is an EmlocoLocoValStep (emloco_predictor.h), dev_inverted the heading-inversion flags [n_env] (bytes) or NULL.  A step
 * with staging arrays (staged_reward / staged_done) is only STAGED here; emloco_locoval_returns_finish completes it once the AMP
 * discriminator's reward of the step exists. */
int emloco_task_post_physics_returns(const EmlocoTaskBufs *bufs, int mode, const void *step /* const EmlocoLocoValStep * */,
                                     const uint8_t *dev_inverted, void *stream);

/* AMP rows from explicit states (history back-fill from the motion library, humanoid_amp.py:486-535):
 * n rows; inputs [n][3|4|3|3|69|69|4*3|17]; out [n][206], of which a row fills its first 35 + 3 n_dof_subset values (n_dof_subset:
 * a multiple of 3, at most 57: refused otherwise). */
int emloco_task_amp_rows(int n, const float *root_pos, const float *root_rot, const float *root_vel,
                         const float *root_ang_vel, const float *dof_pos, const float *dof_vel,
                         const float *key_pos, const float *betas, const int32_t *dof_subset,
                         int n_dof_subset, float *out, void *stream);

/* pre_physics_step: pd_tar = offset + scale * action, zeroed where mask != 0 (humanoid.py:1184-1202,1281-1283) */
int emloco_task_pd_targets(int n_env, const float *actions, const float *offset, const float *scale,
                           const uint8_t *zero_mask, float *pd_targets, void *stream);

/* Same, and a copy of the actions as they were read into `actions_copy` ([n_env][69], optional, ignored when it aliases
 * `actions`): the reference keeps `self.actions = actions.clone()` (humanoid.py:1185); one launch instead of a copy and a launch. */
int emloco_task_pd_targets_copy(int n_env, const float *actions, const float *offset, const float *scale,
                                const uint8_t *zero_mask, float *pd_targets, float *actions_copy, void *stream);

/* wall-clock of the last emloco_task_post_physics launch measured with HIP events [ms]; <0 if none */
float emloco_task_last_ms(void);
int emloco_task_enable_timing(int on);


/* ------------------------------------------------------------------------------------------------------------
 * Fused reset of finished envs (reference-state init + task reset; per-episode, but with 4096 envs some env
 * resets almost every step).  Replaces the ~1 100 small torch launches of the host-side path:
 *   _sample_ref_state / get_motion_state_smpl      humanoid_pedestrain_terrain.py:526-573, motion_lib_smpl.py:485-606
 *   _reset_ref_state_init, _set_env_state          humanoid_pedestrain_terrain.py:575-631, humanoid_amp.py:537-563
 *   _reset_env_tensors                             humanoid.py:467-481
 *   TrajGenerator.reset                            env/util/traj_generator.py:60-237
 *   _reset_task (LocoVal input capture)            humanoid_pedestrain_terrain.py:493-523
 *   _init_amp_obs_ref (history back-fill)          humanoid_amp.py:486-535
 * Random numbers are supplied by the caller (`rnd`, uniform [0,1), EMLOCO_RESET_RND floats per env) so a test can
 * drive the kernels and the host mirror with the same draws. */
#define EMLOCO_RESET_RND 512
enum {
    EMLOCO_RESET_RANDOM_HEADING = 1, EMLOCO_RESET_INIT_HEADING = 2, EMLOCO_RESET_HEADING_INVERSION = 4,
    EMLOCO_RESET_ADJUST_ROOT_VEL = 8, EMLOCO_RESET_REAL_PATH = 16, EMLOCO_RESET_FIXED_LOCATION = 32,
    EMLOCO_RESET_NO_AMP_HISTORY = 64      /* emloco_task_reset leaves the AMP history back-fill to emloco_task_reset_amp_history */
};
/* layout of one env's random row */
enum {
    EMLOCO_RND_MOTION = 0, EMLOCO_RND_TIME = 1, EMLOCO_RND_YAW = 2, EMLOCO_RND_SPEED = 3, EMLOCO_RND_LOC = 4,
    EMLOCO_RND_REAL = 5, EMLOCO_RND_REAL_PICK = 6, EMLOCO_RND_INVERSION = 7, EMLOCO_RND_HEADING = 8, EMLOCO_RND_SPEED0 = 9,
    EMLOCO_RND_DTHETA = 16, EMLOCO_RND_SHARP = 116, EMLOCO_RND_BERN = 216, EMLOCO_RND_DSPEED = 316
};

typedef struct {
    int32_t flags;
    int32_t n_motions, n_real, n_valid, n_dof_subset;
    int32_t hf_rows, hf_cols;
    float fixed_x, fixed_y;
    float dt;                       /* control dt */
    float height_tolerance;         /* lowest collision point above ground after reset (0.02) */
    float vert_dt, dtheta_max, speed_min, speed_max, accel_max, sharp_prob, hybrid_prob;   /* TrajGenerator */
    float traj_dur, sample_dt, hscale, vscale;
    /* motion cache (motion_lib_smpl.py:334-341) */
    const float *gts, *grs, *lrs, *gvs, *gavs, *dvs;
    const float *motion_len, *motion_dt;
    const int64_t *motion_nframes, *motion_start;
    const float *real_traj;         /* [n_real][101][3] or NULL */
    const int16_t *heightfield;
    const float *valid_x, *valid_y; /* walkable sample locations [n_valid] */
    const float *betas;             /* [E][17] */
    const int32_t *key_bodies, *dof_subset;
    /* task buffers written */
    float *traj_verts;              /* [E][101][3] */
    uint8_t *inverted;              /* [E] (bool) */
    int64_t *progress_buf, *reset_buf, *terminate_buf;
    float *waypoint_traj;           /* [E][15][3] */
    float *init_pose;               /* [E][24][3] */
    float *init_vel;                /* [E][2] */
    float *amp_obs_buf;             /* [E][15][206]: rows 1..14 back-filled here, row 0 by emloco_task_post_physics */
    int64_t *motion_ids;            /* [E] */
    float *motion_times;            /* [E] */
    float *ground_h;                /* [E] scratch: ground height under the reset pose */
    /* real paths (traj_generator.py:121-160): list entry i takes row P_key(i mod n_real) of real_traj, P_key a keyed
     * bijection of [0, n_real) -- distinct rows within one call, like the reference's random.sample(range(n), k);
     * real_pick (device, [n] rows, optional) replaces the permutation by explicit rows */
    const int32_t *real_pick;
    uint32_t real_pick_key;
    int32_t amp_ring;               /* as EmlocoTaskBufs.amp_ring: where the back-filled history rows 1..14 go */
} EmlocoResetBufs;

struct EmlocoSim;
/* resets the listed envs of `sim` (device env ids, n entries, rnd [n][EMLOCO_RESET_RND]) */
int emloco_task_reset(struct EmlocoSim *sim, const EmlocoResetBufs *bufs, const int32_t *dev_env_ids, int n,
                      const float *dev_rnd, void *stream);

/* Same, with the random rows produced on the device: row i of `dev_rnd_ws` ([n][EMLOCO_RESET_RND] floats, caller-owned
 * workspace) is filled with uniforms in [0, 1) from a stateless hash of (seed, i, k) for the list entries that are present,
 * then emloco_task_reset runs on it.  Pass a fresh seed per call (e.g. base seed + call counter; the reference draws from
 * torch's global generator: humanoid_amp.py:284-379, traj_generator.py:60-237).  With a compacted done-list this avoids
 * generating n_env rows per step when a few dozen envs finish.
 * Whatever emloco_task_reset refuses (a NULL simulator, buffer struct, list or workspace, n < 0 or above the simulator's env count,
 * a missing buffer) is refused here with the same code before anything is written, the workspace included -- also at n == 0, where
 * a NULL simulator or buffer struct is an error as it is for emloco_task_reset. */
int emloco_task_reset_seeded(struct EmlocoSim *sim, const EmlocoResetBufs *bufs, const int32_t *dev_env_ids, int n,
                             uint64_t seed, float *dev_rnd_ws, void *stream);

/* The AMP history back-fill of a reset (_init_amp_obs_ref, humanoid_amp.py:486-535) alone: rows 1..14 of the listed envs'
 * AMP observations from the motion ids / start times the reset sampled.  It reads nothing the simulator writes, so a caller
 * that passed EMLOCO_RESET_NO_AMP_HISTORY may run it on another stream beside the rest of the reset chain. */
int emloco_task_reset_amp_history(const EmlocoResetBufs *bufs, const int32_t *dev_env_ids, int n, void *stream);

/* TrajGenerator.reset(env_ids, init_pos, root_vel) alone (traj_generator.py:60-237): writes traj_verts / inverted of the
 * listed envs from the random rows; dev_init_pos, dev_root_vel [n][3] (one row per list entry).  Only the trajectory
 * fields of `bufs` are read (flags, vert_dt ... hybrid_prob, n_real, real_traj, real_pick*, traj_verts, inverted). */
int emloco_task_traj_reset(const EmlocoResetBufs *bufs, const int32_t *dev_env_ids, int n, const float *dev_rnd,
                           const float *dev_init_pos, const float *dev_root_vel, void *stream);

/* HumanoidPedestrianTerrain.get_heights / get_center_heights for arbitrary poses (humanoid_pedestrain_terrain.py:761-815,
 * 732-759; Terrain.world_points_to_map / sample_height_points :1212-1218,1282-1288): dev_pose7 [n][7] = position + xyzw
 * rotation; grid = 1: the 32x32 sensor grid rotated by the pose's heading -> [n][1024]; grid = 0: the 3x3 yaw-only centre
 * probes -> [n][9].  dev_heights (metres) and the int64 map indices dev_px / dev_py are each optional.  The fused
 * post-physics kernel evaluates the same device functions. */
int emloco_task_get_heights(const int16_t *dev_heightfield, int rows, int cols, float hscale, float vscale, const float *dev_pose7,
                            int n, int grid, float *dev_heights, int64_t *dev_px, int64_t *dev_py, void *stream);

/* Device-side `reset_buf.nonzero()`: dev_ids[0..count) = ascending indices of the non-zero flags, the rest of the n
 * entries = -1, dev_ids[n] = count.  Every *_indexed / env-id-list entry point of this library takes such a list -- negative ids
 * only BEHIND the last valid one -- and skips its padding (the list kernels walk a list of more than 256 entries with a stride of 256
 * and stop at the first negative id they meet, so an entry behind a negative id in the middle of a list may be dropped: its env is
 * then left exactly as it was).  emloco_task_post_physics and emloco_sim_step_subset skip negative ids anywhere in their list.  So
 *   emloco_task_compact_done(reset_buf, E, ids, s); emloco_task_reset(sim, bufs, ids, E, rnd, s);
 *   emloco_task_post_physics(bufs, EMLOCO_POST_OBS | EMLOCO_POST_AMP_ROW, ids, E, s);
 * resets exactly the finished envs without the host ever reading the count (the reference's loop,
 * amp_continuous_value.py:46,74, synchronises on `dones.nonzero()` every step). */
int emloco_task_compact_done(const int64_t *dev_flags, int n, int32_t *dev_ids, void *stream);
/* Same, and a copy of the flags as they were (`dev_snapshot`, n entries): the reset kernels clear the flags of the envs they
 * reset, a launch that runs beside them (emloco_sim_step_subset) follows the snapshot. */
int emloco_task_compact_done_snapshot(const int64_t *dev_flags, int n, int32_t *dev_ids, int64_t *dev_snapshot, void *stream);


/* ------------------------------------------------------------------------------------------------------------
 * The chain between two rigid-body steps in three launches ("around the kernel").  In the reference's
 * loop (amp_continuous_value.py:45-75: env_reset(done_indices) -> obs -> policy -> env.step) everything between two
 * gym.simulate calls is one dependent chain; as separate launches it was 11 kernels and two stream hand-overs.
 *
 * emloco_task_compact_done_order: emloco_task_compact_done_snapshot and -- when `sim` has the cost-ordered dispatch on
 * (emloco_sim_set_cost_order) -- the sort of the NEXT rigid-body launch's dispatch order, as two workgroups of one launch;
 * the next emloco_sim_step / emloco_sim_step_subset then uses that order instead of sorting again.  `sim` may be NULL. */
int emloco_task_compact_done_order(struct EmlocoSim *sim, const int64_t *dev_flags, int n, int32_t *dev_ids,
                                   int64_t *dev_snapshot, void *stream);

/* emloco_task_reset_obs: ONE launch for
 *   (a) the reset of the listed envs: emloco_task_reset[_seeded] (random rows, sample, kinematics, height fix, trajectory,
 *       LocoVal inputs, AMP history unless EMLOCO_RESET_NO_AMP_HISTORY) followed by
 *       emloco_task_post_physics(EMLOCO_POST_OBS | EMLOCO_POST_AMP_ROW) of the same envs (humanoid.py:459-465), and
 *   (b) with live_mode != 0: emloco_task_post_physics(live_mode) of every env whose `dev_skip` entry (the flag snapshot
 *       of emloco_task_compact_done_order) is zero -- the observation / AMP part of post_physics_step (humanoid.py:1214,
 *       humanoid_amp.py:150-155) for the envs that did not finish, which the caller left out of its flags launch.
 * live_mode may hold EMLOCO_POST_OBS, _AMP_SHIFT, _AMP_ROW.  Random rows: `dev_rnd` [n][EMLOCO_RESET_RND] as for
 * emloco_task_reset, or NULL: made on the device from `seed` into `dev_rnd_ws` as for emloco_task_reset_seeded.
 * Results are those of the separate calls, byte for byte (the same device functions run). */
int emloco_task_reset_obs(struct EmlocoSim *sim, const EmlocoResetBufs *reset_bufs, const EmlocoTaskBufs *task_bufs, int live_mode,
                          const int64_t *dev_skip, const int32_t *dev_env_ids, int n, uint64_t seed, float *dev_rnd_ws,
                          const float *dev_rnd, void *stream);

/* The same launch with a pool of pre-drawn episodes.  What a reset draws (clip, joint and root state on the terrain, trajectory,
 * LocoVal waypoints) depends on (seed, position in the list) only -- not on which env finished -- so the launch also draws the
 * leading entries (as many as finished this step + 25 % + 32, at most k) of the NEXT call (seed `next_seed`) into `next` in
 * workgroups of its own, and the reset chain of an entry whose slot in `cur` carries THIS call's seed copies it instead of
 * computing it: the longest serial path of the launch loses its two longest phases.  Entries beyond the pool and slots tagged
 * with another seed take the direct path; same bytes either way.
 * The caller alternates two buffers: this call's `next` is the following call's `cur`.  Ignored (direct path, nothing drawn)
 * when dev_rnd is given.  With a pool, dev_env_ids must be a list of emloco_task_compact_done* (n + 1 entries: the draw count
 * follows dev_env_ids[n], the number of finished envs).
 * Rules (tests/chain_cases.py holds the library and the kernel to them):
 *   two buffers   `cur` and `next` (and their tag arrays) are different buffers: the launch reads entries of the one while it fills
 *                 the other.  With k > 0, cur == next or cur_tag == next_tag (non-NULL) is refused: -1, nothing is written.  So is
 *                 k < 0, k > 4096 and a pool buffer without its tag array.
 *   zero tag      a tag of 0 means "empty": pool buffers start zeroed and no entry of a zeroed buffer is ever used.  Seed 0 is
 *                 therefore reserved: a call with seed == 0 takes the direct path for every entry (same bytes as without a pool) and
 *                 still draws `next` for next_seed as usual.  Entries drawn for next_seed == 0 are never used.
 *   drawn entries entries [0, min(k, c + c / 4 + 32)) of `next` and their tags are written, c = dev_env_ids[n]; entries and tags behind
 *                 them are left as they were (stale tags of an earlier seed cannot match a fresh seed).
 *   dev_rnd_ws    row i is written only for the present entries that take the direct path; rows of entries served from the pool
 *                 are left as they were.  Nothing in the library reads the workspace after the launch: it is scratch, not an output. */
#define EMLOCO_POOL_FLOATS 512      /* per entry: root 13 | misc | dof 138 | trajectory 303 | waypoints 45 */
typedef struct {
    int32_t k;                      /* entries per pool buffer (0: no pool) */
    const float *cur;               /* [k][EMLOCO_POOL_FLOATS] or NULL */
    const uint64_t *cur_tag;        /* [k] seed each entry of `cur` was drawn for */
    float *next;                    /* filled by this launch, or NULL */
    uint64_t *next_tag;
    uint64_t next_seed;             /* the seed the caller will pass to its next call */
} EmlocoResetPool;
int emloco_task_reset_obs_pooled(struct EmlocoSim *sim, const EmlocoResetBufs *reset_bufs, const EmlocoTaskBufs *task_bufs, int live_mode,
                                 const int64_t *dev_skip, const int32_t *dev_env_ids, int n, uint64_t seed, float *dev_rnd_ws,
                                 const float *dev_rnd, const EmlocoResetPool *pool, void *stream);

/* Diagnostic (tools/exp/chain_prof.py; the product never calls it): the first call allocates 16 wall-clock stamps (100 MHz) that
 * every later emloco_task_reset_obs* launch overwrites -- [0..5] reset entry 0: start, random row, sample, kinematics, finish,
 * observations; [6, 7] last AMP history row of entry 0; [8, 9] / [10, 11] the observation workgroups of env 0 / the last env -- and
 * copies them to host16 (may be NULL).  Synchronises the device. */
int emloco_task_chain_profile(long long *host16);

/* ------------------------------------------------------------------------------------------------------------
 * Waypoint tracks to dense path vertices: scipy.interpolate.CubicSpline(knot_t, way, axis=0, bc_type='natural')(query_t) for every
 * track of a batch, which is how social-transmotion/load_jta_traj.py:93-95 turns 13 waypoints at 0.4 s into the 101 vertices that
 * TrajGenerator follows (second derivative zero at both end knots; a query outside the knots is evaluated with the nearest end piece).
 *   knot_t   [n_knots]   HOST array, shared by the batch, strictly increasing, 4..16 knots
 *   dev_way  [n_traj][n_knots][3]   device
 *   query_t  [n_query]   HOST array, shared, 1..128 entries in any order, inside or outside the knots
 *   dev_out  [n_traj][n_query][3]   device
 *   dev_valid [n_traj] bytes, device, or NULL: 0 for a track with a non-finite waypoint (its output rows are zeros; load_jta_traj.py:87-89
 *            skips such tracks), 1 for every other
 * Knots and queries are read when the call is made and travel with the launch (no copy, no synchronisation).  The solve runs in
 * coordinates shifted by the track's first waypoint (x and y; fp32 at +-100 m world coordinates loses a digit otherwise):
 * EMLOCO_DENSIFY_ORIGIN leaves the output shifted (the form TrajGenerator wants), without it the origin is added back.
 * Bad sizes, non-finite or non-increasing knots: -1 and nothing is launched. */
#define EMLOCO_DENSIFY_ORIGIN 1
#define EMLOCO_DENSIFY_MAX_KNOTS 16
#define EMLOCO_DENSIFY_MAX_QUERY 128
int emloco_traj_densify(const float *knot_t, int n_knots, const float *dev_way, int64_t n_traj, const float *query_t, int n_query,
                        float *dev_out, uint8_t *dev_valid, int flags, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Game statistics of a training run, kept on the device: what rl_games' game_rewards / game_lengths meters and the per-epoch line of
 * CommonAgent.train report, without the host reading anything between epochs.
 *
 * Per env the step kernel keeps EMLOCO_EPISODE_RUNNING float32 running values of the game in progress -- [0] return, [1] its location
 * part, [2] its power part (the two reward_raw columns), [3] length -- added in step order, and EMLOCO_EPISODE_MOMENTS doubles of epoch
 * totals in the order of the enumerators below.  The causes of a finished game (reset_buf != 0):
 *   FAR      the squared xy distance of the root to the path's target at progress * dt exceeds fail_dist^2 -- the target is sampled by
 *            the device function the post-physics kernel samples it with, on the same traj_verts and progress_buf
 *   FALLEN   terminate_buf is set and the game is not FAR
 *   TIMEOUT  everything else
 * MAX_SPEED2 / MAX_ANG_SPEED2 are the maxima over the env's 24 bodies and the epoch's steps of (vx vx + vy vy) + vz vz of the linear /
 * angular velocity (float32 arithmetic; a NaN counts as 0 here and as a non-finite step), NONFINITE_STEPS the steps at which any of the
 * env's 24 x 13 state values was NaN or +-Inf. */
#define EMLOCO_EPISODE_RUNNING 4
#define EMLOCO_EPISODE_MOMENTS 15
#define EMLOCO_EPISODE_GAME_OUT 8
enum {
    EMLOCO_EPM_GAMES = 0, EMLOCO_EPM_TIMEOUT = 1, EMLOCO_EPM_FAR = 2, EMLOCO_EPM_FALLEN = 3,
    EMLOCO_EPM_SUM_LEN = 4, EMLOCO_EPM_SUM_LEN2 = 5, EMLOCO_EPM_MIN_LEN = 6, EMLOCO_EPM_MAX_LEN = 7,
    EMLOCO_EPM_SUM_RET = 8, EMLOCO_EPM_SUM_RET2 = 9, EMLOCO_EPM_SUM_LOC = 10, EMLOCO_EPM_SUM_POW = 11,
    EMLOCO_EPM_NONFINITE_STEPS = 12, EMLOCO_EPM_MAX_SPEED2 = 13, EMLOCO_EPM_MAX_ANG_SPEED2 = 14
};
enum { EMLOCO_EPISODE_RUNS = 0, EMLOCO_EPISODE_TIMEOUT = 1, EMLOCO_EPISODE_FAR = 2, EMLOCO_EPISODE_FALLEN = 3 };

/* One env step of the bookkeeping, for all n_envs envs; to be launched after the step's post-physics pass and before the finished envs
 * are reset.  Stands in for amp_continuous_value.py:63-64 (the inversion penalty: rew_buf * -inversion_scale where dev_inverted is set;
 * dev_inverted may be NULL, as for the policy trainer), :94-101 / amp_continuous.py:153-154 / common_agent.py:399-400 (current_rewards,
 * current_lengths, game_rewards.update, game_lengths.update) and :104-107 (the running values of a finished env start again from zero).
 *   dev_rew_buf [E], dev_reward_raw [E][2], dev_reset_buf / dev_terminate_buf / dev_progress_buf [E] int64, dev_rb_state [E][24][13],
 *   dev_traj_verts [E][101][3]; dt, traj_dur, fail_dist as in EmlocoTaskBufs
 *   dev_running [E][EMLOCO_EPISODE_RUNNING] float, dev_totals [E][EMLOCO_EPISODE_MOMENTS] double: in/out, zeroed by the caller once
 *   dev_game_out [E][EMLOCO_EPISODE_GAME_OUT] float or NULL (tests): [0..3] the running values of the game that finished at this step
 *   (zeros otherwise), [4] its cause (EMLOCO_EPISODE_*), [5, 6] the target's xy, [7] the squared distance
 * A NULL required buffer, n_envs <= 0, or a dt / traj_dur / fail_dist that is not positive and finite: -1, nothing is written. */
int emloco_episode_stats_step(int n_envs, const float *dev_rew_buf, const float *dev_reward_raw, const int64_t *dev_reset_buf,
                              const int64_t *dev_terminate_buf, const int64_t *dev_progress_buf, const float *dev_rb_state,
                              const float *dev_traj_verts, const uint8_t *dev_inverted, float inversion_scale, float dt, float traj_dur,
                              float fail_dist, float *dev_running, double *dev_totals, float *dev_game_out, void *stream);

/* Once per epoch, one workgroup: dev_moments[EMLOCO_EPISODE_MOMENTS] (double) = the per-env totals folded over the envs in a fixed tree
 * order -- sums, MIN_LEN a minimum over the envs that finished a game (0 when none did), MAX_LEN / MAX_SPEED2 / MAX_ANG_SPEED2 maxima
 * -- then dev_totals is cleared; dev_running (the games in progress) is not touched.  What CommonAgent.train reads off the meters once
 * per epoch (common_agent.py:199-201: game_rewards.get_mean, game_lengths.get_mean) comes from this vector; the means here are over the
 * games of the epoch, not over rl_games' window of the last games.  NULL buffers or n_envs <= 0: -1, nothing is written. */
int emloco_episode_stats_reduce(int n_envs, double *dev_totals, double *dev_moments, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Flight recorder: a ring on the device holds the rigid-body step's per-env INPUTS of the last R control steps of every env; an env
 * that trips a trigger has its ring frozen into a capture slot, with the state after the step, without the host being involved.  The
 * recorder only reads the simulation.  A capture replays through the CPU oracle bit for bit (tools/replay_capture.py).
 *
 * Record, EMLOCO_REC_WORDS 32-bit words, one (env, control step), taken ahead of the rigid-body launch:
 *   [0] progress_buf as int32   [1] the step counter t   [2] drive_mode   [3] 0
 *   [4 ..) root_state [13] | dof_state [69][2] | warm start [EMLOCO_MAXCAND * 3] | drive input [69]  (508 floats, copied bit for bit)
 * Ring [n_env][R][EMLOCO_REC_WORDS]; step t of every env lies in ring row t % R.
 * Slot, EMLOCO_REC_SLOT_WORDS(R) words:
 *   [0] env   [1] t of the trigger   [2] cause bits   [3] n_valid = min(t - t0 + 1, R) records
 *   [4 ..) R records, oldest first: the steps t - n_valid + 1 .. t, the records behind them zero
 *   then EMLOCO_REC_POST_WORDS floats, the state after step t: root_state [13] | dof_state [69][2] | warm start [96 * 3] |
 *   rigid-body state [24][13] | contact force [24][3] | dof force [69]
 * Causes (cause_mask selects which are looked at):
 *   NONFINITE   any of the env's 24 x 13 body-state values is NaN or +-Inf (the test of EMLOCO_EPM_NONFINITE_STEPS)
 *   SPEED       for some body (vx vx + vy vy) + vz vz > speed2_limit, float32 in this order, strictly; a NaN is not greater
 *   ANG_SPEED   the same on the angular velocity against ang_speed2_limit
 *   EARLY_FALL  terminate_buf != 0 and progress_buf < early_fall_steps
 *   REQUEST     request[env] != 0 (request may be NULL: never)
 * An env whose last capture is less than R steps back (t - last_capture_step[env] < R) is suppressed: no cause, no count, and a
 * request byte it carries is cleared.  The triggered envs of a step take the free slots in ascending env index; one that finds none
 * adds one to the overflow counter of each of its causes and keeps last_capture_step -- and its request byte, which is cleared only
 * when the request is served or suppressed.  Nothing of this depends on grid sizes, dispatch order or timing: the claim is one
 * workgroup, everything else writes per-env or per-slot words.
 * counters [EMLOCO_REC_COUNTERS] int32: [0] slots in use (the host reads it, copies that many slots and clears it), [1 + k] envs that
 * found no slot, per cause bit k. */
#define EMLOCO_REC_WORDS 512
#define EMLOCO_REC_POST_WORDS 892
#define EMLOCO_REC_SLOT_WORDS(R) (4 + (R) * EMLOCO_REC_WORDS + EMLOCO_REC_POST_WORDS)
#define EMLOCO_REC_COUNTERS 8
enum {
    EMLOCO_REC_NONFINITE = 1, EMLOCO_REC_SPEED = 2, EMLOCO_REC_ANG_SPEED = 4, EMLOCO_REC_EARLY_FALL = 8, EMLOCO_REC_REQUEST = 16
};
typedef struct EmlocoRecorderBufs {
    int32_t n_env, depth, n_slots;  /* E, R (>= 1), C (>= 1) */
    int32_t drive_mode;             /* the simulator's live drive mode (EmlocoSimParams), written into every record */
    int32_t t0;                     /* t of the first emloco_recorder_record call */
    int32_t cause_mask;             /* EMLOCO_REC_* bits */
    int32_t early_fall_steps;
    int32_t grid;                   /* workgroups of the grid-stride launches, 0: one per env (record, cause bits) / per slot, at most 1024; no result depends on it */
    float speed2_limit, ang_speed2_limit;   /* squared limits, >= 0 (+Inf: never) */
    const float *root_state;        /* [E][13]        EMLOCO_T_ROOT_STATE */
    const float *dof_state;         /* [E][69][2]     EMLOCO_T_DOF_STATE */
    const float *warm_start;        /* [E][96 * 3]    EMLOCO_T_WARM_START */
    const float *drive;             /* [E][69]        EMLOCO_T_PD_TARGET: the position targets, or under drive_mode 1 the torques (one buffer) */
    const float *rb_state;          /* [E][24][13]    EMLOCO_T_RIGID_BODY */
    const float *contact_force;     /* [E][24][3]     EMLOCO_T_CONTACT_FORCE */
    const float *dof_force;         /* [E][69]        EMLOCO_T_DOF_FORCE */
    const int64_t *progress_buf, *reset_buf, *terminate_buf;       /* [E] the task's buffers */
    uint32_t *ring;                 /* [E][R][EMLOCO_REC_WORDS], 16-byte aligned */
    uint32_t *slots;                /* [C][EMLOCO_REC_SLOT_WORDS(R)], 16-byte aligned */
    int32_t *counters;              /* [EMLOCO_REC_COUNTERS], zeroed by the caller */
    int32_t *last_capture_step;     /* [E], initialised by the caller to a value <= t0 - R */
    int32_t *cause_ws;              /* [E] scratch: the step's cause bits */
    uint8_t *request;               /* [E] or NULL */
} EmlocoRecorderBufs;

/* One launch, a pure copy: every env's record of step t into ring row t % R.  To be issued when the drive input of the step is in
 * place and before the rigid-body launch, on the stream every writer of the env state is ordered on.  (The pieces of a record lie
 * back to back, so only its 16-byte stores are wide: of the sources a root row is 52 bytes, a drive row 276.) */
int emloco_recorder_record(const EmlocoRecorderBufs *rec, int t, void *stream);
/* Three launches on the one stream: cause bits per env | the claim (one workgroup) | the copies into the slots claimed at this step.
 * To be issued where emloco_episode_stats_step is: behind the step's post-physics pass, ahead of any reset.
 * Both: a NULL structure or required pointer, n_env <= 0, depth < 1, n_slots < 1, t < t0, a misaligned ring or slot array, a limit
 * that is negative or NaN: -1 with the argument named in emloco_last_error(), nothing is written. */
int emloco_recorder_check(const EmlocoRecorderBufs *rec, int t, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The motion library's clip cache from raw clip frames: what utils/motion_lib_smpl.py `clip_cache` (the reference's
 * load_motion_with_skeleton + poselib, motion_lib_smpl.py:84-131, skeleton3d.py:1249-1272) builds per (clip, skeleton) pair on the host
 * in float64, for n_clips pairs in one launch in float32.  The frames of all clips lie in rows [0, n_frames_total) of every array;
 * clip c owns rows frame_start[c] .. frame_start[c] + n_frames[c] - 1.
 *   dev_quat_global [F][24][4]  global body rotations xyzw (the pickle's pose_quat_global);  dev_root_trans [F][3]
 *   dev_frame_start [n_clips] int64, dev_n_frames [n_clips] (>= 2), dev_fps [n_clips], dev_skel_id [n_clips]
 *   host_frame_start / host_n_frames / host_skel_id: HOST copies of the same arrays, validated here (no device read-back): at least 2
 *       frames, skel_id in [0, n_skel), every clip inside the F rows
 *   dev_local_translation [n_skel][24][3]  joint offsets of the skeletons
 *   host_parent [24]  HOST: -1 for body 0, otherwise an index below the child's;  host_taps [EMLOCO_MOTION_TAPS]  HOST: the gaussian
 *       filter's weights (sigma 2, radius 8, computed in float64 and normalised by the caller); both travel with the launch
 *   outputs, [F] rows each: dev_gts [24][3], dev_grs [24][4] (= the input, bit for bit), dev_lrs [24][4], dev_gvs [24][3],
 *       dev_gavs [24][3], dev_dvs [69]
 *   grid: workgroups to launch, 0 = one per (clip, 64-frame tile) up to 4096; the result does not depend on it
 * Angles are taken as 2 atan2(|xyz|, w); identical consecutive frames give exactly zero velocities.  A NULL array, n_clips < 1, a
 * clip with fewer than 2 frames or outside the arrays, a skel_id out of range, a bad parent list, a negative grid: -1, nothing is
 * launched. */
#define EMLOCO_MOTION_TAPS 17
#define EMLOCO_MOTION_BODIES 24
int emloco_motion_build(int n_clips, int n_skel, int64_t n_frames_total, const float *dev_quat_global, const float *dev_root_trans,
                        const int64_t *dev_frame_start, const int32_t *dev_n_frames, const float *dev_fps, const int32_t *dev_skel_id,
                        const int64_t *host_frame_start, const int32_t *host_n_frames, const int32_t *host_skel_id,
                        const float *dev_local_translation, const int32_t *host_parent, const float *host_taps, float *dev_gts,
                        float *dev_grs, float *dev_lrs, float *dev_gvs, float *dev_gavs, float *dev_dvs, int grid, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The get-up task (HumanoidPedestrianTerrainGetup, pacer/pacer/env/tasks/humanoid_pedestrain_terrain_getup.py): a reset is one of
 *   recovery   the env keeps the (fallen) state it terminated in and may not terminate for recovery_steps steps   :125-133,156-158
 *   fall       the env starts from a row of a pool of pre-generated fallen poses, same grace period              :137-141,160-174
 *   normal     the reset of emloco_task_reset*                                                                    :144-147
 * The state of the task lives in caller-owned device memory; P = n_pool fallen poses (the task uses P = n_env).  A slot of the pool is
 * held by at most one env: pool_taken[slot] != 0 and assign[env] == slot go together; a slot with pool_taken set that no env holds
 * (a pose with a non-finite value) is never handed out.  assign starts at -1 (the reference's 0 can free slot 0 under another env). */
#define EMLOCO_GETUP_STATS 6
enum {
    EMLOCO_GETUP_STAT_RECOVER = 0, EMLOCO_GETUP_STAT_FALL = 1, EMLOCO_GETUP_STAT_NORMAL = 2,   /* list entries of each kind, summed over splits */
    EMLOCO_GETUP_STAT_COUNTER_SUM = 3,     /* sum over envs and emloco_getup_flags calls of recovery_counter (after the decrement) */
    EMLOCO_GETUP_STAT_FLAG_CALLS = 4,      /* emloco_getup_flags calls */
    EMLOCO_GETUP_STAT_HELD = 5             /* envs held back by a counter > 0, summed over emloco_getup_flags calls */
};
typedef struct EmlocoGetupBufs {
    int32_t n_env, n_pool;
    const float *pool_root;         /* [P][13], velocities zero */
    const float *pool_dof;          /* [P][69][2], velocities zero */
    uint8_t *pool_taken;            /* [P] */
    int32_t *assign;                /* [E] slot the env holds, -1: none */
    int32_t *recovery_counter;      /* [E] */
    int64_t *progress_buf, *reset_buf, *terminate_buf;     /* [E] the task's buffers (EmlocoTaskBufs) */
    int32_t *split_ws;              /* [P] scratch of emloco_getup_split: the free slots in the order they are handed out */
    int64_t *stats;                 /* [EMLOCO_GETUP_STATS] running sums for the epoch's log line, or NULL; the caller reads and clears them */
} EmlocoGetupBufs;

/* _reset_actors :122-154 as ONE launch, without a host read: splits an id list (explicit ascending ids, or a list of
 * emloco_task_compact_done*: the entries in front of the first negative id are the list) into three.
 *   two uniforms per list entry: dev_rnd [n][2], or NULL: entry i draws reset_rnd_value(seed, i, 0 | 1), the hash emloco_task_reset_seeded
 *   fills its rows with
 *   1. every listed env that holds a slot gives it back (pool_taken[assign[env]] = 0, assign[env] = -1)                :123
 *   2. an entry is RECOVERY iff u0 < recovery_prob and terminate_buf[env] == 1                                         :125-128
 *   3. otherwise FALL iff u1 < fall_prob                                                                               :137-139
 *   4. otherwise NORMAL
 *   5. the j-th fall entry of the call, in list order, takes the j-th slot with pool_taken == 0 in the order P_key(0), P_key(1), ...
 *      (the keyed bijection of [0, P) the real paths are picked with, key = slot_key; the reference draws torch.randperm :165); a fall
 *      entry for which no free slot is left becomes a normal entry (the reference asserts :164)
 *   6. recovery_counter[env] = recovery_steps for recovery and fall entries, 0 for normal ones                          :147,157,169
 * dev_normal, dev_fall, dev_recover, dev_fall_slot (parallel to dev_fall): n + 1 entries each, in the input's order -- valid entries
 * first, -1 behind them, the count at [n]; the id-list contract of emloco_task_compact_done, so every list feeds the entry points of
 * this library as it is; none of them may alias the input list or another output.  Integer logic on one workgroup: the result does not depend on the launch.  n == 0 writes the four counts.
 * A NULL structure, list or output, n < 0 or above n_env, n_pool < 1, a missing buffer: -1, nothing is written. */
int emloco_getup_split(const EmlocoGetupBufs *getup, const int32_t *dev_env_ids, int n, const float *dev_rnd, uint64_t seed,
                       float recovery_prob, float fall_prob, int recovery_steps, uint32_t slot_key, int32_t *dev_normal,
                       int32_t *dev_fall, int32_t *dev_recover, int32_t *dev_fall_slot, void *stream);

/* _reset_fall_episode :160-174 and what _reset_env_tensors (humanoid.py:467-481) / _reset_task (humanoid_pedestrain_terrain.py:493-523)
 * do to an env whose state is in place, for the fall and recovery lists of emloco_getup_split (n + 1 or n entries each):
 *   fall list        pool row dev_fall_slot[i] -> the simulator's root / dof rows of env dev_fall[i], warm-start impulses zeroed, then the
 *                    forward kinematics of those envs (emloco_sim_fk_indexed: the body state is rewritten, where the reference leaves it
 *                    stale until the next simulate)
 *   both lists       progress_buf = reset_buf = terminate_buf = 0, contact forces zeroed, trajectory from the env's root position and
 *                    velocity, LocoVal waypoints, init_pose, init_vel, the inversion flag -- the device functions of emloco_task_reset
 *                    (reset_traj_to, reset_capture_pose), so the same bytes as emloco_task_traj_reset for the same rows; NO height fix
 *   recovery list    root, dof and body state and the warm-start impulses are not written at all
 * Random rows, [n][EMLOCO_RESET_RND] per list, row i for list entry i as emloco_task_traj_reset takes them: dev_rnd_fall and
 * dev_rnd_recover, or both NULL: made on the device into dev_rnd_ws ([2 n][EMLOCO_RESET_RND]: the fall list's rows, then the recovery
 * list's) from `seed` (fall) and ~seed (recovery), with a fresh real-path permutation as emloco_task_reset_seeded.
 * Of `reset` the trajectory fields, traj_verts, inverted, the three flag buffers, waypoint_traj, init_pose, init_vel are read.
 * A NULL simulator / structure / list, n < 0 or above the simulator's env count, one random block without the other, neither rows
 * nor a workspace, a missing buffer: -1 (-3: simulator not prepared), nothing is written. */
int emloco_getup_apply(struct EmlocoSim *sim, const EmlocoResetBufs *reset, const EmlocoGetupBufs *getup, const int32_t *dev_fall,
                       const int32_t *dev_fall_slot, const int32_t *dev_recover, int n, const float *dev_rnd_fall,
                       const float *dev_rnd_recover, uint64_t seed, float *dev_rnd_ws, void *stream);

/* _init_amp_obs_default (humanoid_amp.py:499-502, called for the fall envs: humanoid_pedestrain_terrain_getup.py:183-187): history rows 1..14 of the listed envs = their
 * newest row, in the layout bufs->amp_ring says (EMLOCO_AMP_PHYS_ROW).  NULL structure or list, n < 0 or above n_env, no AMP
 * buffer: -1, nothing is written. */
int emloco_getup_amp_default(const EmlocoTaskBufs *bufs, const int32_t *dev_env_ids, int n, void *stream);

/* _update_recovery_count :191-194 and the recovery part of _compute_reset :196-204 for all envs, to be launched right behind a step's
 * post-physics launch: recovery_counter = max(recovery_counter - 1, 0); where it is still > 0: reset_buf = terminate_buf = 0,
 * progress_buf -= 1.  (The reference decrements in pre_physics_step and masks in _compute_reset of the same step; nothing reads the
 * counter in between.)  NULL structure, n_env < 1, a missing buffer: -1, nothing is written. */
int emloco_getup_flags(const EmlocoGetupBufs *getup, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The crowd-aware terrain sensor (pacer_group_cnn.yaml: divide_group, num_env_group, velocity_map, sensor_res, sensor_extent;
 * humanoid_pedestrain_terrain.py:400-452,455-492,650-702,761-815,1212-1297, humanoid.py:221-226).  Env e belongs to group
 * e / group_size.  With `stamps` every env marks the map cells under its 10 x 20 root points (root_x x root_y, meshgrid 'ij', rotated
 * by the root's heading, world_points_to_map) in the owner map of its group; a marked cell reads int16(height + stamp_units).  The
 * res x res probes (probe_xy x probe_xy, 'ij', rotated by the heading of body head_body about its position) read
 *   channel 0      clip(centre_mean - vscale * min(cell(px, py), cell(px + 1, py + 1)), -3, 3) * 5, centre_mean as EMLOCO_POST_OBS has it
 *   channels 1, 2  (channels == 3) x, y of quat_rotate(inverse root heading, v_cell - v_own), clipped and scaled the same way; v_cell is
 *                  the root linear velocity of the member that marked (px, py), zero for an unmarked cell and without stamps
 * into obs[env][n_copy + (i * res + j) * channels + c]; flip_obs takes the same values at j' = res - 1 - j (no sign changes: the
 * reference's :471 discards its result).  The first n_copy columns of both rows are copied from src_obs / src_flip_obs (rows of
 * src_width floats; n_copy 0: nothing is copied, the two may be NULL).
 * Two members on one cell: the one with the highest member_in_group * 200 + point owns it (the reference's duplicate-index
 * assignment on one thread).  An owner word is (tag << tag_shift) | (that index + 1), written with atomicMax; only words whose tag
 * equals `tag` count, so the map is never cleared between calls as long as the caller raises `tag` by one per call (>= 1; it clears
 * the map before it starts over).  The root is body 0 of rb_state.  A non-finite root lands on cell (0, 0). */
#define EMLOCO_CROWD_ROOT_X 10
#define EMLOCO_CROWD_ROOT_Y 20
#define EMLOCO_CROWD_MAX_RES 64
typedef struct EmlocoCrowdBufs {
    int32_t n_env, group_size;      /* n_env a multiple of group_size (no groups: group_size = n_env) */
    int32_t hf_rows, hf_cols;       /* >= 2 each */
    int32_t head_body;
    int32_t res, channels;          /* 1 .. EMLOCO_CROWD_MAX_RES; 1 or 3 */
    int32_t stamps;                 /* 0 | 1 */
    int32_t stamp_units;            /* int16(1.7 / vertical_scale), the division in double precision */
    int32_t src_width, dst_width;   /* floats per row of src_obs / obs; dst_width >= n_copy + channels * res * res */
    int32_t n_copy;                 /* <= src_width */
    int32_t tag_shift;              /* group_size * 200 < 2^tag_shift <= 2^30, 1 <= tag < 2^(32 - tag_shift) */
    uint32_t tag;
    float hscale, vscale;
    const float *rb_state;          /* [E][24][13] */
    const int16_t *heightfield;     /* [hf_rows][hf_cols] */
    const float *probe_xy;          /* [res] float32(np.linspace(-extent, extent, res)) */
    const float *root_x;            /* [10] float32(np.linspace(-0.25, 0.25, 10)); stamps only */
    const float *root_y;            /* [20] float32(np.linspace(-0.5, 0.5, 20)); stamps only */
    uint32_t *owner;                /* [n_env / group_size][hf_rows * hf_cols]; stamps only */
    const float *src_obs;           /* [E][src_width] */
    const float *src_flip_obs;      /* [E][src_width] */
    float *obs;                     /* [E][dst_width] */
    float *flip_obs;                /* [E][dst_width] */
} EmlocoCrowdBufs;

/* Two launches on the one stream: the stamps of ALL n_env members (with `stamps`), then the rows of every env (dev_env_ids == NULL)
 * or of the n listed envs (entries of -1 are skipped).  A NULL structure or required pointer, n_env not a positive multiple of
 * group_size, res outside 1 .. 64, channels not 1 or 3, a map smaller than 2 x 2, a row too narrow, a tag or tag_shift outside the
 * ranges above, n < 0: -1 with the argument named in emloco_last_error(), nothing is written. */
int emloco_task_crowd_sensor(const EmlocoCrowdBufs *bufs, const int32_t *dev_env_ids, int n, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The crowd contact audit: how close the members of a group come to each other.  The members of a group do not collide (every env is
 * its own rigid-body problem); this measures, once per control step and without a host read, the capsule overlaps BETWEEN the
 * humanoids of a group from the collision segments the self-collision step uses (EmlocoSelfCollisionDesc: cap_a, cap_b, cap_r,
 * seg_body).  Env e belongs to group e / group_size, as in the crowd sensor.  All arithmetic is fp32 in the stated order, no
 * contraction, sums left to right:
 *   segment i of env e on body b = seg_body[i]:  R = q2mat(quat_b) (the stored quaternion, not normalised), o = p_b - p_root(e),
 *       A_i = o + R cap_a[e][i], B_i = o + R cap_b[e][i], r_i = cap_r[e][i] -- relative to the env's OWN root (body 0), so the rounding
 *       is that of a body, not of the terrain's extent
 *   bound_e = max_i(max(|A_i|, |B_i|) + r_i), |v| = sqrtf((x x + y y) + z z)
 *   env e is finite when the 24 x 7 position and quaternion values of its bodies are; a non-finite env gets flags = 1, zeros and -1
 *       in its other fields, and is nobody's neighbour.  No index is derived from a state value.
 *   ordered pair (e, m), m != e of the same group, both finite:  s = p_root(m) - p_root(e), d_xy = sqrtf(s.x s.x + s.y s.y);
 *       for every (i, j): seg_seg_closest(A_i, B_i, A_j(m) + s, B_j(m) + s) -> c1, c2; dv = c1 - c2; dist2 = (dv.x dv.x + dv.y dv.y) +
 *       dv.z dv.z; rs = r_i + r_j; dist2 < rs rs: pen_ij = rs - sqrtf(dist2).  pen(e, m) = max pen_ij, 0 if none.
 * The kernels skip a member whose root is farther than bound_e + bound_m + 1e-3 and a segment pair whose midpoints are farther apart
 * than the half lengths and radii allow; both follow from the triangle inequality, and the result is that of the full sweep.  Maxima,
 * minima and counts do not depend on the visiting order: the same bytes from run to run. */
typedef struct EmlocoCrowdContactNow {
    float nearest;          /* horizontal (xy) root distance to the nearest finite member of the group, 0 if none */
    float pen;              /* deepest capsule penetration against any member [m], 0 if none */
    int32_t nearest_member; /* env id (the lowest at that distance), -1 if none */
    int32_t pen_member;     /* env id of the member at `pen`, -1 if pen == 0 */
    int32_t pen_segs;       /* own segment | (other segment << 8), -1 if pen == 0; of the lowest (member, own, other) at `pen` */
    int32_t n_pen;          /* members with penetration > 0 */
    int32_t n_near;         /* members with root distance < near_dist */
    int32_t flags;          /* bit 0: this env's state is non-finite */
} EmlocoCrowdContactNow;

/* One finished game.  A step counts as finite when flags == 0; the distances only look at steps with a finite neighbour. */
typedef struct EmlocoCrowdContactRecord {
    float min_nearest;      /* -1: no step of the game had a finite neighbour */
    float mean_nearest;     /* (float)(double sum in step order / steps with a neighbour), 0 if none */
    float max_pen;          /* deepest `pen` of the game, 0 if none */
    int32_t steps, nonfinite_steps;         /* finite / non-finite steps */
    int32_t near_steps, contact_steps;      /* steps with n_near > 0 / n_pen > 0 */
    int32_t contacts;                       /* sum of n_pen */
    int32_t pen_member, pen_segs, pen_step; /* of the first step at max_pen (1-based, counting every call of the game); -1 if none */
    int32_t first_contact_step;             /* 1-based, -1 if none */
} EmlocoCrowdContactRecord;

#define EMLOCO_CROWD_CONTACT_WS 16          /* 32-bit words of game_ws per env */
#define EMLOCO_CROWD_CONTACT_TOTALS 13
#define EMLOCO_CROWD_CONTACT_MOMENTS 13
enum {                                      /* totals[e][k] and the epoch vector */
    EMLOCO_CCT_STEPS = 0, EMLOCO_CCT_NONFINITE_STEPS = 1, EMLOCO_CCT_CONTACT_STEPS = 2, EMLOCO_CCT_CONTACTS = 3,
    EMLOCO_CCT_NEAR_STEPS = 4, EMLOCO_CCT_SUM_NEAREST = 5, EMLOCO_CCT_SUM_PEN = 6,
    EMLOCO_CCT_MAX_PEN = 7,                 /* maximum */
    EMLOCO_CCT_MIN_NEAREST = 8,             /* minimum over the steps with a neighbour, 0 if there was none */
    EMLOCO_CCT_GAMES = 9, EMLOCO_CCT_GAMES_CONTACT = 10, EMLOCO_CCT_GAMES_START_CONTACT = 11,
    EMLOCO_CCT_NEIGHBOUR_STEPS = 12         /* steps with a finite neighbour: what SUM_NEAREST is a sum over */
};
enum {                                      /* moments of emloco_crowd_contacts_reduce: sums and counts only */
    EMLOCO_CCM_GAMES = 0, EMLOCO_CCM_GAMES_CONTACT = 1, EMLOCO_CCM_GAMES_START_CONTACT = 2, EMLOCO_CCM_STEPS = 3,
    EMLOCO_CCM_CONTACT_STEPS = 4, EMLOCO_CCM_NEAR_STEPS = 5, EMLOCO_CCM_CONTACTS = 6, EMLOCO_CCM_NONFINITE_STEPS = 7,
    EMLOCO_CCM_SUM_MAX_PEN = 8, EMLOCO_CCM_SUM_MAX_PEN2 = 9,       /* over the games with a contact */
    EMLOCO_CCM_SUM_MIN_NEAREST = 10, EMLOCO_CCM_SUM_MEAN_NEAREST = 11, EMLOCO_CCM_GAMES_NEIGHBOUR = 12   /* over the games with min_nearest >= 0 */
};
typedef struct EmlocoCrowdContacts {
    int32_t n_env, group_size;      /* group_size >= 2 divides n_env */
    int32_t n_seg;                  /* 24 .. EMLOCO_SC_MAXSEG (include/emloco_sim.h) */
    int32_t games_per_env;          /* slots per env of `records` */
    float near_dist;                /* finite, > 0 */
    int32_t _pad;
    const float *rb_state;          /* [E][24][13] */
    const float *cap_a, *cap_b;     /* [E][n_seg][3] body frame */
    const float *cap_r;             /* [E][n_seg] */
    const uint8_t *seg_body;        /* [n_seg], every entry < 24 (checked on the device: a larger one reads body 23) */
    float *caps_ws;                 /* [E][EMLOCO_SC_MAXSEG][8] workspace: A, r, B, half length + r per segment */
    float *roots_ws;                /* [E][4] workspace: root position, bound (-1: non-finite) */
    /* emloco_crowd_contacts_accumulate only */
    const uint8_t *done8;           /* [E] this step's end-of-game flags, or */
    const int64_t *done64;          /* [E] the same as int64; at most one of the two, neither: no game ever ends */
    const int32_t *slot;            /* [E] slot of the game in progress; records only */
    uint32_t *game_ws;              /* [E][EMLOCO_CROWD_CONTACT_WS] the games' accumulators, zeros to start */
    EmlocoCrowdContactRecord *records;      /* [E][games_per_env] or NULL */
    double *totals;                 /* [E][EMLOCO_CROWD_CONTACT_TOTALS] or NULL; zeros to start, cleared by the epoch reduction */
} EmlocoCrowdContacts;

/* Two launches: the root-relative segments and bounds of every env, then now[E] (one wave per env).  A NULL structure, rb_state,
 * capsule array, workspace or now, n_env < 1, group_size < 2 or not dividing n_env, n_seg outside 24 .. EMLOCO_SC_MAXSEG, near_dist
 * not finite and positive: -1 with the argument named in emloco_last_error(), nothing is launched. */
int emloco_crowd_contacts(const EmlocoCrowdContacts *c, EmlocoCrowdContactNow *now, void *stream);

/* One launch, one thread per env, behind emloco_crowd_contacts on the same stream: now[e] joins the accumulators of env e's game; with
 * `totals` it also adds to the epoch totals.  Where this step's flag is set the game ends: with `records` and 0 <= slot[e] <
 * games_per_env its record goes to records[e][slot[e]], and the accumulators start over.  A NULL structure, now or game_ws, n_env < 1,
 * both done arrays, records without slot or with games_per_env < 1: -1, nothing is launched. */
int emloco_crowd_contacts_accumulate(const EmlocoCrowdContacts *c, const EmlocoCrowdContactNow *now, void *stream);

/* records[e][g], g < games[e], to moments[EMLOCO_CROWD_CONTACT_MOMENTS] on one workgroup, in double, in a fixed tree order; sums and
 * counts only, so one all-reduce(sum) over ranks is correct.  A NULL pointer, n_env < 1, games_per_env < 1: -1. */
int emloco_crowd_contacts_reduce(int n_env, int games_per_env, const EmlocoCrowdContactRecord *records, const int32_t *games,
                                 double *moments, void *stream);

/* totals[E][EMLOCO_CROWD_CONTACT_TOTALS] to epoch[EMLOCO_CROWD_CONTACT_TOTALS] the same way (MAX_PEN as maximum, MIN_NEAREST as
 * minimum over the envs with a neighbour step), then totals is cleared.  A NULL pointer, n_env < 1: -1. */
int emloco_crowd_contacts_epoch_reduce(int n_env, double *totals, double *epoch, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The group observation (cfg["env"]["group_obs"]; humanoid_pedestrain_terrain.py:312-335,444-450,481-484 and
 * compute_group_observation :1613-1666): the EMLOCO_PEOPLE_JOINTS selected joints and the root velocity of the EMLOCO_PEOPLE_TOPK
 * nearest members of the env's group, in the env's heading frame.  Env e belongs to group e / group_size, as in the crowd sensor.
 * All arithmetic is fp32 in the stated order, no contraction:
 *   distance from e to member m:  d = p_root(m) - p_root(e), dist = sqrtf((d.x d.x + d.y d.y) + d.z d.z), z included; a non-finite
 *       distance counts as +inf
 *   selection:  the five members other than e itself with the lowest (dist, member index), ascending.  DEPARTURE: the reference takes
 *       topk(6) and drops the first hit, which is the env itself only while no other member is at distance 0, and torch.topk leaves
 *       the order among equal distances unspecified (with all roots equal the reference's function drops member 4 for every env; the
 *       shipped crowd configuration resets every env to one spot, so ties are the common case at the first step).  The rule here
 *       equals the reference's whenever the distances are distinct.
 *   row, neighbour-major (the reference's bytes, whatever its view(B, -1, top_k, 3) suggests):
 *       [0, 150)    [k][j][xyz]  position of body EMLOCO_PEOPLE_BODIES[j] of neighbour k minus the env's ROOT position
 *       [150, 165)  [k][xyz]     the neighbour's root linear velocity (absolute, not relative)
 *       each triple rotated by the inverse heading quaternion of the env's root rotation (calc_heading_quat_inv, my_quat_rotate: the
 *       functions of the location observation); a neighbour with dist > EMLOCO_PEOPLE_FAR has its 30 + 3 values written as zeros
 *   mirrored row (:481-484): the same 55 triples with y negated.  DEPARTURE: the reference finds the block at
 *       traj + num_height_points, which with velocity_map lies inside the height map; here the mirrored block is the block's own
 *       columns, whatever the map's width.
 * The rows go to columns [col, col + EMLOCO_PEOPLE_WIDTH) of obs and flip_obs (row stride obs_stride floats); no other byte of
 * either is touched.  The selection is a minimum over the integer key (distance bits, member index): the same bytes from run to
 * run. */
#define EMLOCO_PEOPLE_TOPK 5
#define EMLOCO_PEOPLE_JOINTS 10
#define EMLOCO_PEOPLE_WIDTH 165
#define EMLOCO_PEOPLE_FAR 10.0f
#define EMLOCO_PEOPLE_BODIES {0, 1, 5, 9, 3, 7, 16, 21, 18, 23}
typedef struct EmlocoCrowdPeople {
    int32_t n_env, group_size;      /* group_size >= EMLOCO_PEOPLE_TOPK + 1 divides n_env */
    int32_t obs_stride, col;        /* floats per row of obs / flip_obs; 0 <= col, col + EMLOCO_PEOPLE_WIDTH <= obs_stride */
    const float *rb_state;          /* [E][24][13] */
    float *roots_ws;                /* [E][4] workspace: the root positions, packed */
    float *obs;                     /* [E][obs_stride] */
    float *flip_obs;                /* [E][obs_stride] */
    int32_t *neighbours;            /* [E][EMLOCO_PEOPLE_TOPK] the chosen members' env ids, nearest first, or NULL */
} EmlocoCrowdPeople;

/* Two launches on the one stream: the packed roots of ALL n_env members, then the rows (and neighbours) of every env
 * (dev_env_ids == NULL) or of the n listed envs (entries of -1 are skipped).  A NULL structure or buffer, group_size < 6 (five
 * others must exist; the reference's topk(6) fails there too), n_env not a positive multiple of group_size, col < 0 or
 * col + 165 > obs_stride, n < 0: -1 with the argument named in emloco_last_error(), nothing is launched. */
int emloco_task_crowd_people(const EmlocoCrowdPeople *p, const int32_t *dev_env_ids, int n, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The crowd spawn (cfg["env"]["group_spawn"], this project's key): at a reset every listed member of a group is put on a random
 * admissible spot of its group's square, at least min_dist from every member of the group that is standing at that moment.  The
 * reference's placement for groups (Terrain.sample_valid_locations(..., sample_groups=True), humanoid_pedestrain_terrain.py:1196-1204,
 * never called there) draws a group centre plus a U(-8, 8) m offset per member and checks neither clearance nor walkability.
 *
 * Env e belongs to group e / group_size, as in the sensor.  A call gets three things:
 *   an id list dev_env_ids[n].  Entries of -1 are skipped (and so is any entry outside [0, n_env)).  NULL means every env, and row
 *       i is env i.
 *   u[n][tries][2], uniforms in [0, 1) chosen by the caller.  Row i belongs to list position i.  If an env is listed twice, its
 *       lowest list position counts.
 *   the roots of all envs, read as roots[e * root_stride + 0/1].  Horizontal distance only.
 * All arithmetic is fp32 in the stated order, with no contraction.
 *   candidate k of env e:  t = 2.0f * u - 1.0f;  c = centre[g] + extent * t, one multiply then one add, per axis.
 *   admissible:  min_x <= c.x <= max_x and min_y <= c.y <= max_y, and walkable[ix * cols + iy] == 0, with ix = (int)(c.x / hscale)
 *       and iy = (int)(c.y / hscale): IEEE division truncated, the reference's world_points_to_map.  Both indices must lie in
 *       [0, rows) x [0, cols).  Otherwise the candidate is inadmissible.
 *   standing members of e's group:  every member j != e whose root x and y are finite, and that is either not listed in this call,
 *       or is listed and already placed by this call (then at its new spot).
 *   clearance2(c):  the minimum over standing members of (dx * dx) + (dy * dy).  It is +inf when no member is standing.
 *   order:  the listed members of a group are placed in ascending env index, one after another.  Each sees the ones placed before
 *       it at their new spots.
 *   choice:  take the lowest admissible k with clearance2 >= min_dist * min_dist.  If there is none, take the admissible k with the
 *       largest clearance2, lowest k on ties, and set flag EMLOCO_SPAWN_CROWDED.  If no candidate is admissible, the spot is
 *       centre[g], tried = -1, and flag EMLOCO_SPAWN_NO_GROUND is set (and EMLOCO_SPAWN_CROWDED beside it when
 *       clearance2(centre[g]) < min_dist * min_dist).
 * Outputs, written for listed envs only; no other byte is touched:
 *   place_xy[e][2]
 *   info[e] = {clearance2 of the spot taken, tried = the k taken, flags, order = the env's rank among its group's placements in
 *       this call}
 *   mark_ws[E] is a workspace.  It holds -1 everywhere on entry and again on exit.
 * Nothing in the rule depends on scheduling.  Minima are exact, there are no float atomics, and equal inputs give equal bytes. */
#define EMLOCO_SPAWN_CROWDED 1
#define EMLOCO_SPAWN_NO_GROUND 2
#define EMLOCO_SPAWN_MAX_TRIES 8
#define EMLOCO_SPAWN_MAX_GROUP 2048
typedef struct EmlocoCrowdSpawnInfo {
    float clearance2;
    int32_t tried, flags, order;
} EmlocoCrowdSpawnInfo;

typedef struct EmlocoCrowdSpawn {
    int32_t n_env, group_size;      /* 1 <= group_size <= EMLOCO_SPAWN_MAX_GROUP divides n_env (the group's roots are staged on chip) */
    int32_t tries, root_stride;     /* 1 <= tries <= EMLOCO_SPAWN_MAX_TRIES; floats between two envs' roots, >= 2 */
    int32_t rows, cols;             /* of walkable */
    float hscale;
    float min_x, max_x, min_y, max_y;   /* the box a spot must lie in, bounds included */
    float extent, min_dist;         /* half the side of a group's square; both in metres */
    int32_t _pad;
    const float *roots;             /* [E] roots, root_stride floats apart: x, y first */
    const int16_t *walkable;        /* [rows][cols], 0: walkable */
    const float *centres;           /* [E / group_size][2] */
    int32_t *mark_ws;               /* [E] workspace, -1 everywhere between calls */
    float *place_xy;                /* [E][2] */
    EmlocoCrowdSpawnInfo *info;     /* [E] */
} EmlocoCrowdSpawn;

/* Two launches on the one stream: the lowest list position of every listed env into mark_ws, then one workgroup per group places
 * its listed members and clears their marks.  u is on the device.  A NULL structure or buffer, group_size < 1 or above
 * EMLOCO_SPAWN_MAX_GROUP, n_env not a positive multiple of group_size, tries outside 1..8, root_stride < 2, rows, cols or hscale not
 * positive, extent not finite and positive, min_dist negative or non-finite, an empty box (min > max, or a NaN bound), n < 0, u NULL
 * with work to do: -1 with the argument named in emloco_last_error(), nothing is launched.  n == 0 with a list: 0, nothing is
 * launched. */
int emloco_task_crowd_spawn(const EmlocoCrowdSpawn *s, const int32_t *dev_env_ids, int n, const float *u, void *stream);

#ifdef __cplusplus
}
#endif
#endif

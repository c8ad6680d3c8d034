"""ctypes binding of libemloco_hip.so (the C ABI declared in include/*.h).

There is no CPU fallback: if the gfx950 library is missing or no MI355X is visible, every entry
point that needs the device raises `EmlocoError`.  Build the library with `python -m emloco_amd.build`.
"""
import ctypes as C
import os

from ._abi import EmlocoError, bind  # noqa: F401  (EmlocoError is raised under this module's name everywhere)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EMLOCO_LIB") or os.path.join(HERE, "lib", "libemloco_hip.so")     # (EMLOCO_LIB: another build of the library, for A/B runs)

NB, NDOF, MAXC, MAXCAND = 24, 69, 20, 96
SELF_OBS, TRAJ_SAMPLES, TRAJ_VERTS, HEIGHT_POINTS = 368, 15, 101, 1024
TASK_OBS = 2 * TRAJ_SAMPLES + HEIGHT_POINTS
OBS = SELF_OBS + TASK_OBS
AMP_ROW, AMP_STEPS = 206, 15

T_ROOT_STATE, T_DOF_STATE, T_RIGID_BODY, T_CONTACT_FORCE, T_DOF_FORCE, T_PD_TARGET, T_WARM_START = range(7)
POST_ADVANCE, POST_OBS, POST_REWARD, POST_RESET, POST_AMP_SHIFT, POST_AMP_ROW = 1, 2, 4, 8, 16, 32
POST_STEP = 63
POST_SKIP_DONE = 64
POST_AMP_DONE_ONLY = 128


class SimParams(C.Structure):
    """EmlocoSimParams (include/emloco_sim.h)."""
    _fields_ = [("n_sub", C.c_int32), ("n_iter", C.c_int32), ("h", C.c_float), ("gravity_z", C.c_float),
                ("contact_offset", C.c_float), ("erp", C.c_float), ("max_depen_vel", C.c_float),
                ("mu", C.c_float), ("ang_damping", C.c_float), ("max_ang_vel", C.c_float),
                ("ground_z", C.c_float), ("cfm", C.c_float), ("warm", C.c_float), ("drive_mode", C.c_int32)]


class ModelDesc(C.Structure):
    """EmlocoModelDesc (include/emloco_sim.h)."""
    _fields_ = [("n_env", C.c_int32), ("parent", C.POINTER(C.c_int32)), ("geom_type", C.POINTER(C.c_int32)),
                ("joint_off", C.POINTER(C.c_float)), ("mass", C.POINTER(C.c_float)), ("com", C.POINTER(C.c_float)),
                ("inertia", C.POINTER(C.c_float)), ("geom_a", C.POINTER(C.c_float)), ("geom_b", C.POINTER(C.c_float)),
                ("geom_r", C.POINTER(C.c_float)), ("kp", C.POINTER(C.c_float)), ("kd", C.POINTER(C.c_float)),
                ("armature", C.POINTER(C.c_float)), ("effort", C.POINTER(C.c_float))]


class SelfCollisionDesc(C.Structure):
    """EmlocoSelfCollisionDesc (include/emloco_sim.h)."""
    _fields_ = [("n_pairs", C.c_int32), ("pairs", C.POINTER(C.c_uint8)), ("cap_a", C.POINTER(C.c_float)),
                ("cap_b", C.POINTER(C.c_float)), ("cap_r", C.POINTER(C.c_float)), ("k", C.c_float), ("c", C.c_float),
                ("max_pen", C.c_float), ("mu", C.c_float), ("n_seg", C.c_int32), ("seg_body", C.POINTER(C.c_uint8))]


class TaskBufs(C.Structure):
    """EmlocoTaskBufs (include/emloco_task.h); pointers are raw device addresses."""
    _fields_ = [("n_env", C.c_int32), ("hf_rows", C.c_int32), ("hf_cols", C.c_int32), ("head_body", C.c_int32),
                ("n_dof_subset", C.c_int32),
                ("dt", C.c_float), ("traj_dur", C.c_float), ("sample_dt", C.c_float), ("hscale", C.c_float),
                ("vscale", C.c_float), ("power_coef", C.c_float), ("fail_dist", C.c_float),
                ("max_episode_length", C.c_float),
                ("rb_state", C.c_void_p), ("dof_state", C.c_void_p), ("dof_force", C.c_void_p),
                ("contact_force", C.c_void_p),
                ("betas", C.c_void_p), ("traj_verts", C.c_void_p), ("heightfield", C.c_void_p),
                ("left_to_right", C.c_void_p), ("contact_body_mask", C.c_void_p), ("key_bodies", C.c_void_p),
                ("dof_subset", C.c_void_p),
                ("progress_buf", C.c_void_p), ("reset_buf", C.c_void_p), ("terminate_buf", C.c_void_p),
                ("obs_buf", C.c_void_p), ("flip_obs_buf", C.c_void_p), ("rew_buf", C.c_void_p),
                ("reward_raw", C.c_void_p), ("amp_obs_buf", C.c_void_p), ("amp_ring", C.c_int32)]


class ResetBufs(C.Structure):
    """EmlocoResetBufs (include/emloco_task.h)."""
    _fields_ = [("flags", C.c_int32), ("n_motions", C.c_int32), ("n_real", C.c_int32), ("n_valid", C.c_int32),
                ("n_dof_subset", C.c_int32), ("hf_rows", C.c_int32), ("hf_cols", C.c_int32),
                ("fixed_x", C.c_float), ("fixed_y", C.c_float), ("dt", C.c_float), ("height_tolerance", C.c_float),
                ("vert_dt", C.c_float), ("dtheta_max", C.c_float), ("speed_min", C.c_float), ("speed_max", C.c_float),
                ("accel_max", C.c_float), ("sharp_prob", C.c_float), ("hybrid_prob", C.c_float),
                ("traj_dur", C.c_float), ("sample_dt", C.c_float), ("hscale", C.c_float), ("vscale", C.c_float),
                ("gts", C.c_void_p), ("grs", C.c_void_p), ("lrs", C.c_void_p), ("gvs", C.c_void_p), ("gavs", C.c_void_p),
                ("dvs", C.c_void_p), ("motion_len", C.c_void_p), ("motion_dt", C.c_void_p), ("motion_nframes", C.c_void_p),
                ("motion_start", C.c_void_p), ("real_traj", C.c_void_p), ("heightfield", C.c_void_p),
                ("valid_x", C.c_void_p), ("valid_y", C.c_void_p), ("betas", C.c_void_p), ("key_bodies", C.c_void_p),
                ("dof_subset", C.c_void_p), ("traj_verts", C.c_void_p), ("inverted", C.c_void_p),
                ("progress_buf", C.c_void_p), ("reset_buf", C.c_void_p), ("terminate_buf", C.c_void_p),
                ("waypoint_traj", C.c_void_p), ("init_pose", C.c_void_p), ("init_vel", C.c_void_p),
                ("amp_obs_buf", C.c_void_p), ("motion_ids", C.c_void_p), ("motion_times", C.c_void_p), ("ground_h", C.c_void_p),
                ("real_pick", C.c_void_p), ("real_pick_key", C.c_uint32), ("amp_ring", C.c_int32)]


RESET_RND = 512
RESET_RANDOM_HEADING, RESET_INIT_HEADING, RESET_HEADING_INVERSION, RESET_ADJUST_ROOT_VEL, RESET_REAL_PATH, RESET_FIXED_LOCATION = 1, 2, 4, 8, 16, 32
RESET_NO_AMP_HISTORY = 64
RND_MOTION, RND_TIME, RND_YAW, RND_SPEED, RND_LOC, RND_REAL, RND_REAL_PICK, RND_INVERSION, RND_HEADING, RND_SPEED0 = range(10)
RND_DTHETA, RND_SHARP, RND_BERN, RND_DSPEED = 16, 116, 216, 316


def _fmix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def real_pick_perm(i, n, key):
    """Row of the real-path table list entry i takes (restates reset_kernels.hip: real_pick_perm, the keyed bijection of
    [0, n) that stands where the reference calls random.sample, traj_generator.py:132)."""
    bits = 2
    while (1 << bits) < n:
        bits += 2
    half = bits >> 1
    mask = (1 << half) - 1
    x = i % n
    while True:
        l, r = x >> half, x & mask
        for rnd in range(4):
            f = _fmix32((r * 0x9E3779B1 + key + rnd * 0x85EBCA6B) & 0xFFFFFFFF) & mask
            l, r = r, l ^ f
        x = (l << half) | r
        if x < n:
            return x


POOL_FLOATS = 512              # EMLOCO_POOL_FLOATS


class ResetPool(C.Structure):   # EmlocoResetPool
    _fields_ = [("k", C.c_int32), ("cur", C.c_void_p), ("cur_tag", C.c_void_p), ("next", C.c_void_p), ("next_tag", C.c_void_p),
                ("next_seed", C.c_uint64)]


GETUP_STATS = 6                # EMLOCO_GETUP_STATS
GETUP_STAT_RECOVER, GETUP_STAT_FALL, GETUP_STAT_NORMAL, GETUP_STAT_COUNTER_SUM, GETUP_STAT_FLAG_CALLS, GETUP_STAT_HELD = range(6)


class GetupBufs(C.Structure):
    """EmlocoGetupBufs (include/emloco_task.h): the get-up task's fall pool and per-env recovery state."""
    _fields_ = [("n_env", C.c_int32), ("n_pool", C.c_int32), ("pool_root", C.c_void_p), ("pool_dof", C.c_void_p),
                ("pool_taken", C.c_void_p), ("assign", C.c_void_p), ("recovery_counter", C.c_void_p),
                ("progress_buf", C.c_void_p), ("reset_buf", C.c_void_p), ("terminate_buf", C.c_void_p),
                ("split_ws", C.c_void_p), ("stats", C.c_void_p)]


REC_WORDS, REC_POST_WORDS, REC_COUNTERS = 512, 892, 8          # EMLOCO_REC_*
REC_NONFINITE, REC_SPEED, REC_ANG_SPEED, REC_EARLY_FALL, REC_REQUEST = 1, 2, 4, 8, 16


def rec_slot_words(depth):
    """EMLOCO_REC_SLOT_WORDS(R)"""
    return 4 + int(depth) * REC_WORDS + REC_POST_WORDS


class RecorderBufs(C.Structure):
    """EmlocoRecorderBufs (include/emloco_task.h): the flight recorder's view of the simulator, the task's flags and its own buffers."""
    _fields_ = [("n_env", C.c_int32), ("depth", C.c_int32), ("n_slots", C.c_int32), ("drive_mode", C.c_int32), ("t0", C.c_int32),
                ("cause_mask", C.c_int32), ("early_fall_steps", C.c_int32), ("grid", C.c_int32),
                ("speed2_limit", C.c_float), ("ang_speed2_limit", C.c_float),
                ("root_state", C.c_void_p), ("dof_state", C.c_void_p), ("warm_start", C.c_void_p), ("drive", C.c_void_p),
                ("rb_state", C.c_void_p), ("contact_force", C.c_void_p), ("dof_force", C.c_void_p),
                ("progress_buf", C.c_void_p), ("reset_buf", C.c_void_p), ("terminate_buf", C.c_void_p),
                ("ring", C.c_void_p), ("slots", C.c_void_p), ("counters", C.c_void_p), ("last_capture_step", C.c_void_p),
                ("cause_ws", C.c_void_p), ("request", C.c_void_p)]


CROWD_ROOT_X, CROWD_ROOT_Y, CROWD_MAX_RES = 10, 20, 64          # EMLOCO_CROWD_*


class CrowdBufs(C.Structure):
    """EmlocoCrowdBufs (include/emloco_task.h): the crowd-aware terrain sensor's inputs, owner map and observation rows."""
    _fields_ = [("n_env", C.c_int32), ("group_size", C.c_int32), ("hf_rows", C.c_int32), ("hf_cols", C.c_int32), ("head_body", C.c_int32),
                ("res", C.c_int32), ("channels", C.c_int32), ("stamps", C.c_int32), ("stamp_units", C.c_int32),
                ("src_width", C.c_int32), ("dst_width", C.c_int32), ("n_copy", C.c_int32), ("tag_shift", C.c_int32), ("tag", C.c_uint32),
                ("hscale", C.c_float), ("vscale", C.c_float),
                ("rb_state", C.c_void_p), ("heightfield", C.c_void_p), ("probe_xy", C.c_void_p), ("root_x", C.c_void_p),
                ("root_y", C.c_void_p), ("owner", C.c_void_p), ("src_obs", C.c_void_p), ("src_flip_obs", C.c_void_p),
                ("obs", C.c_void_p), ("flip_obs", C.c_void_p)]


CROWD_CONTACT_WS, CROWD_CONTACT_TOTALS, CROWD_CONTACT_MOMENTS = 16, 13, 13          # EMLOCO_CROWD_CONTACT_*
(CCT_STEPS, CCT_NONFINITE_STEPS, CCT_CONTACT_STEPS, CCT_CONTACTS, CCT_NEAR_STEPS, CCT_SUM_NEAREST, CCT_SUM_PEN, CCT_MAX_PEN,
 CCT_MIN_NEAREST, CCT_GAMES, CCT_GAMES_CONTACT, CCT_GAMES_START_CONTACT, CCT_NEIGHBOUR_STEPS) = range(13)       # EMLOCO_CCT_*
(CCM_GAMES, CCM_GAMES_CONTACT, CCM_GAMES_START_CONTACT, CCM_STEPS, CCM_CONTACT_STEPS, CCM_NEAR_STEPS, CCM_CONTACTS,
 CCM_NONFINITE_STEPS, CCM_SUM_MAX_PEN, CCM_SUM_MAX_PEN2, CCM_SUM_MIN_NEAREST, CCM_SUM_MEAN_NEAREST, CCM_GAMES_NEIGHBOUR) = range(13)   # EMLOCO_CCM_*


class CrowdContactNow(C.Structure):
    """EmlocoCrowdContactNow (include/emloco_task.h): one env's distances and overlaps at one step."""
    _fields_ = [("nearest", C.c_float), ("pen", C.c_float), ("nearest_member", C.c_int32), ("pen_member", C.c_int32),
                ("pen_segs", C.c_int32), ("n_pen", C.c_int32), ("n_near", C.c_int32), ("flags", C.c_int32)]


class CrowdContactRecord(C.Structure):
    """EmlocoCrowdContactRecord (include/emloco_task.h): one finished game of the crowd contact audit."""
    _fields_ = [("min_nearest", C.c_float), ("mean_nearest", C.c_float), ("max_pen", C.c_float), ("steps", C.c_int32),
                ("nonfinite_steps", C.c_int32), ("near_steps", C.c_int32), ("contact_steps", C.c_int32), ("contacts", C.c_int32),
                ("pen_member", C.c_int32), ("pen_segs", C.c_int32), ("pen_step", C.c_int32), ("first_contact_step", C.c_int32)]


class CrowdContacts(C.Structure):
    """EmlocoCrowdContacts (include/emloco_task.h): inputs, workspaces and game state of the crowd contact audit."""
    _fields_ = [("n_env", C.c_int32), ("group_size", C.c_int32), ("n_seg", C.c_int32), ("games_per_env", C.c_int32),
                ("near_dist", C.c_float), ("_pad", C.c_int32),
                ("rb_state", C.c_void_p), ("cap_a", C.c_void_p), ("cap_b", C.c_void_p), ("cap_r", C.c_void_p), ("seg_body", C.c_void_p),
                ("caps_ws", C.c_void_p), ("roots_ws", C.c_void_p), ("done8", C.c_void_p), ("done64", C.c_void_p), ("slot", C.c_void_p),
                ("game_ws", C.c_void_p), ("records", C.c_void_p), ("totals", C.c_void_p)]


PEOPLE_TOPK, PEOPLE_JOINTS, PEOPLE_WIDTH = 5, 10, 165          # EMLOCO_PEOPLE_*
PEOPLE_FAR = 10.0                                               # EMLOCO_PEOPLE_FAR
PEOPLE_BODIES = (0, 1, 5, 9, 3, 7, 16, 21, 18, 23)              # EMLOCO_PEOPLE_BODIES


class CrowdPeople(C.Structure):
    """EmlocoCrowdPeople (include/emloco_task.h): the group observation's inputs, workspace and observation rows."""
    _fields_ = [("n_env", C.c_int32), ("group_size", C.c_int32), ("obs_stride", C.c_int32), ("col", C.c_int32),
                ("rb_state", C.c_void_p), ("roots_ws", C.c_void_p), ("obs", C.c_void_p), ("flip_obs", C.c_void_p),
                ("neighbours", C.c_void_p)]


SPAWN_CROWDED, SPAWN_NO_GROUND, SPAWN_MAX_TRIES, SPAWN_MAX_GROUP = 1, 2, 8, 2048          # EMLOCO_SPAWN_*


class CrowdSpawnInfo(C.Structure):
    """EmlocoCrowdSpawnInfo (include/emloco_task.h): what the crowd spawn decided for one env."""
    _fields_ = [("clearance2", C.c_float), ("tried", C.c_int32), ("flags", C.c_int32), ("order", C.c_int32)]


class CrowdSpawn(C.Structure):
    """EmlocoCrowdSpawn (include/emloco_task.h): the crowd spawn's inputs, workspace and outputs."""
    _fields_ = [("n_env", C.c_int32), ("group_size", C.c_int32), ("tries", C.c_int32), ("root_stride", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32), ("hscale", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("extent", C.c_float), ("min_dist", C.c_float), ("_pad", C.c_int32),
                ("roots", C.c_void_p), ("walkable", C.c_void_p), ("centres", C.c_void_p), ("mark_ws", C.c_void_p),
                ("place_xy", C.c_void_p), ("info", C.c_void_p)]


class LocoValStep(C.Structure):
    """EmlocoLocoValStep (include/emloco_predictor.h)."""
    _fields_ = [("n_env", C.c_int32), ("step_to_pred", C.c_int32), ("gamma", C.c_float), ("inversion_penalty", C.c_float),
                ("min_cum_rewards", C.c_float), ("max_cum_rewards", C.c_float),
                ("current_rewards", C.c_void_p), ("current_lengths", C.c_void_p), ("current_combined_rewards", C.c_void_p),
                ("discount_coefs", C.c_void_p), ("waypoint_traj", C.c_void_p), ("init_pose", C.c_void_p), ("init_vel", C.c_void_p),
                ("traj13", C.c_void_p), ("pose", C.c_void_p), ("vel", C.c_void_p), ("target", C.c_void_p), ("weight", C.c_void_p),
                ("staged_reward", C.c_void_p), ("staged_done", C.c_void_p)]          # staged mode (both NULL: off)


class LocoValEval(C.Structure):
    """EmlocoLocoValEval (include/emloco_predictor.h): the per-env game state of the LocoVal evaluation (`run.py --test`)."""
    _fields_ = [("n_env", C.c_int32), ("step_to_pred", C.c_int32), ("games_per_env", C.c_int32), ("_pad", C.c_int32),
                ("gamma", C.c_double), ("coef", C.c_void_p), ("c_disc", C.c_void_p), ("tp_disc", C.c_void_p),
                ("cr", C.c_void_p), ("c_loc", C.c_void_p), ("c_pow", C.c_void_p), ("tp_cr", C.c_void_p), ("tp_loc", C.c_void_p),
                ("tp_pow", C.c_void_p), ("steps", C.c_void_p), ("games", C.c_void_p), ("done", C.c_void_p), ("terminated", C.c_void_p),
                ("inverted", C.c_void_p), ("n_full", C.c_void_p), ("waypoint_traj", C.c_void_p), ("init_pose", C.c_void_p),
                ("init_vel", C.c_void_p), ("traj13", C.c_void_p), ("pose", C.c_void_p), ("vel", C.c_void_p), ("row_mask", C.c_void_p)]


EVAL_MAX_NETS = 8           # EMLOCO_EVAL_MAX_NETS


class LocoValNet(C.Structure):
    """EmlocoLocoValNet (include/emloco_predictor.h): one network of the evaluation's table."""
    _fields_ = [("variant", C.c_int32), ("_pad", C.c_int32), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p), ("value", C.c_void_p)]


class LocoValNets(C.Structure):
    """EmlocoLocoValNets: the networks scored on the same games (emloco_locoval_eval_fwd_multi / _finish_multi)."""
    _fields_ = [("n_nets", C.c_int32), ("_pad", C.c_int32), ("net", LocoValNet * EVAL_MAX_NETS)]


TRACK_SAMPLES = 16          # EMLOCO_TRACK_SAMPLES
TRACK_MOMENTS = 12          # EMLOCO_TRACK_MOMENTS
EPISODE_RUNNING = 4         # EMLOCO_EPISODE_RUNNING
EPISODE_MOMENTS = 15        # EMLOCO_EPISODE_MOMENTS
EPISODE_GAME_OUT = 8        # EMLOCO_EPISODE_GAME_OUT


class LocoValTrack(C.Structure):
    """EmlocoLocoValTrack (include/emloco_predictor.h): the path tracking of the evaluation's games (emloco_locoval_eval_track)."""
    _fields_ = [("stride", C.c_int32), ("root_stride", C.c_int32), ("dt", C.c_float), ("traj_dur", C.c_float),
                ("root_pos", C.c_void_p), ("traj_verts", C.c_void_p), ("progress_buf", C.c_void_p),
                ("sum_dev", C.c_void_p), ("sum_sample_dev", C.c_void_p), ("path_len", C.c_void_p), ("max_dev", C.c_void_p),
                ("prev_xy", C.c_void_p), ("last_sample_dev", C.c_void_p), ("n_samples", C.c_void_p), ("dev_now", C.c_void_p)]


def default_sim_params(**kw):
    """Engine parameters of pacer.yaml:93-104 / config.py:143-163 mapped onto EmlocoSimParams."""
    p = dict(n_sub=2, n_iter=4, h=(1.0 / 60.0) / 2, gravity_z=-9.81, contact_offset=0.02, erp=0.2,
             max_depen_vel=10.0, mu=1.0, ang_damping=0.01, max_ang_vel=100.0, ground_z=0.0, cfm=1e-4, warm=1.0, drive_mode=0)
    p.update(kw)
    return SimParams(**p)


_lib = None


def load():
    """Load the library (no device needed for loading; device entry points fail without a GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; it must be the one the process binds first, otherwise torch
    # later fails with "No HIP GPUs are available" (two runtimes with the same soname).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise EmlocoError(f"{LIB_PATH} is missing: run `python -m emloco_amd.build` (hipcc, gfx950). "
                          "There is no CPU fallback.")
    _lib = bind(C.CDLL(LIB_PATH))         # every prototype of include/*.h, typed (_abi.py)
    return _lib


def check(rc, what=""):
    """The one place a status of the C ABI becomes an EmlocoError: `rc` is what the entry point `what` returned on this thread, just now.
    The message carries the library's own text for that failure (emloco_last_error, every entry point of include/*.h sets it)."""
    if rc != 0:
        msg = load().emloco_last_error()
        raise EmlocoError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def require_device():
    lib = load()
    if lib.emloco_device_count() < 1:
        raise EmlocoError("no MI355X / HIP device visible: the emloco hot path has no CPU fallback")
    return lib

"""CPU execution of the HIP kernel sources through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from emloco_amd._lib import ModelDesc, SelfCollisionDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_EXTRA = os.environ.get("EMLOCO_EMU_EXTRA", "").split()          # e.g. -DEMLOCO_SIM_PAIR=1: the experimental two-envs-per-wave rigid-body kernel
_SO = os.path.join(_HERE, "_build", "libemu" + ("_" + "".join(c for c in "".join(_EXTRA) if c.isalnum()) if _EXTRA else "") + ".so")
_SRCS = ["emu_sim.cpp", "emu_task.cpp", "emu_predictor.cpp", "emu_ppo.cpp", "emu_eval.cpp", "emu_runtime.cpp", "hip/hip_runtime.h"]
def build():
    """g++ over the kernel sources; every file under emloco_amd/csrc and include/ is a dependency.  Built under a file lock into a
    temporary name and renamed, so that the workers of a parallel test run neither build twice at once nor load a half-written file."""
    import fcntl
    csrc, inc = os.path.join(_ROOT, "emloco_amd", "csrc"), os.path.join(_ROOT, "include")
    deps = [os.path.join(_HERE, s) for s in _SRCS] + [os.path.join(d, f) for d in (csrc, inc) for f in os.listdir(d)]
    deps = [d for d in deps if os.path.isfile(d)]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                cpps = [os.path.join(_HERE, s) for s in _SRCS if s.endswith(".cpp") and os.path.exists(os.path.join(_HERE, s))]
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi",
                                       "-I", _HERE, "-o", tmp] + _EXTRA + cpps + ["-lpthread"])
                os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        # the evaluation's records as locoval_eval.py views them (RECORD_DTYPE, TRACK_DTYPE)
        assert _lib.emu_locoval_record_size() == 48 and _lib.emu_locoval_track_record_size() == 32
        _lib.emu_locoval_track_reduce.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        _lib.emu_traj_densify_error.restype = C.c_char_p
    return _lib


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def model_desc(arr):
    return ModelDesc(arr["mass"].shape[0], _p(arr["parent"], C.c_int32), _p(arr["geom_type"], C.c_int32),
                     _p(arr["joint_off"]), _p(arr["mass"]), _p(arr["com"]), _p(arr["inertia"]), _p(arr["geom_a"]),
                     _p(arr["geom_b"]), _p(arr["geom_r"]), _p(arr["kp"]), _p(arr["kd"]), _p(arr["armature"]),
                     _p(arr["effort"]))


def sim_step(osim, n_calls=1, expect_error=None, cost_ticks=None, order=None, ids=None, skip=None, parts=0, grid_pad=0):
    """Advance an oracle.Sim-shaped state holder with the emulated HIP kernel (same arrays, in place).  `cost_ticks`: a uint32 array
    [n_env] that takes the key of the cost-ordered dispatch (what emloco_sim_cost_ticks reads back on the device).  The launch-level
    arguments of emloco_sim_step / emloco_sim_step_subset: `order` int32 [n_env], a permutation -- workgroup i of a full launch steps
    env order[i] (emloco_sim_set_cost_order); `ids` int32, a compacted id list (valid ids first, -1 after them): only the listed envs
    are stepped, unsplit; `skip` int64 [n_env]: envs with a non-zero flag are left untouched; `parts`: the split launch
    (emloco_sim_set_split; 0: the EMLOCO_EMU_PARTS variable decides); `grid_pad`: that many workgroups past the launch's last one."""
    assert cost_ticks is None or (cost_ticks.dtype == np.uint32 and cost_ticks.shape == (osim.E,) and cost_ticks.flags.c_contiguous)
    assert order is None or (order.dtype == np.int32 and order.flags.c_contiguous and sorted(order.tolist()) == list(range(osim.E)))
    assert ids is None or (ids.dtype == np.int32 and ids.flags.c_contiguous and ids.ndim == 1 and len(ids) <= osim.E and ids.max(initial=-1) < osim.E)
    assert skip is None or (skip.dtype == np.int64 and skip.shape == (osim.E,) and skip.flags.c_contiguous)
    assert ids is None or skip is None, "exactly one of skip flags / id list, as emloco_sim_step_subset asks"
    lib().emu_sim_set_cost_ticks(C.c_void_p(cost_ticks.ctypes.data if cost_ticks is not None else None))
    fl = lib().emu_sim_set_launch
    fl.argtypes, fl.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int], None
    fl(_vp(order), _vp(ids), len(ids) if ids is not None else 0, _vp(skip), int(parts), int(grid_pad))
    desc = model_desc(osim.arr)
    sc = getattr(osim, "sc", None)
    scd = None
    if sc is not None:
        scd = SelfCollisionDesc(int(sc["pairs"].shape[0]), _p(sc["pairs"], C.c_uint8), _p(sc["cap_a"]), _p(sc["cap_b"]),
                                _p(sc["cap_r"]), float(sc["k"]), float(sc["c"]), float(sc["max_pen"]), float(sc.get("mu", 1.0)),
                                int(sc["seg_body"].shape[0]) if sc.get("seg_body") is not None else 0,
                                _p(sc["seg_body"], C.c_uint8) if sc.get("seg_body") is not None else None)
    lib().emu_sim_set_self_collision(C.byref(scd) if scd is not None else None)
    hf = getattr(osim, "hf", None)
    fn = lib().emu_sim_set_heightfield
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    if hf is not None:
        m = osim.model
        mv = getattr(osim, "hf_mv", None)
        fn(hf.ctypes.data, hf.shape[0], hf.shape[1], m.hf_hs, m.hf_vs, m.hf_ox, m.hf_oy, mv.ctypes.data if mv is not None else None)
    else:
        fn(None, 0, 0, 0.0, 0.0, 0.0, 0.0, None)
    rc = lib().emu_sim_step(C.byref(osim.params), C.byref(desc), _p(osim.root_state), _p(osim.dof_state),
                            _p(osim.pd_target), _p(osim.rb_state), _p(osim.contact_force), _p(osim.dof_force),
                            _p(osim.lambda_ws), C.c_int(n_calls))
    if expect_error is None:
        assert rc == 0
    return rc


def sim_fk(osim, ids=None, grid=0):
    """sim_fk_kernel: body states of every env, or of the envs of an int32 id list up to its first -1; `grid` > 0: that many
    workgroups stride over the list."""
    desc = model_desc(osim.arr)
    assert ids is None or (ids.dtype == np.int32 and ids.flags.c_contiguous and ids.max(initial=-1) < osim.E)
    fn = lib().emu_sim_fk
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert fn(C.byref(desc), _vp(osim.root_state), _vp(osim.dof_state), _vp(osim.rb_state), _vp(ids), len(ids) if ids is not None else 0, int(grid)) == 0


def sim_copy_rows(src, dst, ids, row_len, n_env, grid_pad=0):
    """copy_rows_kernel (the *_indexed setters with a foreign `dev_full`) on host arrays: `dst` may be a view into a larger buffer."""
    assert src.dtype == np.float32 and dst.dtype == np.float32 and ids.dtype == np.int32
    assert src.flags.c_contiguous and dst.flags.c_contiguous and ids.flags.c_contiguous
    fn = lib().emu_sim_copy_rows
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    fn.restype = None
    fn(src.ctypes.data, dst.ctypes.data, ids.ctypes.data, len(ids), row_len, n_env, int(grid_pad))


# ------------------------------------------------------------------ task kernels
def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class TaskHost:
    """Host-memory buffers laid out like the task's device buffers, for running the kernel under emulation."""
    L2R = [0, 5, 6, 7, 8, 1, 2, 3, 4, 9, 10, 11, 12, 13, 19, 20, 21, 22, 23, 14, 15, 16, 17, 18]

    def __init__(self, E, heightfield, dt=1.0 / 30.0, episode_len=168):
        from emloco_amd import _lib as L
        self.L = L
        self.E = E
        f32 = lambda *s: np.zeros(s, np.float32)
        self.rb_state = f32(E, 24, 13); self.rb_state[:, :, 6] = 1
        self.dof_state = f32(E, 69, 2)
        self.dof_force = f32(E, 69)
        self.contact_force = f32(E, 24, 3)
        self.betas = f32(E, 17)
        self.traj_verts = f32(E, 101, 3)
        self.heightfield = np.ascontiguousarray(heightfield, dtype=np.int16)
        self.l2r = np.asarray(self.L2R, np.int32)
        mask = np.zeros(24, np.uint8); mask[[7, 3, 8, 4]] = 1
        self.contact_mask = mask
        self.key_bodies = np.asarray([7, 3, 22, 17], np.int32)
        self.dof_subset = np.concatenate([np.arange(3 * j, 3 * j + 3) for j in range(23) if j not in (3, 7, 17, 22)]).astype(np.int32)
        self.progress = np.zeros(E, np.int64)
        self.reset = np.ones(E, np.int64)
        self.terminate = np.ones(E, np.int64)
        self.obs = f32(E, L.OBS); self.flip_obs = f32(E, L.OBS)
        self.rew = f32(E); self.reward_raw = f32(E, 2)
        self.amp = f32(E, L.AMP_STEPS, L.AMP_ROW)
        vdt = episode_len * dt / 100.0
        self.dt, self.traj_dur = dt, 101 * vdt
        self.episode_len = episode_len

    def bufs(self):
        L = self.L
        return L.TaskBufs(self.E, self.heightfield.shape[0], self.heightfield.shape[1], 13, len(self.dof_subset),
                          self.dt, self.traj_dur, 0.4, 0.1, 0.005, 0.0005, 4.0, float(self.episode_len),
                          _vp(self.rb_state), _vp(self.dof_state), _vp(self.dof_force), _vp(self.contact_force),
                          _vp(self.betas), _vp(self.traj_verts), _vp(self.heightfield), _vp(self.l2r),
                          _vp(self.contact_mask), _vp(self.key_bodies), _vp(self.dof_subset),
                          _vp(self.progress), _vp(self.reset), _vp(self.terminate), _vp(self.obs), _vp(self.flip_obs),
                          _vp(self.rew), _vp(self.reward_raw), _vp(self.amp))

    def post_physics(self, mode, env_ids=None):
        b = self.bufs()
        fn = lib().emu_task_post_physics
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        if env_ids is None:
            rc = fn(C.byref(b), mode, None, 0)
        else:
            ids = np.ascontiguousarray(env_ids, np.int32)
            rc = fn(C.byref(b), mode, _vp(ids), len(ids))
        assert rc == 0


def task_pd_targets(actions, offset, scale, zero_mask, copy=None):
    """pd_targets_kernel; copy: a float32 array like `actions` that takes the kernel's copy of the actions (emloco_task_pd_targets_copy)"""
    actions = np.ascontiguousarray(actions, np.float32)
    out = np.zeros_like(actions)
    fn = lib().emu_task_pd_targets_copy
    fn.argtypes = [C.c_int] + [C.c_void_p] * 6
    fn(actions.shape[0], _vp(actions), _vp(np.ascontiguousarray(offset, np.float32)),
       _vp(np.ascontiguousarray(scale, np.float32)), _vp(np.ascontiguousarray(zero_mask, np.uint8)), _vp(out), _vp(copy))
    return out


def chain_prof(buf):
    """the stamps of emloco_task_chain_profile under emulation: `buf` (int64 [16], or None to stop) is stamped by every later reset_obs"""
    assert buf is None or (buf.dtype == np.int64 and buf.shape == (16,) and buf.flags.c_contiguous)
    fn = lib().emu_task_set_chain_prof
    fn.argtypes, fn.restype = [C.c_void_p], None
    fn(_vp(buf))


# ------------------------------------------------------------------ reset kernels
RESET_SAMPLE, RESET_FK, RESET_FINISH, RESET_HISTORY = 1, 2, 4, 8
RESET_ALL = 15


class ResetHost:
    """Host-memory simulator state, motion cache and reset buffers for running the reset kernels under emulation: `arr` holds the arrays a
    reset writes (root_state, dof_state, rb_state, contact_force, warm_start, traj_verts, inverted, progress, reset, terminate,
    waypoint_traj, init_pose, init_vel, amp, motion_ids, motion_times, ground_h), `const` what it reads (the motion cache's arrays,
    heightfield, valid_x, valid_y, betas, real_traj), `scalars` the scalar fields of EmlocoResetBufs by name."""

    def __init__(self, models, arr, const, scalars):
        from emloco_amd import _lib as L
        self.L, self.models, self.arr, self.scalars = L, models, arr, dict(scalars)
        self.const = {k: np.ascontiguousarray(v) for k, v in const.items()}
        self.key_bodies = np.asarray([7, 3, 22, 17], np.int32)
        self.dof_subset = np.concatenate([np.arange(3 * j, 3 * j + 3) for j in range(23) if j not in (3, 7, 17, 22)]).astype(np.int32)

    def bufs(self, **override):
        b = self.L.ResetBufs()
        for k, v in {**self.scalars, **override}.items():
            setattr(b, k, v)
        a, c = self.arr, self.const
        for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs", "motion_len", "motion_dt", "motion_nframes", "motion_start", "heightfield",
                  "valid_x", "valid_y", "betas"):
            setattr(b, k, c[k].ctypes.data)
        b.real_traj = c["real_traj"].ctypes.data if b.n_real > 0 else None
        b.key_bodies, b.dof_subset = self.key_bodies.ctypes.data, self.dof_subset.ctypes.data
        for k, f in (("traj_verts", "traj_verts"), ("inverted", "inverted"), ("progress", "progress_buf"), ("reset", "reset_buf"),
                     ("terminate", "terminate_buf"), ("waypoint_traj", "waypoint_traj"), ("init_pose", "init_pose"), ("init_vel", "init_vel"),
                     ("amp", "amp_obs_buf"), ("motion_ids", "motion_ids"), ("motion_times", "motion_times"), ("ground_h", "ground_h")):
            setattr(b, f, a[k].ctypes.data)
        return b

    def _sim_args(self):
        a = self.arr
        self._desc = model_desc(self.models)
        return [C.byref(self._desc)] + [_vp(a[k]) for k in ("root_state", "dof_state", "rb_state", "contact_force", "warm_start")]

    def fill_rnd(self, ids, n, seed, rnd):
        fn = lib().emu_reset_fill_rnd
        fn.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        assert fn(_vp(ids), n, seed, _vp(rnd)) == 0

    def stages(self, stages, ids, n, rnd, **override):
        """the launches of emloco_task_reset chosen by `stages` (RESET_* bits), in the launcher's order"""
        b = self.bufs(**override)
        fn = lib().emu_task_reset_stages
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [C.c_void_p, C.c_int, C.c_void_p]
        assert fn(stages, C.byref(b), *self._sim_args(), _vp(ids), n, _vp(rnd)) == 0

    def reset_obs(self, task_host, ids, n, seed=0, rnd_ws=None, rnd=None, pool=None, live_mode=0, skip=None, may_refuse=False, **override):
        """emloco_task_reset_obs_pooled through the launcher's own arithmetic (emloco::chain_pack); task_host: a TaskHost whose state
        arrays are this object's.  pool: None or (k, cur, cur_tag, next, next_tag, next_seed) -- float32 [k][512] / uint64 [k] arrays or
        None; with a pool `ids` holds n + 1 entries.  live_mode / skip: the live envs' role and its flag snapshot (int64 [E]).
        may_refuse=True: returns 0, or -1 for a pool argument that emloco::chain_pool_error refuses, instead of asserting 0."""
        b, pb = self.bufs(**override), task_host.bufs()
        pb.amp_ring = b.amp_ring
        fn = lib().emu_task_reset_obs
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p,
                                                                                  C.c_void_p, C.c_int, C.c_void_p]
        pl = None
        if pool is not None:
            k, cur, cur_tag, nxt, nxt_tag, next_seed = pool
            pl = self.L.ResetPool(k, *(a.ctypes.data if a is not None else None for a in (cur, cur_tag, nxt, nxt_tag)), next_seed)
        rc = fn(C.byref(pb), C.byref(b), *self._sim_args(), _vp(ids), n, seed, _vp(rnd_ws), _vp(rnd), C.byref(pl) if pl is not None else None,
                live_mode, _vp(skip))
        if may_refuse:
            lib().emu_task_reset_obs_error.restype = C.c_char_p
            assert rc in (0, -1) and (rc == 0) == (lib().emu_task_reset_obs_error() == b""), rc
            return rc
        assert rc == 0, rc

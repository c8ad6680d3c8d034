"""HumanoidPedestrianTerrainGetup: the get-up curriculum on top of the terrain task -- recovery episodes, fall-state resets and the
schedule between them.

Mirror of pacer/pacer/env/tasks/humanoid_pedestrain_terrain_getup.py (file name spelt as in the reference), class
HumanoidPedestrianTerrainGetup :21-204.  A reset is one of three kinds (`_reset_actors` :122-154):

    recovery   with probability `recoveryEpisodeProb`, an env that TERMINATED keeps the fallen state it is in
    fall       otherwise, with probability `fallInitProb`, the env starts from a row of a pool of pre-generated fallen poses
    normal     otherwise the reference-state reset of HumanoidPedestrianTerrain

and a recovery or fall env cannot terminate (nor does its progress advance) for `recoverySteps` steps.

On the device (include/emloco_task.h, emloco_getup_*) a reset is, without the host reading a count anywhere:
    1. emloco_getup_split        the id list -> normal / fall / recovery lists, pool slots handed out, recovery counters set
    2. emloco_task_reset[_seeded] on the normal list -- the existing entry point, unchanged
    3. emloco_getup_apply        pool rows and forward kinematics for the fall list; flags, trajectory, LocoVal inputs for both others
    4. emloco_task_post_physics(POST_OBS | POST_AMP_ROW) on the reset envs (the three lists are the input list)
    5. emloco_getup_amp_default  the fall envs' AMP history = their newest row (:183-187)
and a step is the parent's post-physics launch with emloco_getup_flags right behind it (:191-204).

The launch arrangements that decide per env from the flags launch's reset_buf -- `fused_chain`, `overlap_obs`, `overlap_reset` and the
returns bookkeeping of `attach_returns` -- would act on a flag that emloco_getup_flags clears afterwards (an env would get its AMP row
twice): this task runs the sequential arrangement, and switching one of the four on raises.

Deviations from the reference:
  * Body state after a fall reset.  The reference leaves the body-state tensors of a fall-reset env stale until the next simulate; here
    forward kinematics rewrites them, as for every reset in this repository.
  * `assign` starts at -1, not 0: the reference's zero start can free slot 0 while another env holds it (:123).
  * Free slots are taken in the order of a keyed permutation (a fresh key per call) instead of torch.randperm (:165); a fall entry for
    which no slot is free becomes a normal reset where the reference asserts (:164).
  * A pool row with a non-finite value is marked taken for good, so it is never handed out.

Whether a policy learns to stand up with this curriculum on this physics has not been shown: the task provides the mechanism.
"""
import ctypes as C

import numpy as np
import torch

from ... import _lib as L
from ...gym import gymtorch
from ...utils.flags import flags
from .humanoid_pedestrain_terrain import HumanoidPedestrianTerrain

_MASK64 = 0xFFFFFFFFFFFFFFFF


def _sequential_only(name):
    """a launch-arrangement switch that stays off: reading gives False, switching it on raises"""
    def fget(self):
        return False

    def fset(self, value):
        if value:
            raise RuntimeError(f"HumanoidPedestrianTerrainGetup runs the sequential launch arrangement: {name} decides per env from the "
                               "reset_buf of the flags launch, which emloco_getup_flags clears afterwards for an env in recovery")
    return property(fget, fset)


class HumanoidPedestrianTerrainGetup(HumanoidPedestrianTerrain):
    fused_chain = _sequential_only("fused_chain")
    overlap_obs = _sequential_only("overlap_obs")
    overlap_reset = _sequential_only("overlap_reset")

    def __init__(self, cfg, sim_params, physics_engine, device_type, device_id, headless):
        env = cfg["env"]
        from ...crowd_sensor import is_crowd_config
        if is_crowd_config(env):
            raise NotImplementedError("HumanoidPedestrianTerrainGetup: the crowd sensor (divide_group / velocity_map / sensor_res / sensor_extent) "
                                      "is built for HumanoidPedestrianTerrain only")
        self._recovery_episode_prob_tgt = self._recovery_episode_prob = float(env["recoveryEpisodeProb"])       # :24-26
        self._recovery_steps_tgt = self._recovery_steps = int(env["recoverySteps"])
        self._fall_init_prob_tgt = self._fall_init_prob = float(env["fallInitProb"])
        self.getup_schedule = bool(env.get("getup_schedule", False))
        if flags.server_mode:                                                                                       # :27-29
            self._recovery_episode_prob_tgt = self._recovery_episode_prob = 1.0
            self._fall_init_prob_tgt = self._fall_init_prob = 0.0
        self._reset_fall_env_ids = []
        self._getup_bufs = None
        super().__init__(cfg=cfg, sim_params=sim_params, physics_engine=physics_engine, device_type=device_type, device_id=device_id,
                         headless=headless)
        E, dev = self.num_envs, self.device
        self._recovery_counter = torch.zeros(E, device=dev, dtype=torch.int32)
        self._fall_root_states = torch.zeros((E, 13), device=dev)
        self._fall_dof_state = torch.zeros((E, self.num_dof, 2), device=dev)
        self._fall_taken = torch.zeros(E, device=dev, dtype=torch.uint8)            # availalbe_fall_states :33
        self._fall_assign = torch.full((E,), -1, device=dev, dtype=torch.int32)     # fall_id_assignments :34 (-1: none, see above)
        self._getup_split_ws = torch.zeros(E, device=dev, dtype=torch.int32)
        self._getup_stats = torch.zeros(L.GETUP_STATS, device=dev, dtype=torch.int64)
        self._getup_lists = torch.full((4, E + 1), -1, device=dev, dtype=torch.int32)     # normal | fall | recovery | the fall entries' slots
        self._getup_calls = 0
        self._generate_fall_states()

    # ------------------------------------------------------------------ schedule (:50-57)
    def update_getup_schedule(self, epoch_num, getup_udpate_epoch=5000):
        if epoch_num > getup_udpate_epoch:
            self._recovery_episode_prob = self._recovery_episode_prob_tgt
            self._fall_init_prob = self._fall_init_prob_tgt
        else:
            self._recovery_episode_prob = 0
            self._fall_init_prob = 1

    def attach_returns(self, step_struct, before=None):
        if step_struct is not None:
            raise RuntimeError("HumanoidPedestrianTerrainGetup runs the sequential launch arrangement: the returns bookkeeping of "
                               "attach_returns reads the reset_buf of the flags launch, which emloco_getup_flags clears afterwards for an "
                               "env in recovery")
        super().attach_returns(None)

    # ------------------------------------------------------------------ the fall pool (:65-113)
    def _generate_fall_states(self):
        """Drop every humanoid from a random orientation with random PD targets, simulate 150 frames, keep the poses they come to rest
        in (velocities zeroed) as the pool; clears the pool's bookkeeping."""
        max_steps = 150
        E = self.num_envs
        self.wait_obs()
        self.wait_reset()
        env_ids = torch.arange(E, device=self.device, dtype=torch.long)
        root_states = self._initial_humanoid_root_states.clone()
        root_states[:, 3:7] = torch.nn.functional.normalize(torch.randn(E, 4, device=self.device), dim=-1)
        root_states[:, :2] = self.terrain.sample_valid_locations(E, env_ids)
        root_states[:, 2] += self.get_center_heights(root_states, env_ids=env_ids).mean(dim=-1)
        self._humanoid_root_states[:] = root_states
        ids32 = self._humanoid_actor_ids.contiguous()
        self.gym.set_actor_root_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self._root_states), gymtorch.unwrap_tensor(ids32), E)
        self.gym.set_dof_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(torch.zeros_like(self._dof_state)),
                                              gymtorch.unwrap_tensor(ids32), E)
        native = getattr(self.sim, "native", None)
        if native is not None:
            native.warm_start.zero_()                     # contact impulses of the games that were in progress
        rand_actions = torch.from_numpy(np.random.uniform(-0.5, 0.5, size=[E, self.get_action_size()])).float().to(self.device)
        self.pre_physics_step(rand_actions)
        self.gym.simulate_n(self.sim, max_steps)          # the reference's 150 gym.simulate calls as one launch
        self._refresh_sim_tensors()
        self._fall_root_states.copy_(self._humanoid_root_states)
        self._fall_root_states[:, 7:13] = 0
        self._fall_dof_state.copy_(self._dof_state.view(E, -1, 2)[:, :self.num_dof])
        self._fall_dof_state[:, :, 1] = 0
        bad = ~(torch.isfinite(self._fall_root_states).all(dim=1) & torch.isfinite(self._fall_dof_state).flatten(1).all(dim=1))
        self._fall_taken.copy_(bad.to(torch.uint8))       # a pose that blew up is never handed out: taken, and no env holds it
        self._fall_assign.fill_(-1)

    def resample_motions(self):                           # :115-120
        info = super().resample_motions()
        self._generate_fall_states()
        self.reset()
        return info

    # ------------------------------------------------------------------ device path
    def _make_getup_bufs(self):
        p = lambda t: t.data_ptr()
        assert self.progress_buf.dtype == self.reset_buf.dtype == self._terminate_buf.dtype == torch.int64
        return L.GetupBufs(self.num_envs, self.num_envs, p(self._fall_root_states), p(self._fall_dof_state), p(self._fall_taken),
                           p(self._fall_assign), p(self._recovery_counter), p(self.progress_buf), p(self.reset_buf), p(self._terminate_buf),
                           p(self._getup_split_ws), p(self._getup_stats))

    def _getup_ready(self):
        if self._reset_bufs is None:
            self._reset_bufs = self._make_reset_bufs()
            if hasattr(self, "_amp_ring_to_bufs"):
                self._amp_ring_to_bufs()
        if self._getup_bufs is None:
            self._getup_bufs = self._make_getup_bufs()
        if getattr(self, "_rnd_seed0", None) is None:
            self._rnd_seed0 = int(torch.initial_seed()) & 0xFFFFFFFFFFFF
        return self._post_bufs if self._post_bufs is not None else self._ensure_post_bufs()

    def _getup_reset(self, ids32, n, rnd=None, split_rnd=None, seeded_rows=False):
        """The five launches of the module docstring for the id list `ids32` (n entries; explicit ids or a compacted list).
        `rnd` [n][RESET_RND] (a test's hook): row j serves the j-th entry of EACH of the three lists, so that with every entry normal
        the call is the parent's reset with the same rows; `split_rnd` [n][2]: the uniforms of the split.  Without them the rows come
        from per-call seeds (torch's seed and a call counter): made on the device when `seeded_rows`, else drawn with torch.rand as the
        parent's reset(env_ids) draws them."""
        from ...sim import current_stream_handle
        post_bufs = self._getup_ready()
        lib, dev, E = self._post.lib, torch.device(self.device), self.num_envs
        st = current_stream_handle(dev)
        self._getup_calls += 1
        seed = (self._rnd_seed0 * 0x9E3779B97F4A7C15 + 0x6A09E667F3BCC908 + self._getup_calls) & _MASK64
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        normal, fall, recover, slot = (self._getup_lists[i] for i in range(4))
        g, sim = C.byref(self._getup_bufs), self.sim.native._h
        L.check(lib.emloco_getup_split(g, ptr(ids32), n, ptr(split_rnd), C.c_uint64(seed), float(self._recovery_episode_prob),
                                       float(self._fall_init_prob), int(self._recovery_steps), (seed * 0xD6E8FEB86659FD93 & _MASK64) >> 32,
                                       ptr(normal), ptr(fall), ptr(recover), ptr(slot), st), "emloco_getup_split")
        if rnd is None and seeded_rows:
            if getattr(self, "_rnd_ws", None) is None:
                self._rnd_ws = torch.empty((E, L.RESET_RND), device=self.device)
            L.check(lib.emloco_task_reset_seeded(sim, C.byref(self._reset_bufs), ptr(normal), n, C.c_uint64(seed), ptr(self._rnd_ws), st),
                    "emloco_task_reset_seeded")
        else:
            rows = rnd if rnd is not None else torch.rand((n, L.RESET_RND), device=self.device)
            L.check(lib.emloco_task_reset(sim, C.byref(self._reset_bufs), ptr(normal), n, ptr(rows), st), "emloco_task_reset")
        if rnd is None and getattr(self, "_getup_rnd_ws", None) is None:
            self._getup_rnd_ws = torch.empty((2 * E, L.RESET_RND), device=self.device)
        L.check(lib.emloco_getup_apply(sim, C.byref(self._reset_bufs), g, ptr(fall), ptr(slot), ptr(recover), n, ptr(rnd), ptr(rnd),
                                       C.c_uint64(seed ^ 0x5851F42D4C957F2D), None if rnd is not None else ptr(self._getup_rnd_ws), st),
                "emloco_getup_apply")
        self._post.run(post_bufs, L.POST_OBS | L.POST_AMP_ROW, ids32[:n])
        L.check(lib.emloco_getup_amp_default(C.byref(post_bufs), ptr(fall), n, st), "emloco_getup_amp_default")
        if flags.init_heading and flags.heading_inversion:
            self._traj_gen.inverted = self._inverted_u8.view(torch.bool)     # the kernels write 0 / 1 bytes: a view, no launch
        self.inverted = self._traj_gen.show_inverted()

    def _fused_reset_envs(self, env_ids, rnd=None, split_rnd=None):
        ids32 = self._humanoid_actor_ids[env_ids.to(self.device)].contiguous()
        self._getup_reset(ids32, int(ids32.numel()), rnd=rnd, split_rnd=split_rnd)

    def reset_done(self, rnd=None, split_rnd=None):
        """Reset every env whose reset_buf is set without the host reading which ones (the parent's reset_done, sequential
        arrangement), each as a recovery, fall or normal reset."""
        from ...sim import current_stream_handle
        if not (getattr(self, "_fused_reset", False) and getattr(self, "_traj_gen", None) is not None):
            return super().reset_done()
        E, dev = self.num_envs, torch.device(self.device)
        if getattr(self, "_done_ids", None) is None:
            self._done_ids = torch.full((E + 1,), -1, dtype=torch.int32, device=self.device)
        L.check(self._post.lib.emloco_task_compact_done(C.c_void_p(self.reset_buf.data_ptr()), E, C.c_void_p(self._done_ids.data_ptr()),
                                                        current_stream_handle(dev)), "emloco_task_compact_done")
        self._getup_reset(self._done_ids, E, rnd=rnd, split_rnd=split_rnd, seeded_rows=True)

    def post_physics_step(self):
        super().post_physics_step()             # the post-physics launch; extras hold the flag tensors, nothing has read them yet
        if torch.device(self.device).type == "cuda":
            from ...sim import current_stream_handle
            self._getup_ready()
            L.check(self._post.lib.emloco_getup_flags(C.byref(self._getup_bufs), current_stream_handle(torch.device(self.device))),
                    "emloco_getup_flags")
        else:
            self._update_recovery_count()
            self._hold_recovering_envs()

    def getup_epoch_stats(self):
        """The epoch's reset mix and mean recovery counter from the sums the kernels keep on the device (one read, then cleared):
        shares of recovery / fall / normal resets, the mean of recovery_counter over envs and steps, the share of env-steps held back."""
        s = self._getup_stats.tolist()
        self._getup_stats.zero_()
        resets = s[L.GETUP_STAT_RECOVER] + s[L.GETUP_STAT_FALL] + s[L.GETUP_STAT_NORMAL]
        env_steps = max(s[L.GETUP_STAT_FLAG_CALLS] * self.num_envs, 1)
        share = lambda k: s[k] / resets if resets else 0.0
        return dict(getup_resets=resets, getup_recovery_share=share(L.GETUP_STAT_RECOVER), getup_fall_share=share(L.GETUP_STAT_FALL),
                    getup_normal_share=share(L.GETUP_STAT_NORMAL), getup_mean_recovery_counter=s[L.GETUP_STAT_COUNTER_SUM] / env_steps,
                    getup_held_share=s[L.GETUP_STAT_HELD] / env_steps)

    # ------------------------------------------------------------------ host path (fused_reset off): the same structure in torch
    def _reset_actors(self, env_ids):                     # :122-154
        env_ids = torch.as_tensor(env_ids, device=self.device).long()
        held = self._fall_assign[env_ids]
        self._fall_taken[held[held >= 0].long()] = 0
        self._fall_assign[env_ids] = -1
        u = torch.rand((env_ids.shape[0], 2), device=self.device)
        recovery = (u[:, 0] < self._recovery_episode_prob) & (self._terminate_buf[env_ids] == 1)
        fall = ~recovery & (u[:, 1] < self._fall_init_prob)
        fall_ids = env_ids[fall]
        self._getup_calls += 1
        key = (int(torch.initial_seed()) * 0x9E3779B1 + self._getup_calls) & 0xFFFFFFFF
        P = self.num_envs
        taken = self._fall_taken.cpu()
        free = [s for s in (L.real_pick_perm(k, P, key) for k in range(P)) if taken[s] == 0][:len(fall_ids)]
        fall_ids, surplus = fall_ids[:len(free)], fall_ids[len(free):]
        recovery_ids = env_ids[recovery]
        self._recovery_counter[recovery_ids] = self._recovery_steps
        self._reset_fall_env_ids = []
        if len(fall_ids) > 0:                             # _reset_fall_episode :160-174
            slots = torch.tensor(free, device=self.device, dtype=torch.long)
            self._humanoid_root_states[fall_ids] = self._fall_root_states[slots]
            self._dof_state.view(self.num_envs, -1, 2)[fall_ids, :self.num_dof] = self._fall_dof_state[slots]
            self._recovery_counter[fall_ids] = self._recovery_steps
            self._fall_taken[slots] = 1
            self._fall_assign[fall_ids] = slots.to(torch.int32)
            self._reset_fall_env_ids = fall_ids
        normal_ids = torch.cat([env_ids[~recovery & ~fall], surplus])
        if len(normal_ids) > 0:
            super()._reset_actors(normal_ids)
            self._recovery_counter[normal_ids] = 0
        s = self._getup_stats
        s[L.GETUP_STAT_RECOVER] += len(recovery_ids)
        s[L.GETUP_STAT_FALL] += len(fall_ids)
        s[L.GETUP_STAT_NORMAL] += len(normal_ids)

    def _reset_envs(self, env_ids):                       # :176-181
        self._reset_fall_env_ids = []
        super()._reset_envs(env_ids)

    def _init_amp_obs(self, env_ids):                     # :183-189
        super()._init_amp_obs(env_ids)
        if len(self._reset_fall_env_ids) > 0:
            self._init_amp_obs_default(self._reset_fall_env_ids)

    def _update_recovery_count(self):                     # :191-194
        self._recovery_counter.sub_(1).clamp_(min=0)

    def _hold_recovering_envs(self):                      # _compute_reset :199-203
        is_recovery = self._recovery_counter > 0
        self.reset_buf[is_recovery] = 0
        self._terminate_buf[is_recovery] = 0
        self.progress_buf[is_recovery] -= 1

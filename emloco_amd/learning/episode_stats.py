"""Game statistics of a training run, kept on the device: what rl_games' `game_rewards` / `game_lengths` meters give the reference's
loops (amp_continuous_value.py:94-101, amp_continuous.py:153-154, common_agent.py:399-400) and what the per-epoch line of
CommonAgent.train prints from them (common_agent.py:199-201,236-238), plus the health values the soak script read (fastest body,
non-finite states, why the games end).

`EpisodeStats.step()` is one HIP launch per env step (`emloco_episode_stats_step`, csrc/episode_stats_kernels.hip) on the caller's
stream, behind `env.step(...)` and ahead of the next `reset_done()` / `reset`: at that point the step's rewards, flags, progress, body
states and paths are in place and no finished env has been reset.  `end_epoch()` is one launch (`emloco_episode_stats_reduce`), ONE read of
the moment vector and ONE collective across ranks; the host reads nothing in between.

The means are over the games that FINISHED IN THE EPOCH.  rl_games' `AverageMeter` is a capped running window over about the last 100
games, whatever epoch they ended in; rl_games is not vendored, its exact arithmetic cannot be pinned here, and the two numbers are not
to be compared as equals: an epoch with many games is averaged over all of them, an epoch with none reports `games: 0` and no mean.

The numpy restatement of the whole bookkeeping lives with the tests (tests/episode_stats_ref.py)."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib as L

# the moment vector of emloco_episode_stats_reduce (EMLOCO_EPISODE_MOMENTS doubles, include/emloco_task.h: EMLOCO_EPM_*)
MOMENT_NAMES = ("games", "timeout", "far", "fallen", "sum_len", "sum_len2", "min_len", "max_len", "sum_ret", "sum_ret2", "sum_loc",
                "sum_pow", "nonfinite_steps", "max_speed2", "max_ang_speed2")
MOMENT_OPS = tuple("min" if n == "min_len" else "max" if n.startswith("max_") else "sum" for n in MOMENT_NAMES)
RUNNING_NAMES = ("ret", "loc", "pow", "len")                 # the float32 running values of a game in progress
CAUSES = ("runs", "timeout", "far", "fallen")                # EMLOCO_EPISODE_*
assert len(MOMENT_NAMES) == L.EPISODE_MOMENTS and len(RUNNING_NAMES) == L.EPISODE_RUNNING


def merge_moments(*vectors):
    """The moment vector of several shards' games together (ranks, or parts of an env range): sums added, extrema folded.  The minimum
    length of a shard without games (it carries 0) does not take part."""
    vs = [np.asarray(v, np.float64) for v in vectors]
    out = np.zeros(len(MOMENT_NAMES), np.float64)
    for k, op in enumerate(MOMENT_OPS):
        if op == "sum":
            out[k] = sum(float(v[k]) for v in vs)
        elif op == "max":
            out[k] = max(float(v[k]) for v in vs)
        else:
            played = [float(v[k]) for v in vs if v[0] > 0]
            out[k] = min(played) if played else 0.0
    return out


def report_from_moments(m):
    """The epoch's report from its moment vector: a dict of plain floats / ints.  With no finished game: `games: 0` and none of the
    means (nothing is divided); the health values are there either way."""
    m = dict(zip(MOMENT_NAMES, (float(x) for x in m)))
    n = int(round(m["games"]))
    out = {"games": n}
    if n > 0:
        mean_len, mean_ret = m["sum_len"] / n, m["sum_ret"] / n
        out.update(timeout=m["timeout"] / n, far=m["far"] / n, fallen=m["fallen"] / n,
                   len_mean=mean_len, len_std=math.sqrt(max(m["sum_len2"] / n - mean_len * mean_len, 0.0)),
                   len_min=m["min_len"], len_max=m["max_len"],
                   ret_mean=mean_ret, ret_std=math.sqrt(max(m["sum_ret2"] / n - mean_ret * mean_ret, 0.0)),
                   ret_loc_mean=m["sum_loc"] / n, ret_pow_mean=m["sum_pow"] / n)
    out.update(max_speed=math.sqrt(m["max_speed2"]), max_ang_speed=math.sqrt(m["max_ang_speed2"]),
               nonfinite_steps=int(round(m["nonfinite_steps"])))
    return out


class EpisodeStats:
    """Owns the per-env buffers; `task` is the env's task object (its fused post-physics buffers name every input).  `inverted_penalty`:
    the scale of the LocoVal loop's heading-inversion penalty (amp_continuous_value.py:63-64), or None -- the policy trainer -- for the
    rewards as they are."""

    def __init__(self, task, inverted_penalty=None, game_out=False):
        self.task = task
        self.device = torch.device(task.device)
        if self.device.type != "cuda":
            raise RuntimeError("EpisodeStats keeps its books in HIP kernels: it needs libemloco_hip.so and a gfx950 device")
        self.lib = L.require_device()
        self.num_envs = E = int(task.num_envs)
        bufs = task._post_bufs if getattr(task, "_post_bufs", None) is not None else task._ensure_post_bufs()
        if int(bufs.n_env) != E:
            raise RuntimeError("EpisodeStats: the task's post-physics buffers are for another env count")
        self._bufs = bufs                                     # the addresses the post-physics kernel itself reads and writes
        self.inverted_penalty = None if inverted_penalty is None else float(inverted_penalty)
        self.running = torch.zeros(E, L.EPISODE_RUNNING, device=self.device)
        self.totals = torch.zeros(E, L.EPISODE_MOMENTS, dtype=torch.float64, device=self.device)
        self.moments = torch.zeros(L.EPISODE_MOMENTS, dtype=torch.float64, device=self.device)
        self.game_out = torch.zeros(E, L.EPISODE_GAME_OUT, device=self.device) if game_out else None
        self._inv_keep = None
        self.last_extra = None

    def step(self):
        from ..sim import current_stream_handle
        b, inv = self._bufs, None
        if self.inverted_penalty is not None:
            inv = getattr(self.task, "inverted", None)
            if isinstance(inv, torch.Tensor):
                inv = (inv.view(torch.uint8) if inv.dtype == torch.bool else inv.to(torch.uint8)).contiguous()
                if inv.numel() != self.num_envs:
                    raise RuntimeError("EpisodeStats: task.inverted has another length than the env count")
            else:
                inv = None
        self._inv_keep = inv
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        a = lambda x: C.c_void_p(x) if x else None
        L.check(self.lib.emloco_episode_stats_step(
            self.num_envs, a(b.rew_buf), a(b.reward_raw), a(b.reset_buf), a(b.terminate_buf), a(b.progress_buf), a(b.rb_state),
            a(b.traj_verts), p(inv), float(self.inverted_penalty or 0.0), float(b.dt), float(b.traj_dur), float(b.fail_dist),
            p(self.running), p(self.totals), p(self.game_out), current_stream_handle(self.device)), "emloco_episode_stats_step")

    def reduce(self):
        """The reduce launch alone: `self.moments` (device) holds this rank's vector afterwards, the per-env totals are cleared."""
        from ..sim import current_stream_handle
        L.check(self.lib.emloco_episode_stats_reduce(self.num_envs, C.c_void_p(self.totals.data_ptr()), C.c_void_p(self.moments.data_ptr()),
                                                     current_stream_handle(self.device)), "emloco_episode_stats_reduce")
        return self.moments

    def end_epoch(self, extra=None):
        """Reduce, read once, exchange once across ranks, report.  `extra`: a device float64 vector of this rank's SUMS that the caller
        wants to ride along (read and exchanged with the moments); the global sums are left in `self.last_extra`."""
        from ..dist import all_gather_vector
        m = self.reduce()
        n = m.numel()
        if extra is not None:
            m = torch.cat([m, extra.to(torch.float64).reshape(-1)])
        parts = all_gather_vector(m)                          # the one read (and, on several ranks, the one collective)
        self.last_moments = merge_moments(*[v[:n] for v in parts])
        self.last_extra = None if extra is None else np.sum([v[n:] for v in parts], axis=0)
        return report_from_moments(self.last_moments)

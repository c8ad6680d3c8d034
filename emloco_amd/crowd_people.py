"""Python side of the group observation (include/emloco_task.h: EmlocoCrowdPeople, emloco_task_crowd_people).

With `group_obs: True` and `divide_group: True` every env's task observation ends in a 165-wide `people` block: the ten selected joints
and the root velocity of the five nearest members of its group, in the env's heading frame, zeros for a neighbour farther than 10 m.
Reference: humanoid_pedestrain_terrain.py:312-335,444-450,481-484 and compute_group_observation :1613-1666; the two departures (ties
by member index, the mirrored block at its own columns) are stated in the header.

`CrowdPeople` owns what the kernels need beyond the task's tensors: the packed root workspace and, on request, the neighbour table.
The kernels run on torch's current stream.
"""
import ctypes as C

import torch

from . import _lib as L

WIDTH, TOPK = L.PEOPLE_WIDTH, L.PEOPLE_TOPK
MIN_GROUP = TOPK + 1


class CrowdPeopleError(L.EmlocoError):
    pass


def config_block(env_cfg):
    """Whether cfg["env"] switches the `people` block on: group_obs with divide_group, and not disable_group_obs (humanoid.py:223,
    humanoid_pedestrain_terrain.py:312,792).  group_obs without divide_group adds nothing, as in the reference."""
    return bool(env_cfg.get("group_obs", False) and env_cfg.get("divide_group", False) and not env_cfg.get("disable_group_obs", False))


def group_refusal(group_size):
    """Why a group of this size cannot carry the block, or None"""
    if group_size < MIN_GROUP:
        return (f"group_obs: the people block holds the {TOPK} nearest OTHER members of an env's group, and num_env_group gives groups of "
                f"{group_size}: a group needs at least {MIN_GROUP} members (the reference's topk({MIN_GROUP}) fails there too)")
    return None


class CrowdPeople:
    def __init__(self, *, rb_state, n_env, group_size, obs, flip_obs, col, neighbours=False):
        L.require_device()
        from .sim import dptr
        self.lib = L.load()
        why = group_refusal(int(group_size))
        if why:
            raise CrowdPeopleError(why)
        assert obs.is_contiguous() and flip_obs.is_contiguous() and obs.shape == flip_obs.shape and obs.dtype == torch.float32
        assert rb_state.is_contiguous() and rb_state.dtype == torch.float32 and rb_state.numel() == int(n_env) * L.NB * 13
        dev = rb_state.device
        self.device, self.n_env, self.group_size, self.col = dev, int(n_env), int(group_size), int(col)
        self.roots_ws = torch.zeros(self.n_env * 4, dtype=torch.float32, device=dev)
        self.neighbours = torch.full((self.n_env, TOPK), -1, dtype=torch.int32, device=dev) if neighbours else None
        self._keep = (rb_state, obs, flip_obs)
        p = lambda t: None if t is None else dptr(t).value
        self.bufs = L.CrowdPeople(self.n_env, self.group_size, int(obs.shape[1]), self.col, p(rb_state), p(self.roots_ws), p(obs), p(flip_obs),
                                  p(self.neighbours))

    def run(self, env_ids=None):
        """The block of every env, or of the envs of an int32 id list on the device (-1 entries are skipped)."""
        from .sim import current_stream_handle, dptr
        n = 0 if env_ids is None else int(env_ids.numel())
        if env_ids is not None and n == 0:
            return
        rc = self.lib.emloco_task_crowd_people(C.byref(self.bufs), dptr(env_ids), n, current_stream_handle(self.device))
        L.check(rc, "emloco_task_crowd_people")

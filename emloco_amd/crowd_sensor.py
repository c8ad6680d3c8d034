"""Python side of the crowd-aware terrain sensor (include/emloco_task.h: EmlocoCrowdBufs, emloco_task_crowd_sensor).

The members of a group of envs see each other on the height map: every env stamps the cells under its 10 x 20 root points into the
owner map of its group, and the res x res probes around the head read the stamped height (channel 0) and, with the velocity map, the
relative velocity of whoever stands on the cell (channels 1, 2).  Reference: pacer_group_cnn.yaml (divide_group, num_env_group,
velocity_map, sensor_res, sensor_extent), humanoid_pedestrain_terrain.py:400-452,761-815,1212-1297.

`CrowdSensor` owns what the kernels need beyond the task's tensors: the owner map, its epoch tag and the coordinate tables.  The
kernels run on torch's current stream.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

ROOT_POINTS = L.CROWD_ROOT_X * L.CROWD_ROOT_Y


class CrowdSensorError(L.EmlocoError):
    pass


def probe_table(res, extent):
    """float32(np.linspace(-extent, extent, res)) (:650-668): the x and the y coordinates of the probe grid"""
    return np.linspace(-extent, extent, res).astype(np.float32)


def root_tables():
    """the x (10) and y (20) coordinates of the root points (:685-702)"""
    return np.linspace(-0.25, 0.25, L.CROWD_ROOT_X).astype(np.float32), np.linspace(-0.5, 0.5, L.CROWD_ROOT_Y).astype(np.float32)


def stamp_units(vscale):
    """torch.tensor(1.7 / vertical_scale).short() (:1247): the quotient in double precision, held as float32, truncated, wrapped to int16"""
    v = int(np.float32(1.7 / float(vscale)))
    return ((v + 32768) % 65536) - 32768


def group_layout(n_env, num_env_group):
    """(group_size, n_groups) of humanoid.py:221-226; the reference's np.arange(float).repeat breaks silently when n_env is no multiple"""
    group_size = min(int(num_env_group), int(n_env))
    if group_size < 1 or n_env % group_size != 0:
        raise CrowdSensorError(f"num_env_group: numEnvs ({n_env}) is not a multiple of the group size ({group_size}); under several "
                               "ranks the groups are formed inside each rank's share of the envs")
    return group_size, n_env // group_size


def is_crowd_config(env_cfg):
    """whether cfg["env"] departs from the 32 x 32, +-2 m, one-channel height grid without groups (pacer.yaml)"""
    return bool(env_cfg.get("divide_group", False) or env_cfg.get("velocity_map", False) or env_cfg.get("sensor_res", 32) != 32
                or float(env_cfg.get("sensor_extent", 2)) != 2.0)


class EpochTag:
    """The tag in the high bits of an owner word.  A call's stamps carry a tag above every earlier call's, so atomicMax lets them beat
    what the map still holds and the map is not cleared between calls; when the tag would overflow the caller clears the map and the
    count starts over at 1 (0 is the cleared map)."""

    def __init__(self, group_size):
        self.shift = max(1, int(group_size * ROOT_POINTS).bit_length())       # group_size * 200 < 2^shift
        if self.shift > 30:
            raise CrowdSensorError(f"num_env_group: a group of {group_size} envs leaves no room for the owner map's tag")
        self.last = (1 << (32 - self.shift)) - 1
        self.tag = 0

    def advance(self):
        """(tag of the next call, whether the map must be cleared first)"""
        clear = self.tag >= self.last
        self.tag = 1 if clear else self.tag + 1
        return self.tag, clear


class CrowdSensor:
    def __init__(self, *, rb_state, heightfield, hscale, vscale, head_body, n_env, num_env_group, stamps, velocity_map, res, extent,
                 obs, flip_obs, src_obs=None, src_flip_obs=None, n_copy=0):
        L.require_device()
        from .sim import dptr
        self.lib = L.load()
        if not 1 <= int(res) <= L.CROWD_MAX_RES:
            raise CrowdSensorError(f"sensor_res {res} outside 1 .. {L.CROWD_MAX_RES}")
        dev = rb_state.device
        self.device = dev
        self.n_env, self.res, self.channels, self.stamps = int(n_env), int(res), 3 if velocity_map else 1, bool(stamps)
        self.group_size, self.n_groups = group_layout(n_env, num_env_group) if stamps else (int(n_env), 1)
        assert heightfield.dtype == torch.int16 and heightfield.dim() == 2 and heightfield.is_contiguous()
        assert obs.is_contiguous() and flip_obs.is_contiguous() and obs.shape == flip_obs.shape and rb_state.is_contiguous()
        rx, ry = root_tables()
        self.probe_xy = torch.from_numpy(probe_table(res, extent)).to(dev)
        self.root_x, self.root_y = torch.from_numpy(rx).to(dev), torch.from_numpy(ry).to(dev)
        self.epoch = EpochTag(self.group_size)
        self.owner = None
        self.owner_bytes = 0
        if self.stamps:
            cells = int(heightfield.shape[0]) * int(heightfield.shape[1])
            self.owner_bytes = 4 * self.n_groups * cells
            print(f"crowd sensor: owner map of {self.n_groups} groups x {heightfield.shape[0]} x {heightfield.shape[1]} cells, {self.owner_bytes} bytes")
            try:
                self.owner = torch.zeros(self.n_groups * cells, dtype=torch.int32, device=dev)
            except RuntimeError as e:          # torch.cuda.OutOfMemoryError is one
                raise CrowdSensorError(f"crowd sensor: the owner map of {self.n_groups} groups x {heightfield.shape[0]} x {heightfield.shape[1]} "
                                       f"cells ({self.owner_bytes} bytes) could not be allocated: {e}") from e
        self._keep = (rb_state, heightfield, obs, flip_obs, src_obs, src_flip_obs)
        p = lambda t: None if t is None else dptr(t).value
        self.bufs = L.CrowdBufs(self.n_env, self.group_size, int(heightfield.shape[0]), int(heightfield.shape[1]), int(head_body),
                                self.res, self.channels, int(self.stamps), stamp_units(vscale),
                                0 if src_obs is None else int(src_obs.shape[1]), int(obs.shape[1]), int(n_copy), self.epoch.shift, 0,
                                float(hscale), float(vscale), p(rb_state), p(heightfield), p(self.probe_xy), p(self.root_x), p(self.root_y),
                                p(self.owner), p(src_obs), p(src_flip_obs), p(obs), p(flip_obs))

    def run(self, env_ids=None):
        """Stamps of all envs, then the rows of every env, or of the envs of an int32 id list on the device (-1 entries are skipped)."""
        from .sim import current_stream_handle, dptr
        n = 0 if env_ids is None else int(env_ids.numel())
        if env_ids is not None and n == 0:
            return
        if self.stamps:
            self.bufs.tag, clear = self.epoch.advance()
            if clear:
                self.owner.zero_()
        rc = self.lib.emloco_task_crowd_sensor(C.byref(self.bufs), dptr(env_ids), n, current_stream_handle(self.device))
        L.check(rc, "emloco_task_crowd_sensor")

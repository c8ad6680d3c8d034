"""CPU execution of emloco_amd/csrc/crowd_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_crowd.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_crowd.so, a library of its own.

`EmuBackend` and `DeviceBackend` (tests/test_gpu_crowd.py) share `CrowdHost`: the sensor's buffers as host arrays with guard words
around every one the kernels write, the epoch tag of the product (emloco_amd.crowd_sensor.EpochTag), one `run(rb, env_ids)`."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_crowd.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crowd_sensor.npz")


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_crowd.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(_ROOT, "emloco_amd", "csrc", f) for f in ("crowd_kernels.hip", "task_device.h", "dev_math.h", "locoval_returns_device.h")]
    deps += [os.path.join(_ROOT, "include", h) for h in ("emloco_task.h", "emloco_sim.h")]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_crowd.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_crowd_sensor.argtypes, _lib.emu_crowd_sensor.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int], C.c_int
        _lib.emu_crowd_error.restype = C.c_char_p
    return _lib


def guarded(n_words, dtype=np.uint32):
    """(whole, view): `view` is n_words zeros of a 4-byte dtype with at least GUARD words of FILL on either side inside `whole`"""
    whole = np.full(n_words + 2 * GUARD, FILL, np.uint32)
    view = whole[GUARD:GUARD + n_words]
    view[:] = 0
    return whole, view.view(dtype)


def guards_intact(whole):
    return bool((whole[:GUARD] == FILL).all() and (whole[-GUARD:] == FILL).all())


def fixtures():
    z = np.load(GOLDEN)
    return z, [str(c) for c in z["cases"]]


def rb_states(n_env, rng, centres, spread=0.6, clear=None):
    """body states [E][24][13] with a root (body 0) and a head (body 13) per env, the members of a group around its centre;
    `clear` = (res, extent): every env is redrawn until crowd_ref.clear_of_boundaries holds for that probe grid"""
    import crowd_ref
    rb = np.zeros((n_env, 24, 13), np.float32)
    rb[:, :, 6] = 1
    for e in range(n_env):
        while True:
            xy = np.asarray(centres[e]) + rng.uniform(-spread, spread, 2)
            yaw = rng.uniform(-np.pi, np.pi)
            rb[e, 0, :3] = [xy[0], xy[1], 0.9]
            rb[e, 0, 3:7] = [0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]
            rb[e, 0, 7:10] = rng.uniform(-1.5, 1.5, 3)
            rb[e, 13, :3] = [xy[0] + 0.05, xy[1] - 0.03, 1.5]
            yh = yaw + rng.uniform(-0.4, 0.4)
            rb[e, 13, 3:7] = [0, 0, np.sin(yh / 2), np.cos(yh / 2)]
            if clear is None or crowd_ref.clear_of_boundaries(rb[e], 13, clear[0], clear[1], 0.1):
                break
    return rb


class CrowdHost:
    """The sensor's buffers on the host.  `launch(bufs, ids, n)` of the subclass runs the two kernels."""

    def __init__(self, n_env, heightfield, hscale, vscale, res, extent, channels, stamps, group_size, head_body=13, src_width=0, n_copy=0,
                 dst_pad=0):
        from emloco_amd import _lib as L, crowd_sensor as S
        self.L, self.S = L, S
        self.E, self.res, self.C, self.stamps, self.gs = n_env, res, channels, bool(stamps), group_size
        self.hf = np.ascontiguousarray(heightfield, np.int16)
        self.block = channels * res * res
        self.width = n_copy + self.block + dst_pad
        self.n_copy = n_copy
        self.rb = np.zeros((n_env, 24, 13), np.float32)
        self.probe_xy = S.probe_table(res, extent)
        self.root_x, self.root_y = S.root_tables()
        self.epoch = S.EpochTag(group_size)
        self._obs_whole, obs = guarded(n_env * self.width, np.float32)
        self._flip_whole, flip = guarded(n_env * self.width, np.float32)
        self.obs, self.flip = obs.reshape(n_env, self.width), flip.reshape(n_env, self.width)
        cells = self.hf.shape[0] * self.hf.shape[1]
        self._owner_whole, self.owner = guarded((n_env // group_size) * cells if stamps else 1)
        self.src = np.zeros((n_env, max(src_width, 1)), np.float32)
        self.src_flip = np.zeros((n_env, max(src_width, 1)), np.float32)
        p = lambda a: a.ctypes.data
        self.bufs = L.CrowdBufs(n_env, group_size, self.hf.shape[0], self.hf.shape[1], head_body, res, channels, int(self.stamps),
                                S.stamp_units(vscale), src_width, self.width, n_copy, self.epoch.shift, 0, hscale, vscale,
                                p(self.rb), p(self.hf), p(self.probe_xy), p(self.root_x), p(self.root_y), p(self.owner),
                                p(self.src) if n_copy else None, p(self.src_flip) if n_copy else None, p(self.obs), p(self.flip))

    def run(self, rb, env_ids=None, **kw):
        """one call of the sensor on the state `rb`; returns (rows, mirrored rows) of the sensor block, all envs"""
        np.copyto(self.rb, np.asarray(rb, np.float32).reshape(self.rb.shape))
        if self.stamps:
            self.bufs.tag, clear = self.epoch.advance()
            if clear:
                self.owner[:] = 0
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
        self.launch(ids, 0 if ids is None else len(ids), **kw)
        at = self.n_copy
        return self.obs[:, at:at + self.block].copy(), self.flip[:, at:at + self.block].copy()

    def guards(self):
        return all(guards_intact(w) for w in (self._obs_whole, self._flip_whole, self._owner_whole))


class EmuBackend(CrowdHost):
    def launch(self, ids, n, grid=0):
        rc = lib().emu_crowd_sensor(C.addressof(self.bufs), None if ids is None else ids.ctypes.data, n, grid)
        assert rc == 0, lib().emu_crowd_error()

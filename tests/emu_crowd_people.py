"""CPU execution of emloco_amd/csrc/crowd_people_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_crowd_people.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_crowd_people.so, a library of its own.

`EmuBackend` and `DeviceBackend` (tests/test_gpu_crowd_people.py) share `PeopleHost`: the observation rows as host arrays with guard
words around both, the neighbour table, and the one entry point of include/emloco_task.h.  `people_f64` is the float64 restatement of
the header's rule (ties by member index) that both test files compare against; `CASES` are the shapes the fixture cannot reach."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_crowd_people.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5
TOPK, WIDTH, FAR = 5, 165, 10.0
BODIES = (0, 1, 5, 9, 3, 7, 16, 21, 18, 23)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crowd_people.npz")
# worst |reference fp32 - float64 restatement| on the committed fixture (both cases, both rows), measured when the fixture was made
# (tests/golden/gen_golden_crowd_people.py prints it; test_crowd_people_cpu.py re-measures it), and the bar: four times that
REF_ERR = 1.3099935e-06
BAR = 4 * REF_ERR


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_crowd_people.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(_ROOT, "emloco_amd", "csrc", f) for f in ("crowd_people_kernels.hip", "dev_math.h")]
    deps += [os.path.join(_ROOT, "include", "emloco_task.h")]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_crowd_people.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_crowd_people.argtypes, _lib.emu_crowd_people.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int], C.c_int
        _lib.emu_crowd_people_error.restype = C.c_char_p
    return _lib


def guarded(n_words):
    """(whole, view): `view` is n_words 32-bit words with GUARD words of FILL on either side inside `whole`"""
    whole = np.full(n_words + 2 * GUARD, FILL, np.uint32)
    return whole, whole[GUARD:GUARD + n_words]


class PeopleHost:
    """The buffers of one EmlocoCrowdPeople on the host.  obs / flip_obs start as a known pattern (`prefill`), so a byte written outside
    the block shows.  The subclass gives `ptr(name)`, `sync_in` / `sync_out` and `_call`."""
    WRITTEN = ("roots_ws", "obs", "flip_obs", "neighbours")

    def __init__(self, n_env, group_size, obs_stride=WIDTH + 11, col=7, neighbours=True):
        from emloco_amd import _lib as L
        self.L = L
        self.E, self.gs, self.stride, self.col, self.with_nb = n_env, group_size, obs_stride, col, neighbours
        self.inputs = dict(rb_state=np.zeros((n_env, 24, 13), np.float32))
        words = dict(roots_ws=n_env * 4, obs=n_env * obs_stride, flip_obs=n_env * obs_stride, neighbours=n_env * TOPK)
        self.whole, self.view = {}, {}
        for name in self.WRITTEN:
            self.whole[name], self.view[name] = guarded(words[name])
        self.prefill()

    def prefill(self):
        self.view["roots_ws"][:] = 0
        self.view["neighbours"][:] = 0xFFFFFFFF
        for k, name in enumerate(("obs", "flip_obs")):
            self.view[name].view(np.float32)[:] = 1000.0 * (k + 1) + np.arange(self.E * self.stride, dtype=np.float32) % 977

    def struct(self):
        p = self.ptr
        return self.L.CrowdPeople(self.E, self.gs, self.stride, self.col, p("rb_state"), p("roots_ws"), p("obs"), p("flip_obs"),
                                  p("neighbours") if self.with_nb else None)

    def run(self, rb, env_ids=None, **kw):
        """the call on state `rb`; env_ids: None or a list"""
        np.copyto(self.inputs["rb_state"], np.asarray(rb, np.float32).reshape(self.E, 24, 13))
        self.inputs["env_ids"] = np.ascontiguousarray([] if env_ids is None else env_ids, np.int32)
        self.sync_in()
        self._call(self.struct(), None if env_ids is None else self.ptr("env_ids"), 0 if env_ids is None else len(env_ids), **kw)
        self.sync_out()
        return self

    def rows(self, name="obs"):
        """[E][obs_stride] float32 (a copy)"""
        return self.view[name].view(np.float32).reshape(self.E, self.stride).copy()

    def block(self, name="obs"):
        return self.rows(name)[:, self.col:self.col + WIDTH]

    def neighbours(self):
        return self.view["neighbours"].view(np.int32).reshape(self.E, TOPK).copy()

    def guards(self):
        return all(bool((w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all()) for w in self.whole.values())

    def written_bytes(self):
        return b"".join(self.view[n].tobytes() for n in ("obs", "flip_obs", "neighbours"))


class EmuBackend(PeopleHost):
    def ptr(self, name):
        return (self.view[name] if name in self.view else self.inputs[name]).ctypes.data

    def sync_in(self):
        pass

    def sync_out(self):
        pass

    def _call(self, s, ids, n, grid=0):
        rc = lib().emu_crowd_people(C.addressof(s), ids, n, grid)
        assert rc == 0, lib().emu_crowd_people_error()


def emu_refusal(s, n=0):
    """the name under which the emulated entry point refuses the structure `s` (or None for a NULL one), '' if it does not"""
    rc = lib().emu_crowd_people(None if s is None else C.addressof(s), None, n, 0)
    return lib().emu_crowd_people_error().decode() if rc != 0 else ""


# ---------------------------------------------------------------------------------------------- float64 restatement
def heading_inv_f64(q):
    """calc_heading_quat_inv in float64: xyzw of the rotation by -heading about z; q [E][4] xyzw"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    # my_quat_rotate(q, ex): the x and y components
    rx = (2.0 * w * w - 1.0) + 2.0 * x * x
    ry = 2.0 * w * z + 2.0 * x * y
    h = np.arctan2(ry, rx)
    out = np.zeros_like(q)
    out[:, 2], out[:, 3] = np.sin(-h / 2), np.cos(-h / 2)
    return out


def quat_rotate_f64(q, v):
    """my_quat_rotate in float64; q [..., 4] xyzw, v [..., 3]"""
    qv, w = q[..., :3], q[..., 3:4]
    return v * (2.0 * w * w - 1.0) + np.cross(qv, v) * w * 2.0 + qv * np.sum(qv * v, -1, keepdims=True) * 2.0


def people_f64(rb, group_size):
    """(rows [E][165], mirrored rows, neighbours [E][5] int32) of the header's rule in float64 on the float32 state `rb` [E][24][13]:
    the distances are formed from the float32 coordinates in float64, a non-finite one counts as +inf, and equal distances are ordered
    by member index."""
    rb = np.asarray(rb, np.float32).reshape(-1, 24, 13).astype(np.float64)
    E = rb.shape[0]
    root = rb[:, 0, :3]
    hinv = heading_inv_f64(rb[:, 0, 3:7])
    rows, nbs = np.zeros((E, WIDTH)), np.zeros((E, TOPK), np.int32)
    for e in range(E):
        g0 = (e // group_size) * group_size
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.sqrt(((root[g0:g0 + group_size] - root[e]) ** 2).sum(-1))
        d[~np.isfinite(d)] = np.inf
        order = [m for m in np.lexsort((np.arange(group_size), d)) if g0 + m != e][:TOPK]
        for k, m in enumerate(order):
            nbs[e, k] = g0 + m
            if d[m] > FAR:
                continue
            pos = rb[g0 + m][list(BODIES), :3] - root[e]
            rows[e, 30 * k:30 * k + 30] = quat_rotate_f64(hinv[e], pos).reshape(-1)
            rows[e, 150 + 3 * k:153 + 3 * k] = quat_rotate_f64(hinv[e], rb[g0 + m, 0, 7:10])
    flip = rows.copy()
    flip[:, 1::3] *= -1
    return rows, flip, nbs


# ---------------------------------------------------------------------------------------------- shapes the fixture cannot reach
def random_state(rng, n_env, group_size, spread=6.0):
    """a crowd: every group scattered over `spread` metres about its own centre, tilted roots, bodies about the root"""
    rb = np.zeros((n_env, 24, 13), np.float32)
    for e in range(n_env):
        g = e // group_size
        root = np.array([20.0 + 3.0 * g, 15.0, 0.9]) + rng.uniform(-1, 1, 3) * [spread, spread, 0.05]
        rb[e, :, :3] = root + rng.uniform(-0.9, 0.9, (24, 3))
        rb[e, 0, :3] = root
        q = rng.normal(size=(24, 4)) * [0.1, 0.1, 1.0, 1.0]
        rb[e, :, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        rb[e, :, 7:13] = rng.uniform(-1.5, 1.5, (24, 6))
    return rb


def case_ragged():
    """130 envs in groups of 65: more than one member per lane and a ragged last round"""
    return random_state(np.random.default_rng(11), 130, 65, spread=9.0), 65


def case_all_equal():
    """all roots equal: every env gets the five lowest indices other than its own"""
    rb = random_state(np.random.default_rng(12), 24, 12)
    rb[:, 0, :3] = np.float32([21.5, 14.25, 0.93])
    return rb, 12


def case_nan_root():
    """one NaN root (env 3): never chosen ahead of a finite member; in its own group of 6 it is chosen by everyone, masked"""
    rb = random_state(np.random.default_rng(13), 18, 6, spread=2.0)
    rb[3, 0, 0] = np.nan
    return rb, 6


CASES = {"ragged": case_ragged, "all_equal": case_all_equal, "nan_root": case_nan_root}
ID_LIST = [9, -1, 0, 3]


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}

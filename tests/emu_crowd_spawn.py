"""CPU execution of emloco_amd/csrc/crowd_spawn_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_crowd_spawn.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_crowd_spawn.so, a library of its own.

`EmuBackend` and `DeviceBackend` (tests/test_gpu_crowd_spawn.py) share `SpawnHost`: the inputs of one case (tests/crowd_spawn_cases.py)
as host arrays, the three written buffers with guard words around each and a prefilled pattern, and the one entry point of
include/emloco_task.h."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import crowd_spawn_cases as SC

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_crowd_spawn.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_crowd_spawn.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(_ROOT, "emloco_amd", "csrc", "crowd_spawn_kernels.hip"), os.path.join(_ROOT, "include", "emloco_task.h")]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_crowd_spawn.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_crowd_spawn.argtypes, _lib.emu_crowd_spawn.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], C.c_int
        _lib.emu_crowd_spawn_error.restype = C.c_char_p
    return _lib


def guarded(n_words):
    """(whole, view): `view` is n_words 32-bit words with GUARD words of FILL on either side inside `whole`"""
    whole = np.full(n_words + 2 * GUARD, FILL, np.uint32)
    return whole, whole[GUARD:GUARD + n_words]


class SpawnHost:
    """The buffers of one EmlocoCrowdSpawn on the host.  place_xy / info start as a known pattern and mark_ws as -1 (`prefill`), so a
    byte written for an unlisted env shows.  The subclass gives `ptr(name)`, `sync_in` / `sync_out` and `_call`."""
    WRITTEN = ("mark_ws", "place_xy", "info")

    def __init__(self, case):
        from emloco_amd import _lib as L
        self.L, self.case, self.E = L, case, case["n_env"]
        ids = case["ids"]
        self.inputs = dict(roots=np.ascontiguousarray(case["roots"], np.float32), walkable=np.ascontiguousarray(case["walkable"], np.int16),
                           centres=np.ascontiguousarray(case["centres"], np.float32), u=np.ascontiguousarray(case["u"], np.float32),
                           ids=np.ascontiguousarray([] if ids is None else ids, np.int32))
        assert self.inputs["roots"].shape == (self.E, case["root_stride"]) and self.inputs["u"].shape[1:] == (case["tries"], 2)
        assert self.inputs["u"].shape[0] == (self.E if ids is None else len(ids))
        self.whole, self.view = {}, {}
        for name, words in zip(self.WRITTEN, (self.E, 2 * self.E, 4 * self.E)):
            self.whole[name], self.view[name] = guarded(words)
        self.prefill()

    def prefill(self):
        self.view["mark_ws"][:] = 0xFFFFFFFF
        self.view["place_xy"].view(np.float32)[:] = 1000.0 + np.arange(2 * self.E, dtype=np.float32) % 977
        self.view["info"][:] = 0x5A000000 + np.arange(4 * self.E, dtype=np.uint32)

    def struct(self, **over):
        c, p = self.case, self.ptr
        rows, cols = c["walkable"].shape
        fl = lambda k: float(c[k])
        s = self.L.CrowdSpawn(c["n_env"], c["group_size"], c["tries"], c["root_stride"], rows, cols, fl("hscale"), fl("min_x"), fl("max_x"),
                              fl("min_y"), fl("max_y"), fl("extent"), fl("min_dist"), 0, p("roots"), p("walkable"), p("centres"), p("mark_ws"),
                              p("place_xy"), p("info"))
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def run(self):
        self.sync_in()
        ids = self.case["ids"]
        rc = self._call(self.struct(), None if ids is None else self.ptr("ids"), 0 if ids is None else len(ids), self.ptr("u"))
        assert rc == 0, self.error()
        self.sync_out()
        return self

    def place_xy(self):
        return self.view["place_xy"].view(np.float32).reshape(self.E, 2).copy()

    def info(self):
        return self.view["info"].view(SC.INFO).copy()

    def marks(self):
        return self.view["mark_ws"].view(np.int32).copy()

    def guards(self):
        return all(bool((w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all()) for w in self.whole.values())

    def written_bytes(self):
        return b"".join(self.view[n].tobytes() for n in self.WRITTEN)


class EmuBackend(SpawnHost):
    def ptr(self, name):
        return (self.view[name] if name in self.view else self.inputs[name]).ctypes.data

    def sync_in(self):
        pass

    def sync_out(self):
        pass

    def _call(self, s, ids, n, u):
        return lib().emu_crowd_spawn(None if s is None else C.addressof(s), ids, n, u)

    def error(self):
        return lib().emu_crowd_spawn_error().decode()


def check_against_restatement(host):
    """everything test case 9 asks after a call, and the outputs bit for bit against the float32 restatement"""
    fresh = EmuBackend.__new__(EmuBackend)
    fresh.E, fresh.whole, fresh.view = host.E, {}, {}
    for name, words in zip(SpawnHost.WRITTEN, (host.E, 2 * host.E, 4 * host.E)):
        fresh.whole[name], fresh.view[name] = guarded(words)
    fresh.prefill()
    want_xy, want_info = SC.expected_arrays(host.case, fresh.place_xy(), fresh.info())
    assert host.guards(), "guard words"
    assert (host.marks() == -1).all(), "mark_ws is -1 again"
    assert host.place_xy().tobytes() == want_xy.tobytes(), "place_xy: listed rows bit-equal, unlisted rows hold the prefill"
    assert host.info().tobytes() == want_info.tobytes(), "info: listed rows bit-equal, unlisted rows hold the prefill"
    return SC.spawn_f32(host.case)

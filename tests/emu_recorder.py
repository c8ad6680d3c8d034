"""CPU execution of emloco_amd/csrc/recorder_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_recorder.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_recorder.so, a library of its own."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import flight_recorder_ref as R

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_recorder.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_recorder.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps.append(os.path.join(_ROOT, "emloco_amd", "csrc", "recorder_kernels.hip"))
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
                                       "-o", tmp, os.path.join(_HERE, "emu_recorder.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        for f in (_lib.emu_recorder_record, _lib.emu_recorder_check):
            f.argtypes, f.restype = [C.c_void_p, C.c_int], C.c_int
    return _lib


def guarded(n_words):
    """(guards, view): a uint32 array of n_words zeros, 16-byte aligned, with at least GUARD words of FILL on either side"""
    whole = np.full(n_words + 2 * GUARD + 4, FILL, np.uint32)
    off = (-(whole.ctypes.data // 4 + GUARD)) % 4
    view = whole[GUARD + off:GUARD + off + n_words]
    assert view.ctypes.data % 16 == 0
    view[:] = 0
    return (whole[:GUARD + off], whole[GUARD + off + n_words:]), view


class EmuBackend:
    """The recorder's buffers as host arrays and its two entry points on the emulator; the interface of the case tables
    (tests/recorder_cases.py): push(state), record(t), check(t), pull()."""

    def __init__(self, E, R_, C_, cause_mask=31, speed2=0.0, ang2=0.0, early_fall=0, drive_mode=0, grid=0, request=True, state=None):
        """`state`: a state dict whose arrays the recorder reads in place (a simulator's), instead of arrays of its own"""
        from emloco_amd import _lib as L
        self.E, self.R, self.C = E, R_, C_
        self.st = state if state is not None else R.synthetic_state(E, request=request)
        self._ring_whole, self.ring = guarded(E * R_ * R.REC_WORDS)
        self._slots_whole, self.slots = guarded(C_ * R.slot_words(R_))
        self.counters = np.zeros(R.COUNTERS, np.int32)
        self.last = np.full(E, R.NEVER, np.int32)
        self.cause_ws = np.full(E, -1, np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        s = self.st
        self.bufs = L.RecorderBufs(E, R_, C_, drive_mode, 0, cause_mask, early_fall, grid, speed2, ang2,
                                   p(s["root"]), p(s["dof"]), p(s["warm"]), p(s["drive"]), p(s["rb"]), p(s["cf"]), p(s["df"]),
                                   p(s["progress"]), p(s["reset"]), p(s["terminate"]), p(self.ring), p(self.slots), p(self.counters),
                                   p(self.last), p(self.cause_ws), p(s["request"]))
        self.t0 = None

    def push(self, st):
        for k, v in self.st.items():
            if v is not None:
                np.copyto(v, st[k])

    def record(self, t):
        if self.t0 is None:
            self.t0 = self.bufs.t0 = t
        assert lib().emu_recorder_record(C.addressof(self.bufs), t) == 0

    def check(self, t):
        assert lib().emu_recorder_check(C.addressof(self.bufs), t) == 0

    def pull(self):
        whole_ok = all((g == FILL).all() and g.size >= GUARD for gs in (self._ring_whole, self._slots_whole) for g in gs)
        return dict(ring=self.ring.reshape(self.E, self.R, R.REC_WORDS).copy(), slots=self.slots.reshape(self.C, -1).copy(),
                    counters=self.counters.copy(), last=self.last.copy(), guards=whole_ok,
                    request=None if self.st["request"] is None else self.st["request"].copy())

    def drain(self):
        self.counters[:] = 0

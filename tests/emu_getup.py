"""CPU execution of emloco_amd/csrc/getup_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_getup.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_getup.so, a library of its own."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_getup.so")
_lib = None


def build():
    csrc = os.path.join(_ROOT, "emloco_amd", "csrc")
    deps = [os.path.join(_HERE, f) for f in ("emu_getup.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(csrc, f) for f in ("getup_kernels.hip", "reset_kernels.hip", "task_device.h", "dev_math.h", "emloco_types.h")]
    deps.append(os.path.join(_ROOT, "include", "emloco_task.h"))

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_getup.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.emu_getup_split.argtypes = [vp, vp, C.c_int, vp, C.c_uint64, C.c_float, C.c_float, C.c_int, C.c_uint32, vp, vp, vp, vp]
        _lib.emu_getup_flags.argtypes = [vp]
        _lib.emu_getup_amp_default.argtypes = [vp, C.c_int, vp, C.c_int]
        _lib.emu_getup_copy.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
        for f in (_lib.emu_getup_split, _lib.emu_getup_flags, _lib.emu_getup_amp_default, _lib.emu_getup_copy):
            f.restype = C.c_int
    return _lib


def _p(x):
    return None if x is None else x.ctypes.data


def getup_bufs(st):
    """EmlocoGetupBufs over the host arrays of a state dict (getup_cases.state); the arrays are written in place"""
    from emloco_amd import _lib as L
    return L.GetupBufs(int(st["assign"].shape[0]), int(st["pool_taken"].shape[0]), _p(st["pool_root"]), _p(st["pool_dof"]), _p(st["pool_taken"]),
                       _p(st["assign"]), _p(st["counter"]), _p(st["progress"]), _p(st["reset"]), _p(st["terminate"]), _p(st["split_ws"]),
                       _p(st["stats"]))


def split(st, case):
    """emloco_getup_split of a case (getup_cases.split_case) on the state `st` (written in place); returns the four lists"""
    n = case["n"]
    out = {k: np.full(n + 1, -77, np.int32) for k in ("normal", "fall", "recover", "fall_slot")}
    g = getup_bufs(st)
    rc = lib().emu_getup_split(C.byref(g), _p(case["ids"]), n, _p(case["rnd"]), case["seed"], case["recovery_prob"], case["fall_prob"],
                               case["steps"], case["key"], *[_p(out[k]) for k in ("normal", "fall", "recover", "fall_slot")])
    assert rc == 0
    return out


def flags(st):
    g = getup_bufs(st)
    assert lib().emu_getup_flags(C.byref(g)) == 0


def amp_default(amp, ring, ids):
    assert amp.dtype == np.float32 and amp.flags.c_contiguous and ids.dtype == np.int32
    assert lib().emu_getup_amp_default(_p(amp), ring, _p(ids), len(ids)) == 0


def copy(st, root, dof, lambda_ws, fall, fall_slot):
    g = getup_bufs(st)
    assert lib().emu_getup_copy(C.byref(g), _p(root), _p(dof), _p(lambda_ws), _p(fall), _p(fall_slot), len(fall)) == 0

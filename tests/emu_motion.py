"""CPU execution of emloco_amd/csrc/motion_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_motion.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_motion.so, a library of its own."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_motion.so")
_lib = None


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_motion.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps.append(os.path.join(_ROOT, "emloco_amd", "csrc", "motion_kernels.hip"))

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_motion.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_motion_build.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 15 + [C.c_int]
        _lib.emu_motion_build.restype = C.c_int
        _lib.emu_motion_build_error.restype = C.c_char_p
    return _lib


def motion_build(case, out, grid=0):
    """emloco_motion_build on host arrays: `case` as motion_build_cases.pack makes it, `out` the six output arrays (written in place).
    Returns the entry point's code."""
    p = lambda x: None if x is None else x.ctypes.data
    for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs"):
        assert out[k] is None or (out[k].dtype == np.float32 and out[k].flags.c_contiguous)
    return lib().emu_motion_build(case["n_clips"], case["n_skel"], case["F"], p(case["quat_global"]), p(case["root_trans"]),
                                  p(case["frame_start"]), p(case["n_frames"]), p(case["fps"]), p(case["skel_id"]),
                                  p(case["local_translation"]), p(case["parent"]), p(case["taps"]),
                                  *[p(out[k]) for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs")], grid)

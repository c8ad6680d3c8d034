"""CPU execution of emloco_amd/csrc/cnn_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_cnn.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_cnn.so, a library of its own.

`EmuBackend` and `DeviceBackend` (tests/test_gpu_cnn_policy.py) share `CnnHost`: one case of the trunk as host arrays -- observation rows
wider than the map, an output buffer wider than the features with guard words around the whole of it, the packed parameters -- and one
`run(normalize=True)`.  `CASES` are the shapes both back ends run."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_cnn.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5
EPS, CLIP = 1e-5, 5.0

# name -> (res, channels, filters per layer); every case has 3 rows
CASES = {"r16c3": (16, 3, (16, 16, 16)), "r32c1": (32, 1, (16, 16, 16)), "r32c3": (32, 3, (16, 16, 16)), "r64c3": (64, 3, (16, 16, 16)),
         "r16c1_two_layers": (16, 1, (16, 16))}
SEED = 20


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_cnn.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps.append(os.path.join(_ROOT, "emloco_amd", "csrc", "cnn_kernels.hip"))

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_cnn.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


# the argument list of emloco_cnn_trunk (include/emloco_predictor.h) with `grid` in the stream's place
_ARGS = [C.c_int] * 8 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_cnn_trunk.argtypes, _lib.emu_cnn_trunk.restype = _ARGS, C.c_int
        _lib.emu_cnn_error.restype = C.c_char_p
    return _lib


def guarded(n_words, dtype=np.uint32):
    """(whole, view): `view` is n_words zeros of a 4-byte dtype with GUARD words of FILL on either side inside `whole`"""
    whole = np.full(n_words + 2 * GUARD, FILL, np.uint32)
    view = whole[GUARD:GUARD + n_words]
    view[:] = 0
    return whole, view.view(dtype)


def guards_intact(whole):
    return bool((whole[:GUARD] == FILL).all() and (whole[-GUARD:] == FILL).all())


def pack_params(weights, biases):
    """every layer's weights [F][Cin][4][4], then its bias [F], back to back (the `params` argument)"""
    return np.concatenate([np.concatenate([w.ravel(), b.ravel()]) for w, b in zip(weights, biases)]).astype(np.float32)


def draw_case(name, seed=SEED, rows=3):
    """The inputs of a case: raw observation rows (a few values at +-40 so that the clamp acts), random mean / var, weights with a
    negative share and biases that leave a visible part of every layer at zero after the ReLU."""
    res, ch, filters = CASES[name]
    rng = np.random.default_rng([seed, res, ch, len(filters)])
    width = ch * res * res
    lead, tail = 5, 7                                    # columns before the map (x points past them) and after it
    obs = (rng.standard_normal((rows, lead + width + tail)) * 1.5).astype(np.float32)
    obs[0, lead + 3:lead + 6] = 40.0
    obs[rows - 1, lead + width - 4:lead + width - 1] = -40.0
    mean = (rng.standard_normal(width) * 0.3).astype(np.float32)
    var = (rng.uniform(0.05, 2.05, width)).astype(np.float32)
    weights, biases, cin = [], [], ch
    for f in filters:
        weights.append((rng.standard_normal((f, cin, 4, 4)) / np.sqrt(cin * 16.0) * 1.4).astype(np.float32))
        biases.append((rng.standard_normal(f) * 0.2 - 0.05).astype(np.float32))
        cin = f
    return dict(res=res, ch=ch, filters=filters, rows=rows, lead=lead, obs=obs, mean=mean, var=var, weights=weights, biases=biases)


class CnnHost:
    """One case on the host.  `launch(...)` of the subclass runs the kernel on the arrays it is given."""
    OUT_OFF, OUT_TAIL = 3, 6

    def __init__(self, case):
        self.c = case
        res, ch, filters = case["res"], case["ch"], case["filters"]
        side = res >> len(filters)
        self.features = filters[-1] * side * side
        self.ldo = self.OUT_OFF + self.features + self.OUT_TAIL
        self.obs = np.ascontiguousarray(case["obs"], np.float32)
        self.mean, self.var = case["mean"], case["var"]
        self.params = pack_params(case["weights"], case["biases"])
        self.f4 = tuple(filters) + (0,) * (4 - len(filters))

    def run(self, normalize=True, obs=None, **kw):
        """(features (rows, features), untouched columns still at their fill, guards intact)"""
        c = self.c
        obs = self.obs if obs is None else np.ascontiguousarray(obs, np.float32)
        whole, out = guarded(c["rows"] * self.ldo, np.float32)
        out = out.reshape(c["rows"], self.ldo)
        out[:] = -77.0
        self.launch(c["rows"], c["res"], c["ch"], len(c["filters"]), self.f4, obs, c["lead"], obs.shape[1], self.mean, self.var,
                    int(normalize), self.params, out, self.ldo, self.OUT_OFF, **kw)
        at = self.OUT_OFF
        untouched = bool((out[:, :at] == -77.0).all() and (out[:, at + self.features:] == -77.0).all())
        return out[:, at:at + self.features].copy(), untouched, guards_intact(whole)


class EmuBackend(CnnHost):
    def launch(self, rows, res, ch, layers, f4, obs, lead, ldx, mean, var, normalize, params, out, ldo, out_off, grid=0):
        rc = lib().emu_cnn_trunk(rows, res, ch, layers, *f4, obs.ctypes.data + 4 * lead, ldx, mean.ctypes.data, var.ctypes.data, EPS, CLIP,
                                 normalize, params.ctypes.data, out.ctypes.data, ldo, out_off, grid)
        assert rc == 0, lib().emu_cnn_error()

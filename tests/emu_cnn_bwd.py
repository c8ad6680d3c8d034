"""CPU execution of emloco_amd/csrc/cnn_backward_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_cnn_bwd.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_cnn_bwd.so, a library of its own (tests/emu_cnn.py's
recipe).

`EmuBackend` and `DeviceBackend` (tests/test_gpu_cnn_backward.py) share `CnnBwdHost`: one case of the trunk's backward as host arrays --
observation rows wider than the map, a `dout` wider than the features whose other columns are NaN (a read of them poisons the result),
`dparams` and the workspace with guard words around them, the workspace pre-filled so that a write past grid * P floats shows -- and one
`run()`.  `CASES` are the shapes both back ends run; every seed is chosen so that no float64 pre-activation lies within 2e-6 of its
layer's largest of the ReLU's corner (tests/test_cnn_trunk_backward_cpu.py checks that)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_cnn
from emu_cnn import CLIP, EPS, GUARD, guarded, guards_intact, pack_params

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_cnn_bwd.so")
_lib = None
WS_FILL = np.float32(-123.25)

# name -> (res, channels, filters per layer, rows (None: the workspace query's row limit of one launch + 3), seed)
CASES = {"r16c3": (16, 3, (16, 16, 16), 3, 20), "r32c1": (32, 1, (16, 16, 16), 3, 22), "r64c3": (64, 3, (16, 16, 16), 3, 22),
         "r16c1_two_layers": (16, 1, (16, 16), 3, 20), "r8c3_one_layer": (8, 3, (16,), 3, 20),
         "r16c1_four_layers": (16, 1, (16, 16, 16, 16), 3, 20), "r16c3_f5_16_7": (16, 3, (5, 16, 7), 3, 20),
         "r16c1_two_layers_many_rows": (16, 1, (16, 16), None, 20)}


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_cnn_bwd.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(_ROOT, "emloco_amd", "csrc", f) for f in ("cnn_kernels.hip", "cnn_backward_kernels.hip")]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_cnn_bwd.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


# the argument list of emloco_cnn_trunk_backward (include/emloco_predictor.h) with `grid` in the stream's place
_ARGS = ([C.c_int] * 8 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                          C.c_void_p, C.c_void_p, C.c_int64, C.c_int])


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_cnn_trunk_backward.argtypes, _lib.emu_cnn_trunk_backward.restype = _ARGS, C.c_int
        _lib.emu_cnn_bwd_error.restype = C.c_char_p
    return _lib


def param_count(ch, filters):
    n, cin = 0, ch
    for f in filters:
        n, cin = n + f * cin * 16 + f, f
    return n


def workspace_floats(rows, res, ch, filters):
    """emloco_cnn_trunk_backward_workspace of the product's library (it needs no device)"""
    from emloco_amd import _lib as L
    n = L.load().emloco_cnn_trunk_backward_workspace(rows, res, ch, len(filters), *(tuple(filters) + (0,) * (4 - len(filters))))
    assert n > 0, L.load().emloco_last_error()
    return int(n)


def grid_of(rows, res, ch, filters):
    """the workgroups the C ABI launches for `rows`, read off its workspace query"""
    n, p = workspace_floats(rows, res, ch, filters), param_count(ch, filters)
    assert n % p == 0
    return n // p


def split_params(flat, ch, filters):
    """[(dW [F][Cin][4][4], db [F]) per layer] views of a packed vector"""
    out, at, cin = [], 0, ch
    for f in filters:
        w = flat[at:at + f * cin * 16].reshape(f, cin, 4, 4)
        at += f * cin * 16
        out.append((w, flat[at:at + f]))
        at, cin = at + f, f
    assert at == flat.size
    return out


def draw_case(name):
    """The inputs of a case, drawn like emu_cnn.draw_case (clamped values present, biases non-zero, a visible part of every layer at zero
    after the ReLU), plus a random dout."""
    res, ch, filters, rows, seed = CASES[name]
    if rows is None:
        rows = grid_of(1 << 20, res, ch, filters) + 3
    rng = np.random.default_rng([seed, res, ch, len(filters), rows])
    width = ch * res * res
    lead, tail = 5, 7
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
    side = res >> len(filters)
    dout = rng.standard_normal((rows, filters[-1] * side * side)).astype(np.float32)
    return dict(name=name, res=res, ch=ch, filters=filters, rows=rows, lead=lead, obs=obs, mean=mean, var=var, weights=weights, biases=biases,
                dout=dout)


class CnnBwdHost:
    """One case on the host.  `launch(...)` of the subclass runs the two kernels on the arrays it is given."""
    DOUT_OFF, DOUT_TAIL = 3, 6

    def __init__(self, case):
        self.c = case
        res, ch, filters = case["res"], case["ch"], case["filters"]
        side = res >> len(filters)
        self.features = filters[-1] * side * side
        self.lddo = self.DOUT_OFF + self.features + self.DOUT_TAIL
        self.obs = np.ascontiguousarray(case["obs"], np.float32)
        self.mean, self.var = case["mean"], case["var"]
        self.params = pack_params(case["weights"], case["biases"])
        self.count = param_count(ch, filters)
        assert self.params.size == self.count
        self.f4 = tuple(filters) + (0,) * (4 - len(filters))
        self.ws_floats = workspace_floats(case["rows"], res, ch, filters)
        self.abi_grid = self.ws_floats // self.count

    def run(self, normalize=True, obs=None, dout=None, grid=0):
        """(dparams [P] float32, guards of dparams and of the workspace intact, the workspace untouched past grid * P floats)"""
        c = self.c
        obs = self.obs if obs is None else np.ascontiguousarray(obs, np.float32)
        wide = np.full((c["rows"], self.lddo), np.nan, np.float32)
        wide[:, self.DOUT_OFF:self.DOUT_OFF + self.features] = c["dout"] if dout is None else dout
        dp_whole, dp = guarded(self.count, np.float32)
        dp[:] = 55.0                                               # (overwritten, not accumulated into)
        ws_whole, ws = guarded(self.ws_floats, np.float32)
        ws[:] = WS_FILL
        kw = {"grid": grid} if grid else {}
        self.launch(c["rows"], c["res"], c["ch"], len(c["filters"]), self.f4, obs, c["lead"], obs.shape[1], self.mean, self.var, int(normalize),
                    self.params, wide, self.lddo, self.DOUT_OFF, dp_whole, ws_whole, self.ws_floats, **kw)
        used = (grid if 0 < grid < self.abi_grid else self.abi_grid) * self.count
        tail_ok = bool((ws[used:] == WS_FILL).all())
        return dp.copy(), guards_intact(dp_whole) and guards_intact(ws_whole), tail_ok


class EmuBackend(CnnBwdHost):
    def launch(self, rows, res, ch, layers, f4, obs, lead, ldx, mean, var, normalize, params, dout, lddo, dout_off, dp_whole, ws_whole, ws_floats,
               grid=0):
        rc = lib().emu_cnn_trunk_backward(rows, res, ch, layers, *f4, obs.ctypes.data + 4 * lead, ldx, mean.ctypes.data, var.ctypes.data, EPS, CLIP,
                                          normalize, params.ctypes.data, dout.ctypes.data, lddo, dout_off, dp_whole.ctypes.data + 4 * GUARD,
                                          ws_whole.ctypes.data + 4 * GUARD, ws_floats, grid)
        assert rc == 0, lib().emu_cnn_bwd_error()

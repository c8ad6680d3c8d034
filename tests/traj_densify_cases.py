"""Inputs, reference and bar shared by tests/test_traj_densify_cpu.py (emulated kernel) and tests/test_gpu_traj_densify.py (device).

Reference: scipy.interpolate.CubicSpline(knot_t, way, axis=0, bc_type='natural')(query_t) in float64 on the float32 waypoints the
kernel reads and the float64 knots / queries the caller gave (the kernel rounds those to float32: part of its error).

BAR_M, absolute, in metres, on origin-shifted output.  Measured maxima over every case below (walkers of 0..3 m/s, extent up to
18 m, extrapolation included):
    kernel emulated on the CPU (tests/emu/emu_task.cpp)         MEASURED_EMU_M
    kernel on the MI355X                                        MEASURED_DEVICE_M
The bar is 4 x the larger: the margin covers a different operation order in the device's division and nothing else.  (A float32
restatement of the solve measured 3.9e-6 m at an extent of 2.9 m before the kernel existed; a bar above 2e-5 m would mean the solve
is wrong, not noisy.)  With `origin` off the origin is added back in float32: one ulp of the largest output coordinate on top.
"""
import numpy as np
from scipy.interpolate import CubicSpline

from emloco_amd.env.util.traj_densify import TRAJ_PHASE

MEASURED_EMU_M = 4.24e-6          # 4.233e-6: query128_outside, 65 tracks, no offset
MEASURED_DEVICE_M = 4.24e-6       # 4.233e-6, the same case: the device reproduces the emulation
BAR_M = 4 * max(MEASURED_EMU_M, MEASURED_DEVICE_M)
assert BAR_M <= 2e-5

N_TRAJ = (1, 63, 64, 65, 257)          # one lane, a wave edge on both sides, several workgroups with a ragged tail
QUERY_101 = np.arange(101, dtype=np.float64)


def tracks(n, knot_t, seed, offset=0.0):
    """(n, K, 3) float32 walkers: speed 0..3 m/s along a wandering heading, a little height noise, world offset +-`offset` m.
    One vertex unit is 0.056 s (an episode of 5.6 s over 100 segments), so the shipped 7.07-unit knots are 0.4 s apart."""
    r = np.random.RandomState(seed)
    knot_t = np.asarray(knot_t, np.float64)
    K = knot_t.size
    dt = np.diff(knot_t, prepend=knot_t[0]) * 0.0566
    speed = r.uniform(0, 3, (n, 1))
    head = r.uniform(-np.pi, np.pi, (n, 1)) + np.cumsum(r.randn(n, K) * 0.15, 1)
    step = np.stack([np.cos(head), np.sin(head), np.zeros_like(head)], -1) * (speed * dt[None, :])[..., None]
    way = np.cumsum(step, 1)
    way[..., 2] = 0.9 + r.randn(n, K) * 0.02
    if offset:
        way[..., :2] += r.uniform(-offset, offset, (n, 1, 2))
    return way.astype(np.float32)


def _uneven16():
    r = np.random.RandomState(5)
    return np.cumsum(np.concatenate([[0.0], r.uniform(2.0, 12.0, 15)]))


def _outside128():
    r = np.random.RandomState(6)
    q = r.uniform(-12.0, 100.0, 128)                     # unsorted, below the first and above the last shipped knot (84.87)
    q[:4] = [-12.0, 100.0, 0.0, TRAJ_PHASE[-1]]
    return q


# name -> (knots, queries): the shipped sizes and the limits of the entry point
SHAPES = {
    "shipped": (TRAJ_PHASE, QUERY_101),
    "knots4": (TRAJ_PHASE[[0, 4, 8, 12]], QUERY_101),
    "knots16_uneven": (_uneven16(), np.linspace(-5.0, 110.0, 97)),
    "query1": (TRAJ_PHASE, np.array([33.3])),
    "query128_outside": (TRAJ_PHASE, _outside128()),
}


def reference(way32, knot_t, query_t, origin):
    """float64 scipy on the float32 waypoints; origin-shifted (x, y by the first waypoint) when `origin`."""
    way = way32.astype(np.float64)
    ref = CubicSpline(np.asarray(knot_t, np.float64), way, axis=1, bc_type="natural")(np.asarray(query_t, np.float64))
    if origin:
        ref[..., :2] -= way[:, :1, :2]
    return ref


def bar(ref, origin):
    return BAR_M if origin else BAR_M + float(np.spacing(np.float32(np.abs(ref).max())))

"""Throwaway measurement of emloco_traj_densify: 2e5 tracks at the shipped sizes (13 knots, 101 queries).

    python tools/exp/densify_timing.py [n_traj]

Warm-up launches, then 100 launches between two events; against scipy's CubicSpline on the host for the same batch and against the
kernel's own traffic (156 B read + 1 212 B written per track; `valid` adds a byte).
"""
import os
import sys
import time

import numpy as np
import torch
from scipy.interpolate import CubicSpline

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from emloco_amd.env.util.traj_densify import TRAJ_PHASE, densify  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
r = np.random.RandomState(0)
way = np.cumsum(r.randn(n, 13, 3).astype(np.float32) * 0.4, 1) + r.uniform(-100, 100, (n, 1, 3)).astype(np.float32)
dev = torch.device("cuda", 0)
w = torch.from_numpy(way).to(dev)
for _ in range(10):
    out, valid = densify(w)
torch.cuda.synchronize()
reps = 100
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
best = float("inf")
for _ in range(5):
    e0.record()
    for _ in range(reps):
        densify(w)
    e1.record()
    torch.cuda.synchronize()
    best = min(best, e0.elapsed_time(e1) / reps)
t0 = time.perf_counter()
ref = CubicSpline(TRAJ_PHASE, way.astype(np.float64), axis=1, bc_type="natural")(np.arange(101.0))
host = (time.perf_counter() - t0) * 1e3
org = way[:, :1].astype(np.float64).copy()
org[..., 2] = 0
err = np.abs((out.cpu().numpy().astype(np.float64)) - ref).max()
written, moved = n * 1212, n * (1212 + 156 + 1)
print(f"emloco_traj_densify: {n} tracks, {best * 1e3:.1f} us per launch (python call and two torch.empty included), "
      f"{written / best / 1e6:.0f} GB/s written, {moved / best / 1e6:.0f} GB/s moved; scipy on the host {host:.0f} ms ({host / best:.0f} x); "
      f"max |kernel - scipy| {err:.2e} m at +-100 m (origin added back)")

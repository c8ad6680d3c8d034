#!/usr/bin/env python3
"""Golden vectors of the group observation, made by running the REFERENCE's own functions here.

    python tests/golden/gen_golden_crowd_people.py     # writes tests/golden/crowd_people.npz

Runs `compute_group_observation` and `HumanoidPedestrianTerrain._compute_flip_task_obs` of
pacer/pacer/env/tasks/humanoid_pedestrain_terrain.py (through tests/golden/_ref_shim.py; the method unbound, on a
`types.SimpleNamespace` that carries the attributes it reads) on one torch thread.  Only inputs (body states, group sizes) and outputs
are stored.  The mirrored row is made with velocity_map False: with it the reference looks for the block inside the height map
(include/emloco_task.h, EmlocoCrowdPeople).

  case a   16 envs in groups of 8.  Env 5 stands 40 m away, so every one of its own neighbours is masked; the two groups share one
           patch of ground, so that some env has a member of the OTHER group nearer than its fifth own neighbour.
  case b   12 envs in groups of 6, the minimum.  Envs 7 and 10 are far, so the other four of their group each see two masked neighbours.
Each case is redrawn until, for every env, the distances to the other members of its group differ pairwise by at least 1e-4 m and none
lies within 1e-3 m of 10 m: the selection and the mask then do not hang on the last bit of a square root.  Root rotations carry a tilt
of up to 0.2 rad.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_shim  # noqa: E402
from gen_golden_crowd import yaw_quat  # noqa: E402
import emu_crowd_people as EP  # noqa: E402

T, RES = 15, 2
CASES = [("a", 16, 8, {5: 40.0}), ("b", 12, 6, {7: 25.0, 10: -30.0})]


def draw(rng, n_env, gs, far):
    rb = np.zeros((n_env, 24, 13), np.float32)
    for e in range(n_env):
        root = np.array([30.0, 30.0, 0.9]) + rng.uniform(-1, 1, 3) * [3.5, 3.5, 0.05]
        if e in far:
            root[0] += far[e]
        rb[e, :, :3] = root + rng.uniform(-0.9, 0.9, (24, 3))
        rb[e, 0, :3] = root
        rb[e, 0, 3:7] = yaw_quat(rng.uniform(-np.pi, np.pi), rng.uniform(-0.2, 0.2))
        q = rng.normal(size=(23, 4))
        rb[e, 1:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        rb[e, :, 7:13] = rng.uniform(-1.5, 1.5, (24, 6))
    return rb


def group_distances(rb, gs):
    """[E][gs - 1]: every env's distances to the other members of its group, float64 of the float32 coordinates"""
    root = rb[:, 0, :3].astype(np.float64)
    out = []
    for e in range(len(root)):
        g0 = (e // gs) * gs
        out.append([np.linalg.norm(root[m] - root[e]) for m in range(g0, g0 + gs) if m != e])
    return np.array(out)


def conditions(name, rb, gs, far):
    d = group_distances(rb, gs)
    s = np.sort(d, axis=1)
    if np.diff(s, axis=1).min() < 1e-4 or np.abs(d - 10.0).min() < 1e-3:
        return False
    masked = (s[:, :5] > 10.0).sum(1)
    root = rb[:, 0, :3].astype(np.float64)
    if name == "a":
        other = [min(np.linalg.norm(root[m] - root[e]) for m in range(len(root)) if m // gs != e // gs) for e in range(len(root))]
        return bool(masked[5] == 5 and (np.asarray(other) < s[:, 4]).any() and masked[:5].max() == 0)
    return bool(all(masked[e] == 2 for e in (6, 8, 9, 11)) and masked[:6].max() == 0)


def main():
    _ref_shim.install_pacer()
    import torch
    import env.tasks.humanoid_pedestrain_terrain as HPT
    torch.set_num_threads(1)
    Task = HPT.HumanoidPedestrianTerrain
    rng = np.random.default_rng(20261021)
    out = dict(cases=np.array([c[0] for c in CASES]))
    worst = 0.0
    for name, n_env, gs, far in CASES:
        while True:
            rb = draw(rng, n_env, gs, far)
            if conditions(name, rb, gs, far):
                break
        assert conditions(name, rb, gs, far)
        t = torch.from_numpy(rb)
        rows = HPT.compute_group_observation(t[:, :, 0:3].contiguous(), t[:, :, 3:7].contiguous(), t[:, :, 7:10].contiguous(),
                                             torch.tensor(EP.BODIES), gs, True)
        assert rows.dtype == torch.float32 and rows.shape == (n_env, EP.WIDTH)
        ns = types.SimpleNamespace(_num_traj_samples=T, terrain_obs=True, velocity_map=False, num_height_points=RES * RES,
                                   _divide_group=True, _group_obs=True)
        front = torch.from_numpy(rng.uniform(-1, 1, (n_env, 2 * T + RES * RES)).astype(np.float32))
        flip = Task._compute_flip_task_obs(ns, torch.cat([front, rows], dim=1), None)
        assert flip.shape == (n_env, 2 * T + RES * RES + EP.WIDTH)
        flip = flip[:, 2 * T + RES * RES:]
        r64, f64, nb = EP.people_f64(rb, gs)
        err = max(float(np.abs(rows.numpy() - r64).max()), float(np.abs(flip.numpy() - f64).max()))
        worst = max(worst, err)
        print(f"case {name}: masked neighbours per env {(np.sort(group_distances(rb, gs), 1)[:, :5] > 10).sum(1).tolist()}, "
              f"reference fp32 against the float64 restatement: {err:.7e}")
        out[name + "_rb"], out[name + "_group_size"] = rb, np.array(gs)
        out[name + "_rows"], out[name + "_flip"] = rows.numpy(), flip.numpy()
    print(f"worst difference of the reference's fp32 rows from the float64 restatement: {worst:.7e}; the tests' bar is four times that")
    path = os.path.join(HERE, "crowd_people.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

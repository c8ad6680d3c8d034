#!/usr/bin/env python3
"""Golden vectors of the crowd-aware terrain sensor, made by running the REFERENCE's own methods here.

    python tests/golden/gen_golden_crowd.py     # writes tests/golden/crowd_sensor.npz

Runs `HumanoidPedestrianTerrain.init_square_height_points / init_root_points / init_center_height_points / get_heights /
get_center_heights / _compute_flip_task_obs` and `Terrain.sample_height_points` of
pacer/pacer/env/tasks/humanoid_pedestrain_terrain.py, unbound, on a `types.SimpleNamespace` that carries the attributes they read
(through tests/golden/_ref_shim.py), on one torch thread: the duplicate indices of the stamps then resolve as last writer wins.
The four lines that join the two (:427-437: centre mean minus height, clip, x 5) are restated below.  Only inputs (field, root and
head states, seeds) and outputs are stored.

8 envs, groups of 4, a 96 x 80 field in steps of 30 units.  Every case is redrawn, env by env, until
  * no probe, root point or centre probe lies within MARGIN of a cell boundary, so no case hangs on the last bit of a sine.
    MARGIN is 2e-5 m: about five times what float32 rounding moves a coordinate below 10 m.  A wider margin cannot be met: the 200
    root points of one env at a generic heading already lie 0.0005 m apart modulo the cell size on average, and the 64 probe
    columns of the res 64 grid step through the cell in units of 1 / 63 of it;
  * (stamped cases) at least a tenth of the probes of the +-2 m grids read a stamped cell, and two members share a cell.  The
    +-4 m grid of case d covers 64 m^2 against about 2.6 m^2 of stamps: it has to reach 2 %.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_shim  # noqa: E402
import crowd_ref  # noqa: E402

E, GROUP, HEAD, T = 8, 4, 13, 15
HS, VS, MARGIN = 0.1, 0.005, 2e-5
CASES = [  # name, res, extent, stamps, velocity, env_ids, centres of the two groups, spread, min stamped fraction
    ("a", 8, 2.0, True, True, None, ((3.1, 3.3), (6.2, 4.6)), 0.6, 0.1),
    ("b", 8, 2.0, True, False, None, ((3.4, 4.2), (6.6, 3.1)), 0.6, 0.1),
    ("c", 8, 2.0, False, True, None, ((3.0, 3.0), (6.0, 5.0)), 0.6, 0.0),
    ("d", 64, 4.0, True, True, None, ((4.2, 3.9), (5.3, 4.4)), 0.7, 0.02),
    ("d_subset", 64, 4.0, True, True, [5, 0, 2], ((4.2, 3.9), (5.3, 4.4)), 0.7, 0.02),
    ("e", 8, 2.0, True, True, None, ((0.12, 3.0), (5.0, 7.85)), 0.5, 0.1),
    ("f", 8, 2.0, True, True, None, ((4.5, 4.0), (4.5, 4.0)), 0.6, 0.1),
]


def yaw_quat(yaw, tilt):
    """heading about z with a small tilt about x: xyzw"""
    qz = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
    qx = np.array([np.sin(tilt / 2), 0, 0, np.cos(tilt / 2)])
    x1, y1, z1, w1 = qz
    x2, y2, z2, w2 = qx
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def draw_env(rng, centre, spread, res, extent):
    while True:
        rb1 = np.zeros((1, 24, 13), np.float32)
        rb1[:, :, 6] = 1
        xy = np.asarray(centre) + rng.uniform(-spread, spread, 2)
        yaw = rng.uniform(-np.pi, np.pi)
        rb1[0, 0, :3] = [xy[0], xy[1], 0.9 + rng.uniform(-0.05, 0.05)]
        rb1[0, 0, 3:7] = yaw_quat(yaw, rng.uniform(-0.2, 0.2))
        rb1[0, 0, 7:10] = rng.uniform(-1.5, 1.5, 3) * [1, 1, 0.2]
        rb1[0, HEAD, :3] = [xy[0] + rng.uniform(-0.1, 0.1), xy[1] + rng.uniform(-0.1, 0.1), 1.5]
        rb1[0, HEAD, 3:7] = yaw_quat(yaw + rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2))
        if crowd_ref.clear_of_boundaries(rb1, HEAD, res, extent, HS, MARGIN):
            return rb1[0]


def main():
    _ref_shim.install_pacer()
    import torch
    import env.tasks.humanoid_pedestrain_terrain as HPT
    torch.set_num_threads(1)
    if not hasattr(HPT.flags, "divide_group"):
        HPT.flags.divide_group = False
    Task = HPT.HumanoidPedestrianTerrain

    rng = np.random.default_rng(20261020)
    hf = (rng.integers(-3, 4, size=(96, 80)) * 30).astype(np.int16)
    out = dict(heightfield=hf, hscale=np.array(HS), vscale=np.array(VS), group_size=np.array(GROUP), head_body=np.array(HEAD),
               cases=np.array([c[0] for c in CASES]))
    terrain = object.__new__(HPT.Terrain)
    terrain.heightsamples = torch.from_numpy(hf)
    terrain.horizontal_scale, terrain.vertical_scale = HS, VS
    drawn = {}
    for name, res, extent, stamps, velocity, env_ids, centres, spread, min_frac in CASES:
        key = (res, extent, centres)
        while key not in drawn:
            rb = np.stack([draw_env(rng, centres[e // GROUP], spread, res, extent) for e in range(E)])
            if not stamps:
                drawn[key] = rb
                break
            own = crowd_ref.owners(rb, hf.shape, HS, GROUP)
            pts = crowd_ref.probe_points(rb, HEAD, res, extent)
            px, py = crowd_ref.map_index(pts[..., 0], HS, hf.shape[0]), crowd_ref.map_index(pts[..., 1], HS, hf.shape[1])
            frac = np.mean([(int(px[e, p]), int(py[e, p])) in own[e // GROUP] for e in range(E) for p in range(res * res)])
            root = rb[:, 0]
            rp = crowd_ref.world_points(root[:, :3], crowd_ref.heading(root[:, 3:7]), np.linspace(-0.25, 0.25, 10).astype(np.float32),
                                        np.linspace(-0.5, 0.5, 20).astype(np.float32))
            rx, ry = crowd_ref.map_index(rp[..., 0], HS, hf.shape[0]), crowd_ref.map_index(rp[..., 1], HS, hf.shape[1])
            shared = any(len(set(zip(rx[e].tolist(), ry[e].tolist())) & set(zip(rx[f].tolist(), ry[f].tolist()))) > 0
                         for e in range(E) for f in range(e + 1, E) if e // GROUP == f // GROUP)
            if frac >= min_frac and shared:
                drawn[key] = rb
                print(f"case {name}: {frac:.3f} of the probes on a stamped cell")
        rb = drawn[key]
        root_states = torch.from_numpy(rb[:, 0].copy())
        head_pose = torch.from_numpy(rb[:, HEAD, :7].copy())
        ns = types.SimpleNamespace(
            cfg={"env": {"terrain": {"terrainType": "trimesh"}, "use_center_height": True}}, device="cpu", num_envs=E,
            smpl_humanoid=True, _has_upright_start=True, sensor_extent=extent, sensor_res=res, velocity_map=velocity,
            terrain_obs=True, _divide_group=stamps, _group_obs=False, _disable_group_obs=False, _group_num_people=GROUP,
            _group_ids=torch.tensor(np.arange(E / GROUP).repeat(GROUP).astype(int)), _humanoid_root_states=root_states,
            terrain=terrain, _num_traj_samples=T)
        ns.height_points = Task.init_square_height_points(ns)
        ns.root_points = Task.init_root_points(ns)
        ns.center_height_points = Task.init_center_height_points(ns)
        ids = None if env_ids is None else torch.tensor(env_ids)
        n = E if ids is None else len(env_ids)
        sel = slice(None) if ids is None else ids
        measured = Task.get_heights(ns, root_states=head_pose[sel], env_ids=ids)
        centre = Task.get_center_heights(ns, root_states=root_states[sel], env_ids=ids).mean(dim=-1, keepdim=True)
        if velocity:                                                             # :431-437
            m = measured.view(n, -1, 3)
            m[..., 0] = centre - m[..., 0]
            heights = m.view(n, -1)
        else:
            heights = centre - measured
        heights = torch.clip(heights, -3, 3.) * 5
        loc = torch.from_numpy(rng.uniform(-1, 1, (n, 2 * T)).astype(np.float32))
        flip = Task._compute_flip_task_obs(ns, torch.cat([loc, heights], dim=1), ids)
        assert torch.equal(flip[:, 0:2 * T:2], loc[:, 0::2]) and torch.equal(flip[:, 1:2 * T:2], -loc[:, 1::2])
        assert heights.dtype == torch.float32 and heights.shape == (n, res * res * (3 if velocity else 1))
        out[name + "_rb"] = rb
        out[name + "_cfg"] = np.array([res, int(stamps), int(velocity)])
        out[name + "_extent"] = np.array(extent)
        out[name + "_env_ids"] = np.array([] if env_ids is None else env_ids, np.int32)
        out[name + "_rows"] = heights.numpy()
        out[name + "_flip"] = flip[:, 2 * T:].numpy()
    path = os.path.join(HERE, "crowd_sensor.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

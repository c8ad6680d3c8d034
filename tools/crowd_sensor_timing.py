#!/usr/bin/env python3
"""Time of the crowd-aware terrain sensor on the device against a torch formulation of the same step (profiles/crowd_sensor.txt).

    python tools/crowd_sensor_timing.py [--envs 2048] [--group 512] [--res 64] [--extent 4] [--rows 1800] [--cols 1800] [--iters 200]

Synthetic state: the members of every group stand at random places and headings inside a 40 m square of a stepped height field.  HIP
events around `--iters` calls after a warm-up, on one stream.  emloco_task_crowd_sensor is two launches; they are told apart by a
second timing with an id list of ONE env (the stamps of all envs + the gather of one row).  The torch baseline is the reference's
sample_height_points (humanoid_pedestrain_terrain.py:1221-1297) on device tensors: per group a clone of the field, the indexed stamp,
a zeroed velocity map, the indexed reads.  Its rows are compared with the kernel's before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emloco_amd import _lib as L  # noqa: E402
from emloco_amd.crowd_sensor import CrowdSensor, root_tables, probe_table, stamp_units  # noqa: E402
from emloco_amd.gym import torch_utils as tu  # noqa: E402


def heading_quat(q, inverse=False):
    ref = torch.zeros_like(q[:, :3])
    ref[:, 0] = 1
    d = tu.quat_rotate(q, ref)
    h = torch.atan2(d[:, 1], d[:, 0])
    axis = torch.zeros_like(ref)
    axis[:, 2] = 1
    return tu.quat_from_angle_axis(-h if inverse else h, axis)


def torch_step(rb, hf, hs, vs, head, res, pts, root_pts, group, units):
    """the reference's get_heights + sample_height_points with groups and the velocity map, all envs; [E][res * res][3] before the
    centre mean is subtracted"""
    E = rb.shape[0]
    N, R = pts.shape[0], root_pts.shape[0]
    root = rb[:, 0]
    hq = heading_quat(rb[:, head, 3:7])
    world = tu.quat_apply(hq.repeat(1, N).reshape(-1, 4), pts.repeat(E, 1)).view(E, N, 3) + rb[:, head, None, :3]
    rq = heading_quat(root[:, 3:7])
    rworld = tu.quat_apply(rq.repeat(1, R).reshape(-1, 4), root_pts.repeat(E, 1)).view(E, R, 3) + root[:, None, :3]

    def to_map(p):
        p = (p / hs).long()
        return torch.clip(p[..., 0], 0, hf.shape[0] - 2), torch.clip(p[..., 1], 0, hf.shape[1] - 2)

    px, py = to_map(world)
    rx, ry = to_map(rworld)
    G = E // group
    fields = hf[None].repeat(G, 1, 1)
    vel_maps = torch.zeros(fields.shape + (3,), device=rb.device)
    hinv = heading_quat(root[:, 3:7], inverse=True)
    heights = torch.zeros((E, N), device=rb.device)
    vel = torch.zeros((E, N, 2), device=rb.device)
    for g in range(G):
        sl = slice(g * group, (g + 1) * group)
        gx, gy = rx[sl].reshape(-1), ry[sl].reshape(-1)
        fields[g][gx, gy] += units
        vel_maps[g][gx, gy] = root[sl, 7:10].repeat(1, R).view(-1, 3)
        qx, qy = px[sl].reshape(-1), py[sl].reshape(-1)
        heights[sl] = (torch.min(fields[g][qx, qy], fields[g][qx + 1, qy + 1]).view(group, N).long() * vs)
        v = vel_maps[g][qx, qy].view(group, N, 3) - root[sl, None, 7:10]
        vel[sl] = tu.quat_rotate(hinv[sl].repeat(1, N).view(-1, 4), v.view(-1, 3)).view(group, N, 3)[..., :2]
    return torch.cat([heights[..., None], vel], dim=-1)


def timed(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("envs", 2048), ("group", 512), ("res", 64), ("rows", 1800), ("cols", 1800), ("iters", 200), ("torch_iters", 10)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--extent", type=float, default=4.0)
    a = ap.parse_args()
    L.require_device()
    dev = torch.device("cuda")
    rng = np.random.default_rng(1)
    E, hs, vs = a.envs, 0.1, 0.005
    hf = torch.from_numpy((rng.integers(-3, 4, size=(a.rows, a.cols)) * 30).astype(np.int16)).to(dev)
    rb = np.zeros((E, 24, 13), np.float32)
    rb[:, :, 6] = 1
    centre = rng.uniform(40, min(a.rows, a.cols) * hs - 40, (E // a.group, 2)).repeat(a.group, 0)
    xy = centre + rng.uniform(-20, 20, (E, 2))
    yaw = rng.uniform(-np.pi, np.pi, (E, 2))
    rb[:, 0, :2], rb[:, 13, :2] = xy, xy + 0.05
    rb[:, 0, 2], rb[:, 13, 2] = 0.9, 1.5
    for body, k in ((0, 0), (13, 1)):
        rb[:, body, 5], rb[:, body, 6] = np.sin(yaw[:, k] / 2), np.cos(yaw[:, k] / 2)
    rb[:, 0, 7:10] = rng.uniform(-1.5, 1.5, (E, 3))
    rb = torch.from_numpy(rb).to(dev)
    width = a.res * a.res * 3
    obs, flip = torch.zeros((E, width), device=dev), torch.zeros((E, width), device=dev)
    sensor = CrowdSensor(rb_state=rb, heightfield=hf, hscale=hs, vscale=vs, head_body=13, n_env=E, num_env_group=a.group, stamps=True,
                         velocity_map=True, res=a.res, extent=a.extent, obs=obs, flip_obs=flip)
    one = torch.zeros(1, dtype=torch.int32, device=dev)

    xy_t = torch.from_numpy(probe_table(a.res, a.extent)).to(dev)
    gx, gy = torch.meshgrid(xy_t, xy_t, indexing="ij")
    pts = torch.stack([gx.flatten(), gy.flatten(), torch.zeros(a.res * a.res, device=dev)], -1)
    rx, ry = (torch.from_numpy(t).to(dev) for t in root_tables())
    gx, gy = torch.meshgrid(rx, ry, indexing="ij")
    root_pts = torch.stack([gx.flatten(), gy.flatten(), torch.zeros(200, device=dev)], -1)
    units = torch.tensor(stamp_units(vs), dtype=torch.int16, device=dev)
    step = lambda: torch_step(rb, hf, hs, vs, 13, a.res, pts, root_pts, a.group, units)

    # same results first: height channel back from the kernel's clipped row where it is not clipped, velocity channels directly
    sensor.run()
    ref = step()
    torch.cuda.synchronize()
    got = obs.view(E, -1, 3)
    velref = torch.clip(ref[..., 1:], -3, 3) * 5
    agree = ((got[..., 1:] - velref).abs().max(-1).values <= 2e-5).float().mean().item()
    print(f"crowd sensor, {E} envs in groups of {a.group}, res {a.res}, extent {a.extent}, 3 channels, field {a.rows} x {a.cols}; "
          f"owner map {sensor.owner_bytes} bytes ({sensor.n_groups} groups), tag of {32 - sensor.epoch.shift} bits")
    print(f"probes whose velocity channels equal the torch formulation's within 2e-5: {agree:.6f} "
          "(a duplicate cell has no defined winner in torch on a GPU)")
    t_all = timed(lambda: sensor.run(), a.iters)
    t_one = timed(lambda: sensor.run(one), a.iters)
    t_torch = timed(step, a.torch_iters, warm=2)
    print(f"HIP events, mean of {a.iters} calls after 10 warm-up calls:")
    print(f"  emloco_task_crowd_sensor, all rows (stamp + gather)      {t_all * 1e3:9.1f} us")
    print(f"  emloco_task_crowd_sensor, one row (stamp + 1 workgroup)  {t_one * 1e3:9.1f} us")
    print(f"  gather of {E} rows (difference)                        {(t_all - t_one) * 1e3:9.1f} us")
    print(f"  bytes written: {2 * E * width * 4} (two rows of {width} floats per env) -> {2 * E * width * 4 / (t_all - t_one) / 1e6:.1f} GB/s over the gather")
    print(f"torch formulation of the same step on the same device (mean of {a.torch_iters} after 2): {t_torch:9.3f} ms = {t_torch / t_all:.0f} x")


if __name__ == "__main__":
    main()

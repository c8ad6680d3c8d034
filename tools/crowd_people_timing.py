#!/usr/bin/env python3
"""Time of the group observation on the device (profiles/crowd_people.txt).

    python tools/crowd_people_timing.py [--envs 2048] [--group 512] [--square 40] [--iters 200] [--test_steps 64] [--small_terrain]

Part 1, synthetic state, two crowds: `spread` -- the members of every group at random places inside a `--square` m square (the crowd
sensor's timing shape), bodies about their roots -- and `one spot` -- every root at the same point, what the shipped configuration's
reset gives (every distance ties; the kernel orders by member index).  HIP events around `--iters` calls of emloco_task_crowd_people
(two launches) after a warm-up, on one stream, and beside it a torch formulation written for this tool: the reference's
[groups, gs, gs] distance tensor, topk(6), three gathers, the rotation and the mask (it drops the first hit like the reference, so on
the one-spot crowd its neighbours are not the kernel's; on the spread crowd the two are compared).
Part 2, pacer_group_obs.yaml with a random-init sept policy and LocoVal: the step time of the --test loop, and the share of it that
the call on the loop's last state takes (`--test_steps 0`: skipped)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emloco_amd import _lib as L  # noqa: E402
from emloco_amd.crowd_people import CrowdPeople  # noqa: E402
from emloco_amd.gym import torch_utils as tu  # noqa: E402


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


def synthetic(E, group, square, rng, one_spot):
    rb = np.zeros((E, 24, 13), np.float32)
    centre = rng.uniform(40, 140, (E // group, 2)).repeat(group, 0)
    root = np.concatenate([centre + (0 if one_spot else rng.uniform(-square / 2, square / 2, (E, 2))), np.full((E, 1), 0.95)], axis=1)
    rb[:, :, :3] = root[:, None] + rng.uniform(-0.9, 0.9, (E, 24, 3))
    rb[:, 0, :3] = root
    q = rng.normal(size=(E, 24, 4)) * [0.1, 0.1, 1.0, 1.0]
    rb[:, :, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    rb[:, :, 7:10] = rng.uniform(-1.5, 1.5, (E, 24, 3))
    return rb


def torch_people(rb, group, bodies):
    """compute_group_observation as torch ops on the device: distance tensor, topk, gathers, rotation, mask -> [E][165]"""
    E = rb.shape[0]
    pos, vel = rb[:, :, 0:3], rb[:, 0, 7:10]
    root = pos[:, 0]
    hinv = tu.calc_heading_quat_inv(rb[:, 0, 3:7])
    g = root.view(-1, group, 3)
    dist = torch.norm(g[:, :, None, :] - g[:, None, :, :], dim=-1)
    d, idx = torch.topk(dist, 6, dim=-1, largest=False)
    d, idx = d[..., 1:].reshape(E, 5), idx[..., 1:].reshape(E, 5)
    sel = idx + (torch.arange(E, device=rb.device) // group * group)[:, None]
    far = (d > 10)[..., None]
    p = pos[sel][:, :, bodies] - root[:, None, None, :]                                   # [E][5][10][3]
    p = tu.quat_rotate(hinv[:, None, None, :].expand(E, 5, 10, 4).reshape(-1, 4), p.reshape(-1, 3)).view(E, 5, 30)
    v = tu.quat_rotate(hinv[:, None, :].expand(E, 5, 4).reshape(-1, 4), vel[sel].reshape(-1, 3)).view(E, 5, 3)
    return torch.cat([p.masked_fill(far, 0.0).reshape(E, 150), v.masked_fill(far, 0.0).reshape(E, 15)], dim=1), sel


def part1(a):
    dev = torch.device("cuda")
    E = a.envs
    bodies = torch.tensor(L.PEOPLE_BODIES, device=dev)
    print(f"group observation, {E} envs in groups of {a.group}; HIP events, mean of {a.iters} calls after 10 warm-up calls")
    out = {}
    for name, one_spot in (("spread", False), ("one spot", True)):
        rb = torch.from_numpy(synthetic(E, a.group, a.square, np.random.default_rng(1), one_spot)).to(dev)
        obs, flip = torch.zeros((E, 368 + 30 + 1024 + 165), device=dev), torch.zeros((E, 368 + 30 + 1024 + 165), device=dev)
        people = CrowdPeople(rb_state=rb, n_env=E, group_size=a.group, obs=obs, flip_obs=flip, col=obs.shape[1] - 165, neighbours=True)
        people.run()
        rows, sel = torch_people(rb, a.group, bodies)
        zero = float((obs[:, -165:].view(E, 55, 3) == 0).all(-1).float().mean())
        if not one_spot:
            same = bool(torch.equal(sel.int(), people.neighbours))
            print(f"  {name}: members inside a {a.square} m square; all-zero triples {100 * zero:.1f} %; the torch formulation picks the same "
                  f"neighbours: {same}; largest difference of the rows {float((rows - obs[:, -165:]).abs().max()):.2e}")
        else:
            print(f"  {name}: every root of a group at one point; all-zero triples {100 * zero:.1f} % (the neighbours' roots minus the env's own)")
        ids = torch.arange(0, E, 16, dtype=torch.int32, device=dev)
        t_all, t_ids, t_torch = timed(people.run, a.iters), timed(lambda: people.run(ids), a.iters), timed(lambda: torch_people(rb, a.group, bodies), a.iters)
        print(f"    emloco_task_crowd_people, all rows (two launches)      {t_all * 1e3:9.1f} us")
        print(f"    emloco_task_crowd_people, an id list of {ids.numel():4d} envs      {t_ids * 1e3:9.1f} us")
        print(f"    torch formulation (distance tensor, topk, gathers)     {t_torch * 1e3:9.1f} us  = {t_torch / t_all:.1f} x the kernel")
        out[name] = t_all
    return out


def part2(a):
    import emloco_amd
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group_obs.yaml")
    args = get_args(["--num_envs", str(a.envs), "--seed", "3", "--cfg_env", cfg_env] + (["--small_terrain"] if a.small_terrain else []))
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(num_env_group=a.group)
    env = create_rlgpu_env(args, cfg, cfg_train)
    task = env.task
    bundle = AMPPolicyBundle(task, deterministic=True)
    net = ValuePoseNet(use_pose=True, use_vel=True).to(task.device).eval()
    ev = LocoValEvaluator(RLGPUEnv(env), bundle, net, 4 * a.envs)
    for _ in range(8):                                              # warm-up: the first reset of all envs, the first launches
        ev.step_once()
    torch.cuda.synchronize()
    n = 4 * a.test_steps
    t0 = time.time()
    for _ in range(n):
        ev.step_once()
    torch.cuda.synchronize()
    step_ms = (time.time() - t0) / n * 1e3
    t_call = timed(task._people.run, a.iters)
    print(f"--test loop, pacer_group_obs.yaml at {a.envs} envs in groups of {a.group}{' (small terrain)' if a.small_terrain else ''}, "
          f"sept policy with the people branch ({type(bundle.frozen).__name__}), {n} steps:")
    print(f"  {step_ms:8.3f} ms per step = {a.envs / step_ms * 1e3:10,.0f} env-steps/s; emloco_task_crowd_people on the loop's last state "
          f"{t_call * 1e3:.1f} us = {100.0 * t_call / step_ms:.2f} % of the step")


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("envs", 2048), ("group", 512), ("iters", 200), ("test_steps", 64)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--square", type=float, default=40.0)
    ap.add_argument("--small_terrain", action="store_true")
    a = ap.parse_args()
    L.require_device()
    part1(a)
    if a.test_steps > 0:
        part2(a)


if __name__ == "__main__":
    main()

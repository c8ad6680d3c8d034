#!/usr/bin/env python3
"""Time of the crowd contact audit on the device (profiles/crowd_contacts.txt).

    python tools/crowd_contacts_timing.py [--envs 2048] [--group 512] [--square 40] [--iters 200] [--test_steps 64] [--small_terrain]

Part 1, synthetic state: the members of every group stand at random places inside a `--square` m square (the crowd sensor's timing
shape, tools/crowd_sensor_timing.py), bodies at their bind-pose offsets with a random rotation each, the capsule table of
pack_self_collision for two scaled SMPL models alternating.  HIP events around `--iters` calls after a warm-up, on one stream: the
geometry (emloco_crowd_contacts: two launches) and the bookkeeping (emloco_crowd_contacts_accumulate with epoch totals) on their own.
Part 2, the shipped crowd configuration (pacer_group.yaml, random-init CNN policy and LocoVal): the step rate of the --test loop with and
without --eval_crowd, two evaluators on one env alternated in blocks of `--test_steps` steps in one process (`--test_steps 0`: skipped)."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emloco_amd import _lib as L  # noqa: E402
from emloco_amd.crowd_contacts import CrowdContactAudit  # noqa: E402
from emloco_amd.model import pack_self_collision, smpl_humanoid  # noqa: E402

SENSOR_US = 116.2           # profiles/crowd_sensor.txt: emloco_task_crowd_sensor, all rows, at 2048 envs in groups of 512


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


def synthetic(E, group, square, rng):
    base = smpl_humanoid()
    models = [base.scaled(0.92, 0.9) if e % 2 else base.scaled(1.06, 1.1) for e in range(E)]
    sc = pack_self_collision(models)
    rb = np.zeros((E, 24, 13), np.float32)
    centre = rng.uniform(40, 140, (E // group, 2)).repeat(group, 0)
    root = np.concatenate([centre + rng.uniform(-square / 2, square / 2, (E, 2)), np.full((E, 1), 0.95)], axis=1)
    for e, m in enumerate(models):
        p = np.zeros((24, 3))
        for i in range(1, 24):
            p[i] = p[m.parent[i]] + m.joint_off[i]
        rb[e, :, :3] = root[e] + p
    q = rng.normal(size=(E, 24, 4))
    rb[:, :, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return sc, rb


def part1(a):
    dev = torch.device("cuda")
    rng = np.random.default_rng(1)
    E = a.envs
    sc, rb = synthetic(E, a.group, a.square, rng)
    rb = torch.from_numpy(rb).to(dev)
    task = types.SimpleNamespace(_divide_group=True, _group_num_people=a.group, num_envs=E, device=dev,
                                 sim=types.SimpleNamespace(native=types.SimpleNamespace(_sc=sc, rigid_body_state=rb)))
    audit = CrowdContactAudit(task, near_dist=1.0, totals=True)
    done = torch.zeros(E, dtype=torch.int64, device=dev)
    audit.step(done=done)
    now = audit.now()
    print(f"crowd contact audit, {E} envs in groups of {a.group}, {audit.n_seg} segments, members inside a {a.square} m square, near_dist 1.0")
    print(f"  root tests per call: {E * (a.group - 1)}; envs in contact: {int((now['n_pen'] > 0).sum())}, contacts: {int(now['n_pen'].sum())}, "
          f"members nearer than near_dist: {int(now['n_near'].sum())}, deepest penetration {now['pen'].max():.3f} m, "
          f"mean nearest {now['nearest'].mean():.2f} m")
    st = torch.cuda.current_stream().cuda_stream
    import ctypes as C
    acc = lambda: L.check(audit.lib.emloco_crowd_contacts_accumulate(C.byref(audit.bufs), audit._now.data_ptr(), C.c_void_p(st)), "accumulate")
    t_geo, t_acc, t_both = timed(audit.geometry, a.iters), timed(acc, a.iters), timed(lambda: audit.step(done=done), a.iters)
    print(f"HIP events, mean of {a.iters} calls after 10 warm-up calls:")
    print(f"  emloco_crowd_contacts (segments + pairs: two launches)   {t_geo * 1e3:9.1f} us")
    print(f"  emloco_crowd_contacts_accumulate (with epoch totals)     {t_acc * 1e3:9.1f} us")
    print(f"  both, as one step of the audit                           {t_both * 1e3:9.1f} us")
    print(f"  the sensor it audits (profiles/crowd_sensor.txt)         {SENSOR_US:9.1f} us -> the audit costs {t_both * 1e3 / SENSOR_US:.2f} x the sensor")


def part2(a):
    import yaml
    import emloco_amd
    from emloco_amd.learning.amp_policy import CNN_CFG, AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    args = get_args(["--num_envs", str(a.envs), "--seed", "3", "--cfg_env", cfg_env] + (["--small_terrain"] if a.small_terrain else []))
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(num_env_group=a.group)
    env = create_rlgpu_env(args, cfg, cfg_train)
    task = env.task
    bundle = AMPPolicyBundle(task, cfg_train=yaml.safe_load(open(CNN_CFG)), deterministic=True)
    net = ValuePoseNet(use_pose=True, use_vel=True).to(task.device).eval()
    evs = {on: LocoValEvaluator(RLGPUEnv(env), bundle, net, 4 * a.envs, crowd=on) for on in (False, True)}
    for ev in evs.values():                                         # warm-up: the first reset of all envs, the first launches
        for _ in range(8):
            ev.step_once()
    torch.cuda.synchronize()
    spent = {False: 0.0, True: 0.0}
    blocks = 4
    for _ in range(blocks):
        for on in (False, True):
            t0 = time.time()
            for _ in range(a.test_steps):
                evs[on].step_once()
            torch.cuda.synchronize()
            spent[on] += time.time() - t0
    n = blocks * a.test_steps
    off_ms, on_ms = spent[False] / n * 1e3, spent[True] / n * 1e3
    print(f"--test loop, pacer_group.yaml at {a.envs} envs in groups of {a.group}{' (small terrain)' if a.small_terrain else ''}, "
          f"{blocks} blocks of {a.test_steps} steps each way, alternated:")
    print(f"  without --eval_crowd  {off_ms:8.3f} ms per step = {a.envs / off_ms * 1e3:10,.0f} env-steps/s")
    print(f"  with --eval_crowd     {on_ms:8.3f} ms per step = {a.envs / on_ms * 1e3:10,.0f} env-steps/s  ({100.0 * (on_ms / off_ms - 1.0):+.1f} %)")
    audit = evs[True].crowd
    now = audit.now()
    t_geo = timed(audit.geometry, a.iters)
    print(f"  the loop's last state: envs in contact {int((now['n_pen'] > 0).sum())}, contacts {int(now['n_pen'].sum())}, members nearer than "
          f"near_dist {int(now['n_near'].sum())}, mean nearest {now['nearest'].mean():.2f} m; emloco_crowd_contacts on it {t_geo * 1e3:9.1f} us")


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

#!/usr/bin/env python3
"""Time of the crowd spawn on the device (profiles/crowd_spawn.txt).

    python tools/crowd_spawn_timing.py [--envs 2048] [--group 512] [--ids 78] [--iters 200] [--test_steps 64] [--small_terrain]

Part 1, a flat walkable field: HIP events around `--iters` calls of emloco_task_crowd_spawn (two launches) after a warm-up, on one
stream, with uniforms drawn beforehand -- the full first reset (every env listed: `--group` dependent rounds in each group's
workgroup) and a steady-state call of `--ids` envs on the crowd the full reset left (about `--ids` / groups rounds per workgroup).
Beside them the same two calls through `CrowdSpawn.run`, which also draws the uniforms and adds up the totals with torch ops.
Part 2, pacer_group.yaml with a random-init CNN policy and LocoVal under `--test --eval_crowd`: the step time of the loop with and
without group_spawn, the audit's share of games that started in contact and the spawn's totals (`--test_steps 0`: skipped)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emloco_amd import _lib as L  # noqa: E402
from emloco_amd.crowd_spawn import CrowdSpawn, auto_extent, report_line  # noqa: E402


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


def part1(a):
    dev = torch.device("cuda")
    E, gs = a.envs, a.group
    ext = auto_extent(gs, 1.0)
    side = 2 * (ext + 10.0) + 20.0
    cells = int(side / 0.1)
    roots = torch.zeros((E, 13), device=dev)
    roots[:, 0], roots[:, 1] = 50.0, 55.0                            # every env on the one fixed spot, as the parent's reset leaves them
    sp = CrowdSpawn(roots=roots, n_env=E, group_size=gs, walkable=torch.zeros((cells, cells), dtype=torch.int16), hscale=0.1, min_dist=1.0,
                    tries=8, extent=ext, centre=(side / 2, side / 2), margin=10.0)
    lib, st = sp.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.manual_seed(1)
    u_all = torch.rand((E, 8, 2), device=dev)
    ids = torch.from_numpy(np.sort(np.random.default_rng(1).choice(E, a.ids, replace=False)).astype(np.int32)).to(dev)
    u_ids = torch.rand((a.ids, 8, 2), device=dev)

    def raw(id_t, u):
        L.check(lib.emloco_task_crowd_spawn(C.byref(sp.bufs), None if id_t is None else C.c_void_p(id_t.data_ptr()),
                                            0 if id_t is None else id_t.numel(), C.c_void_p(u.data_ptr()), st), "emloco_task_crowd_spawn")

    print(f"crowd spawn, {E} envs in groups of {gs}, 8 tries, min_dist 1.0 m, extent {ext:.1f} m; HIP events, mean of {a.iters} calls after 10 "
          "warm-up calls")
    t_full = timed(lambda: raw(None, u_all), a.iters)
    sp.run(None, u_all)
    t = sp.totals(clear=True)
    print("  " + report_line(t))
    roots[:, :2] = sp.place_xy                                       # the crowd stands where the full reset put it
    t_ids = timed(lambda: raw(ids, u_ids), a.iters)
    per_group = np.bincount(ids.cpu().numpy() // gs, minlength=E // gs)
    print(f"    emloco_task_crowd_spawn, full first reset ({gs} rounds per workgroup)        {t_full * 1e3:9.1f} us")
    print(f"    emloco_task_crowd_spawn, an id list of {a.ids} envs ({per_group.min()}..{per_group.max()} rounds per workgroup) {t_ids * 1e3:9.1f} us")
    t_full_py, t_ids_py = timed(lambda: sp.run(None), a.iters), timed(lambda: sp.run(ids), a.iters)
    print(f"    CrowdSpawn.run (torch.rand, the call, the totals), full / id list            {t_full_py * 1e3:9.1f} / {t_ids_py * 1e3:.1f} us")


def evaluation(a, spawn):
    import emloco_amd
    import yaml
    from emloco_amd.learning.amp_policy import CNN_CFG, AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    args = get_args(["--num_envs", str(a.envs), "--seed", "3", "--cfg_env", cfg_env] + (["--small_terrain"] if a.small_terrain else []))
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(num_env_group=a.group, group_spawn=spawn)
    env = create_rlgpu_env(args, cfg, cfg_train)
    task = env.task
    bundle = AMPPolicyBundle(task, cfg_train=yaml.safe_load(open(CNN_CFG)), deterministic=True)
    net = ValuePoseNet(use_pose=True, use_vel=True).to(task.device).eval()
    ev = LocoValEvaluator(RLGPUEnv(env), bundle, net, 4 * a.envs, crowd=True)
    for _ in range(8):                                              # warm-up: the first reset of all envs, the first launches
        ev.step_once()
    torch.cuda.synchronize()
    n = 4 * a.test_steps
    t0 = time.time()
    for _ in range(n):
        ev.step_once()
    torch.cuda.synchronize()
    step_ms = (time.time() - t0) / n * 1e3
    rep = ev.report(say=None)
    return step_ms, n, rep["crowd"], None if task._spawn is None else task._spawn.totals()


def part2(a):
    print(f"--test --eval_crowd loop, pacer_group.yaml at {a.envs} envs in groups of {a.group}{' (small terrain)' if a.small_terrain else ''}, "
          "random-init CNN policy:")
    for spawn in (False, True):
        step_ms, n, crowd, totals = evaluation(a, spawn)
        print(f"  group_spawn {str(spawn):5s}: {step_ms:8.3f} ms per step over {n} steps = {a.envs / step_ms * 1e3:10,.0f} env-steps/s; "
              f"{crowd['games']} games, started in contact {100 * crowd['start_contact_share']:.2f} %")
        if totals is not None:
            print("    " + report_line(totals))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("envs", 2048), ("group", 512), ("ids", 78), ("iters", 200), ("test_steps", 64)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--small_terrain", action="store_true")
    a = ap.parse_args()
    L.require_device()
    part1(a)
    if a.test_steps > 0:
        part2(a)


if __name__ == "__main__":
    main()

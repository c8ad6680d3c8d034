"""Cost of the LocoVal evaluation's bookkeeping per step (`run.py --test`, learning/locoval_eval.py).

    python tools/locoval_eval_overhead.py [--num_envs 4096] [--steps 200] [--rounds 3]

Times the evaluation step at E envs (reset_done -> deterministic policy -> env.step -> discriminator reward) WITHOUT and WITH the
three launches of the bookkeeping (emloco_locoval_eval_step, emloco_locoval_fwd_rows, emloco_locoval_eval_finish), interleaved over
several rounds, wall time per step between two device synchronisations; then the three launches alone (device time of a
repeated launch sequence, hipEvents).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import emloco_amd
    emloco_amd.configure_runtime()
    import torch
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(a.num_envs), "--seed", "1", "--random_heading", "--init_heading", "--heading_inversion",
                     "--adjust_root_vel"])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    env = RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))
    task = env.env.task
    dev = torch.device(task.device)
    torch.manual_seed(0)
    bundle = AMPPolicyBundle(task, deterministic=True)
    ev = LocoValEvaluator(env, bundle, ValuePoseNet(True, True).to(dev), games_num=64 * a.num_envs)     # more games than these steps finish

    def plain_step():
        with torch.no_grad():
            env.env.reset_done()
            actions = bundle.frozen.act(task.obs_buf, deterministic=True)
            _o, _r, _d, infos = env.step(actions)
            bundle.disc_reward(infos["amp_obs"])

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for _ in range(a.warmup):
        ev.step_once()
    rounds = []
    for _ in range(a.rounds):
        rounds.append({"without_ms": timed(plain_step, a.steps), "with_ms": timed(ev.step_once, a.steps)})
    # the three launches alone, on this step's inputs, repeated (device time between two events)
    rr, dones, term, inv = task.reward_raw, task.reset_buf, task._terminate_buf, task.inverted
    disc = torch.zeros(a.num_envs, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 500
    launch_us = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            ev._launch(rr, disc, dones, term, inv)
        e1.record()
        torch.cuda.synchronize()
        launch_us.append(e0.elapsed_time(e1) / reps * 1e3)
    w = statistics.median(r["without_ms"] for r in rounds)
    v = statistics.median(r["with_ms"] for r in rounds)
    print(json.dumps({"num_envs": a.num_envs, "steps": a.steps, "rounds": rounds, "step_without_ms": w, "step_with_ms": v,
                      "overhead_us": (v - w) * 1e3, "three_launches_device_us": statistics.median(launch_us)}))


if __name__ == "__main__":
    main()

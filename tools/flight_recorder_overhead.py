"""Cost of the flight recorder per rollout step (`run.py --capture`, learning/flight_recorder.py).

    python tools/flight_recorder_overhead.py [--num_envs 4096] [--steps 200] [--rounds 5] [--depth 8] [--parent_file OLD/locoval_rollout.py]

The method of tools/episode_stats_overhead.py: `LocoValRollout.step_once` (the headline loop of bench.py: pre-sampled noise actions,
horizon 32, one end_epoch per horizon) at E envs between two device synchronisations, in windows of `--steps` steps, for up to three
loop objects on ONE env taking turns in one process: this tree with the recorder off, this tree with it on at `--depth` (drained once
per horizon, as the driver does) and -- with `--parent_file`, the learning/locoval_rollout.py of another commit, loaded as a module of
this package beside the current one -- that commit's loop.  A loop is attached to the task ahead of its window and detached behind it,
outside the timed region.  Then the launches alone, hipEvents around runs of calls: `record` and `check` back to back, `record` alone
(one launch) and `check` alone (three).  Prints one JSON line.

A timing tool only: the loops share one env, and the repeated launches at the end record and check step after step of an env that
stands still (the triggers are off for them).  Neither changes what a launch costs; the numbers these loops keep mean nothing and go with the process.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--parent_file", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import emloco_amd
    emloco_amd.configure_runtime()
    import numpy as np
    import torch
    from emloco_amd.learning.flight_recorder import FlightRecorder
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    classes = {"off": LocoValRollout, "on": LocoValRollout}
    if a.parent_file:
        spec = importlib.util.spec_from_file_location("emloco_amd.learning._parent_locoval_rollout", a.parent_file)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        classes["parent"] = mod.LocoValRollout
    args = get_args(["--num_envs", str(a.num_envs), "--seed", "0", "--random_heading", "--init_heading", "--heading_inversion",
                     "--adjust_root_vel", "--input_init_pose", "--input_init_vel"])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    env = RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))
    task = env.env.task
    dev = torch.device(task.device)
    E, horizon = a.num_envs, 32
    task.sim.native.set_cost_order(True)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    pool = torch.randn(64, E, 69, device=dev, generator=g) * float(np.exp(-2.9))
    counter = [0]

    def noise_policy(obs):
        counter[0] += 1
        return pool[counter[0] % 64]

    agents = {}
    for name, cls in classes.items():
        torch.manual_seed(0)
        agents[name] = cls(env, horizon_length=horizon, policy=noise_policy, overlap_reset=False)
        agents[name]._sched_live = True                    # (the schedule's first-episode check is a host read; not in the timed loop)
        agents[name].detach()
    rec = FlightRecorder(task, depth=a.depth, slots=16, speed=50.0, early_fall=10)

    def window(name, n):
        agent = agents[name]
        agent.attach()
        if name == "on":
            agent.attach_flight_recorder(rec)
        for k in range(8):                                 # (the hand-over between loops is not part of the window)
            agent.step_once()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            agent.step_once()
            if (k + 1) % horizon == 0:
                agent.end_epoch()
                if name == "on":
                    rec.drain()                            # the epoch's read of the counters (and of the used slots) belongs to the cost
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        if name == "on":
            agent.attach_flight_recorder(None)
        agent.detach()
        return ms

    for name in agents:
        window(name, a.warmup)
    rounds = [{name: window(name, a.steps) for name in agents} for _ in range(a.rounds)]
    out = {"num_envs": E, "steps": a.steps, "depth": a.depth, "rounds": rounds}
    for name in agents:
        ms = [r[name] for r in rounds]
        out[f"step_{name}_ms"] = statistics.median(ms)
        out[f"spread_{name}_us"] = (max(ms) - min(ms)) * 1e3
    out["added_us"] = (out["step_on_ms"] - out["step_off_ms"]) * 1e3
    if "parent" in agents:
        ms = [r["parent"] for r in rounds]
        out["off_inside_parent_spread"] = bool(min(ms) <= out["step_off_ms"] <= max(ms))
    rec.cause_mask = 0                                     # the launches alone: no trigger, so no slot fills up over the repeats
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 500

    def timed(calls):
        us = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                calls()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / reps * 1e3)
        return statistics.median(us)

    def pair():
        rec.record()
        rec.check()

    def check_only():                                      # (check() wants a record() for its step: claimed here without the launch)
        rec._recorded = rec.t
        rec.check()
    rec.record()
    out["record_check_device_us"] = timed(pair)
    out["record_device_us"] = timed(rec.record)            # one launch
    out["check_device_us"] = timed(check_only)             # three launches
    out["check_per_launch_us"] = out["check_device_us"] / 3.0
    t0 = time.perf_counter()
    for _ in range(2000):
        rec.bufs()
    out["bufs_host_us"] = (time.perf_counter() - t0) / 2000 * 1e6      # the host's share per call: refreshing the structure
    print(json.dumps(out))


if __name__ == "__main__":
    main()

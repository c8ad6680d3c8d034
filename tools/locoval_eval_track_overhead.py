"""Cost of the evaluation's path tracking per step (`run.py --test --eval_tracks`, learning/locoval_eval.py).

    python tools/locoval_eval_track_overhead.py [--num_envs 4096] [--steps 200] [--rounds 5] [--root OTHER_TREE --plain_only]

Times the evaluation loop's step (`LocoValEvaluator.step_once`: reset_done -> deterministic policy -> env.step -> discriminator reward
-> the bookkeeping launches) at E envs WITHOUT and WITH `track=True`, two evaluators on one env taking turns over several rounds, wall
time per step between two device synchronisations; then the tracking launch alone (device time of a repeated launch, hipEvents).
`--root` imports the package from another checkout (a baseline build of an older commit; `--plain_only` where it has no `track`).
Prints one JSON line.

A timing tool only: the two evaluators share one env, so during the other's turns an evaluator's per-game state (steps, games, the
tracker's prev_xy and sums) falls out of step with the env's progress_buf, and the repeated launch at the end accumulates the same step
500 times into live game state.  Neither changes what a launch costs; the records of these evaluators mean nothing and they are
discarded with the process.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plain_only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
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
    net = ValuePoseNet(True, True).to(dev)
    games = 64 * a.num_envs                                      # more games than these steps finish: every step records
    evs = {"plain": LocoValEvaluator(env, bundle, net, games_num=games)}
    if not a.plain_only:
        evs["track"] = LocoValEvaluator(env, bundle, net, games_num=games, track=True)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for ev in evs.values():
        for _ in range(a.warmup):
            ev.step_once()
    rounds = [{k: timed(ev.step_once, a.steps) for k, ev in evs.items()} for _ in range(a.rounds)]
    out = {"root": os.path.abspath(a.root), "num_envs": a.num_envs, "steps": a.steps, "rounds": rounds,
           "step_plain_ms": statistics.median(r["plain"] for r in rounds)}
    if not a.plain_only:
        import ctypes as C
        from emloco_amd.predictor import ops
        from emloco_amd.sim import current_stream_handle
        ev = evs["track"]
        out["step_track_ms"] = statistics.median(r["track"] for r in rounds)
        out["overhead_us"] = (out["step_track_ms"] - out["step_plain_ms"]) * 1e3
        P = lambda t: C.c_void_p(t.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lib, st, reps, us = ops._lib(), current_stream_handle(dev), 500, []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                ops._chk(lib.emloco_locoval_eval_track(C.byref(ev._s), C.byref(ev._track_inputs()), P(ev._track_records), P(ev._track_samples), st),
                         "emloco_locoval_eval_track")
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / reps * 1e3)
        out["track_launch_device_us"] = statistics.median(us)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

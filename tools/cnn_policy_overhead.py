"""Cost of the CNN policy of the crowd sensor per step (learning/policy_runner.py: CnnFrozenPolicy, csrc/cnn_kernels.hip).

    python tools/cnn_policy_overhead.py [--num_envs 4096] [--reps 200] [--rounds 5]

At E envs with the shape of data/cfg/pacer_group.yaml (rows of 368 + 30 + 3 * 64 * 64 values, full network widths, random weights and
observations -- no simulator is built) it times, as device time between two events around `reps` back-to-back calls, `rounds` times
after a warm-up: the trunk kernel alone (emloco_cnn_trunk), CnnFrozenPolicy.act_mean whole, and for comparison FrozenPolicy.act_mean
on the default task's rows (368 + 30 + 1024) of the same build.  The calls alternate between two observation buffers (2 x 208 MB at
4096 envs, more than the chip's last-level cache), so the map is read from HBM as in a rollout.  Prints one JSON line: the median of
the rounds and their spread (min, max) per figure.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import emloco_amd
    emloco_amd.configure_runtime()
    import torch
    import yaml
    from emloco_amd.learning.amp_policy import CNN_CFG, DEFAULT_CFG, network_classes
    from emloco_amd.utils.running_mean_std import RunningMeanStd
    dev, E = torch.device("cuda:0"), a.num_envs
    torch.manual_seed(0)

    def runner(cfg_path, detail):
        params = yaml.safe_load(open(cfg_path))["params"]["network"]
        builder_cls, runner_cls = network_classes(params["name"])
        task_size = sum(detail.values())
        rms = RunningMeanStd((368 + task_size,)).to(dev).eval()
        b = builder_cls()
        b.load(params)
        net = b.build("amp", actions_num=69, input_shape=(368 + task_size,), num_seqs=1, value_size=1, amp_input_shape=(3090,), self_obs_size=368,
                      task_obs_size=task_size, task_obs_size_detail=detail, mean_std=rms).to(dev).eval()
        obs = [torch.randn(E, 368 + task_size, device=dev) for _ in range(2)]
        return runner_cls(net, rms, E, dev), obs

    def timed(fn, obs):
        for i in range(a.warmup):
            fn(obs[i & 1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.reps):
                fn(obs[i & 1])
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    cnn, cnn_obs = runner(CNN_CFG, {"traj": 30, "heightmap_velocity": 3 * 64 * 64})
    out = {"num_envs": E, "reps": a.reps, "rounds": a.rounds, "trunk": timed(cnn.trunk, cnn_obs), "cnn_policy": timed(cnn.act_mean, cnn_obs),
           "trunk_gflop": 2e-9 * cnn.trunk_macs * E, "map_mbytes": 4e-6 * E * 3 * 64 * 64}
    del cnn, cnn_obs
    sept, sept_obs = runner(DEFAULT_CFG, {"traj": 30, "heightmap": 1024})
    out["sept_policy"] = timed(sept.act_mean, sept_obs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

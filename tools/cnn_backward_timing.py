"""Cost of the CNN trunk's backward next to its forward (csrc/cnn_backward_kernels.hip, csrc/cnn_kernels.hip).

    python tools/cnn_backward_timing.py [--rows 2560 10240] [--reps 200] [--rounds 5] [--train_envs 2048 [--epochs 2]]

At the shipped shape (64 x 64 x 3 map, three layers of 16 filters) and `rows` map rows -- 2 560 is the PPO minibatch, 10 240 the
stacked actor evaluation of one optimiser step -- it times, as device time between two events around `reps` back-to-back calls,
`rounds` times after a warm-up: emloco_cnn_trunk alone (normalisation off, as the training module calls it) and
emloco_cnn_trunk_backward (both launches, the workspace allocated once outside the loop).  The calls alternate between two map
buffers (2 x 126 MB at 2 560 rows), so the map is read from HBM as in a training step.  Random weights, maps and feature gradients; no
simulator is built.  Prints one JSON line: per row count the median of the rounds and their spread (min, max) per figure, and the
backward as a multiple of the forward.

--train_envs E adds what `run.py --train_policy --cnn_backward` costs on data/cfg/pacer_group.yaml at E envs, measured as bench.py's
`policy.ppo` leg measures the sept configuration: one warm-up `AMPAgent.train_epoch` (eager steps, the graph's capture), then `epochs`
timed ones; fps_total = frames / total_time and the update time per optimiser step (the captured graph's replay).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train_leg(E, epochs):
    import torch
    import yaml
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.amp_policy import CNN_CFG
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(E), "--seed", "0", "--cfg_env", os.path.join(ROOT, "emloco_amd", "data", "cfg", "pacer_group.yaml")])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    env = RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))
    pol = yaml.safe_load(open(CNN_CFG))
    c = pol["params"]["config"]
    batch, mb_cfg = int(c["horizon_length"]) * E, int(c["minibatch_size"])
    if batch % mb_cfg:                                       # (bench.py's rule: the largest divisor of the batch below the configured size)
        c["minibatch_size"] = max(d for d in range(1, mb_cfg + 1) if batch % d == 0)
    agent = AMPAgent(env, pol)
    agent.train_epoch()
    infos = [agent.train_epoch() for _ in range(epochs)]
    torch.cuda.synchronize()
    play, total = sum(i["play_time"] for i in infos), sum(i["total_time"] for i in infos)
    steps = agent.mini_epochs_num * (agent.batch_size // agent.minibatch_size)
    return {"num_envs": E, "epochs_timed": epochs, "batch_size": agent.batch_size, "minibatch_size": agent.minibatch_size,
            "optimizer_steps_per_epoch": steps, "fps_step": agent.batch_size * epochs / play, "fps_total": agent.batch_size * epochs / total,
            "update_ms_per_optimizer_step": (total - play) / epochs / steps * 1e3,
            "optimizer_step_as_hip_graph": bool(agent.use_graph and agent._graph is not None),
            "finite": bool(all(torch.isfinite(p).all() for p in agent.a2c_network.parameters()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2560, 10240])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train_envs", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=2)
    a = ap.parse_args()
    import emloco_amd
    emloco_amd.configure_runtime()
    import torch
    from emloco_amd.learning.amp_network_sept_cnn_builder import cnn_trunk
    from emloco_amd.predictor import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res, ch, filters = 64, 3, (16, 16, 16)
    count, cin = 0, ch
    for f in filters:
        count, cin = count + f * cin * 16 + f, f
    features = filters[-1] * (res >> len(filters)) ** 2
    params = (torch.randn(count, device=dev) * 0.08).contiguous()
    lib = ops._lib()

    def timed(fn, bufs):
        for i in range(a.warmup):
            fn(bufs[i & 1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.reps):
                fn(bufs[i & 1])
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    out = {"shape": [res, res, ch], "filters": list(filters), "reps": a.reps, "rounds": a.rounds, "rows": {}}
    for rows in a.rows:
        maps = [torch.randn(rows, ch * res * res, device=dev).clamp_(-5.0, 5.0) for _ in range(2)]
        feat = torch.empty(rows, features, device=dev)
        dout = torch.randn(rows, features, device=dev)
        n_ws = lib.emloco_cnn_trunk_backward_workspace(rows, res, ch, len(filters), *filters, 0)
        workspace, dparams = torch.empty(n_ws, device=dev), torch.empty(count, device=dev)

        def forward(x):
            cnn_trunk(x, 0, res, ch, filters, params, feat)

        def backward(x):
            rc = lib.emloco_cnn_trunk_backward(rows, res, ch, len(filters), *filters, 0, ops._p(x), x.stride(0), None, None, C.c_float(1e-5),
                                               C.c_float(5.0), 0, ops._p(params), ops._p(dout), dout.stride(0), 0, ops._p(dparams),
                                               ops._p(workspace), n_ws, ops._st(x))
            ops._chk(rc, "emloco_cnn_trunk_backward")

        fwd, bwd = timed(forward, maps), timed(backward, maps)
        assert torch.isfinite(dparams).all()
        out["rows"][str(rows)] = {"forward": fwd, "backward": bwd, "backward_over_forward": bwd["median_ms"] / fwd["median_ms"],
                                  "map_mbytes": 4e-6 * rows * ch * res * res}
        del maps, feat, dout, workspace
    if a.train_envs:
        torch.cuda.empty_cache()
        out["train_policy_cnn_backward"] = train_leg(a.train_envs, a.epochs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

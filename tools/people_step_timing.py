"""Cost of one captured optimiser step of the people network (the sept network with the group observation's `people` block).

    python tools/people_step_timing.py [--rows 2560] [--reps 50] [--rounds 5]

Builds AMPAgent at the shipped widths on a stand-in task (no simulator): observation rows [self 368 | path 30 | map 1024 | people 165],
15 AMP steps of 206, the symmetry loss on, one minibatch of `rows` random rows as the whole dataset.  After three eager warm-up steps
the step is captured twice, as one chain and with its arms (AMPAgent._capture), and each graph is timed as device time between two
events around `reps` back-to-back replays, `rounds` times.  Every replay is a real step (the statistics and the weights move).  Prints
one JSON line: per form the median of the rounds and their spread (min, max) in ms per step.  Run it on two trees to compare them.
"""
import argparse
import collections
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SELF, TRAJ, MAP, PEOPLE, ACTIONS, AMP_STEPS, AMP_ROW = 368, 30, 1024, 165, 69, 15, 206


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2560)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import emloco_amd
    emloco_amd.configure_runtime()
    import torch
    import yaml
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.amp_policy import DEFAULT_CFG
    dev = "cuda:0"
    obs_w, amp_w, horizon = SELF + TRAJ + MAP + PEOPLE, AMP_STEPS * AMP_ROW, 32
    assert a.rows % horizon == 0

    class Task:
        def __init__(self):
            self.num_envs, self.device, self.num_actions = a.rows // horizon, dev, ACTIONS
            self._num_amp_obs_steps, self.motion_sym_loss, self.cfg, self.task = AMP_STEPS, True, {"env": {}}, self
            self.left_to_right_index_action = [4, 5, 6, 7, 0, 1, 2, 3, 8, 9, 10, 11, 12, 18, 19, 20, 21, 22, 13, 14, 15, 16, 17]

        def get_obs_size(self): return obs_w
        def get_self_obs_size(self): return SELF
        def get_num_amp_obs(self): return amp_w
        def get_task_obs_size_detail(self): return collections.OrderedDict([("traj", TRAJ), ("heightmap", MAP), ("people", PEOPLE)])
        def fetch_amp_obs_demo(self, n): return torch.randn(n, amp_w, device=dev)

    torch.manual_seed(0)
    cfg = yaml.safe_load(open(DEFAULT_CFG))
    cfg["params"]["config"].update(horizon_length=horizon, minibatch_size=a.rows, amp_minibatch_size=a.rows, amp_batch_size=256,
                                   amp_obs_demo_buffer_size=4096, amp_replay_buffer_size=4096)
    agent = AMPAgent(Task(), cfg)
    assert agent.a2c_network.has_people and agent.use_graph and agent.batch_size == agent.minibatch_size == a.rows
    r = lambda *s: torch.randn(*s, device=dev)
    N = a.rows
    agent.dataset = {"old_values": r(N, 1), "old_logp_actions": r(N) * 0.1 - 100, "advantages": r(N), "returns": r(N, 1),
                     "actions": r(N, ACTIONS) * 0.05, "obs": r(N, obs_w), "mu": r(N, ACTIONS) * 0.05,
                     "sigma": torch.full((N, ACTIONS), math.exp(-2.9), device=dev), "amp_obs": r(N, amp_w), "amp_obs_demo": r(N, amp_w),
                     "amp_obs_replay": r(N, amp_w), "flip_obs": r(N, obs_w), "next_obses": r(N, obs_w)}
    for _ in range(3):
        agent._graph_step(0)
    torch.cuda.synchronize()
    out = {"rows": N, "reps": a.reps, "rounds": a.rounds, "forms": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, arms in (("one_chain", False), ("arms", True)):
        g = agent._capture(arms)
        for _ in range(5):
            agent._replay(g)
        ms = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                agent._replay(g)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        out["forms"][name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    out["finite"] = bool(all(torch.isfinite(p).all() for p in agent.a2c_network.parameters()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

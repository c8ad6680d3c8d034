"""What tests/test_cnn_policy_cpu.py and tests/test_gpu_cnn_policy.py share -- TEST INFRASTRUCTURE ONLY: the CNN network built from the
shipped configuration at a fixture's widths, loaded from the fixture, on a device of the caller's choice; `close`, the bar of
tests/test_gpu_policy.py for this network family (1e-4 of the tensor's max + 1e-5)."""
import copy
import os

import numpy as np
import torch
import yaml

import emloco_amd

CFG = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "train", "rlg", "amp_humanoid_smpl_cnn_task.yaml")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("cnn_policy_net_r16", "cnn_policy_net_r32")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def params(units=(2048, 1024), task_units=(512, 256), disc_units=(1024, 512)):
    p = copy.deepcopy(yaml.safe_load(open(CFG))["params"]["network"])
    p["mlp"]["units"], p["task_mlp"]["units"], p["disc"]["units"] = list(units), list(task_units), list(disc_units)
    return p


def build(device, net_params, self_size, traj, kind, map_size, amp=3090, actions=69):
    from emloco_amd.learning.amp_network_sept_cnn_builder import AMPSeptCNNBuilder
    from emloco_amd.utils.running_mean_std import RunningMeanStd
    obs_size = self_size + traj + map_size
    rms = RunningMeanStd((obs_size,)).to(device)
    rms.eval()
    b = AMPSeptCNNBuilder()
    b.load(net_params)
    net = b.build("amp", actions_num=actions, input_shape=(obs_size,), num_seqs=1, value_size=1, amp_input_shape=(amp,), self_obs_size=self_size,
                  task_obs_size=traj + map_size, task_obs_size_detail={"traj": traj, kind: map_size}, mean_std=rms).to(device).eval()
    return net, rms


def build_from(g, device):
    """(network, normaliser) of a fixture, loaded with strict=True"""
    self_size, task_size, amp, actions = (int(v) for v in g["sizes"])
    traj = int(g["traj"])
    net, rms = build(device, params(g["units"], g["task_units"], g["disc_units"]), self_size, traj, str(g["kind"]), task_size - traj, amp, actions)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    rms.running_mean.copy_(torch.from_numpy(g["running_mean"]))
    rms.running_var.copy_(torch.from_numpy(g["running_var"]))
    return net, rms


def close(a, b, rel=1e-4, abs_=1e-5, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = abs_ + rel * np.abs(b).max()
    err = np.abs(a - b).max()
    print(f"{what}: max err {err:.3e}, bar {tol:.3e}")
    assert a.shape == b.shape and err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"

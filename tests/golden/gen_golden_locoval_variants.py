#!/usr/bin/env python3
"""Golden vectors of the four LocoVal input configurations, from the REFERENCE's own ValuePoseNet on the CPU.

    python tests/golden/gen_golden_locoval_variants.py        # writes tests/golden/locoval_variants.npz

The reference is imported read-only through tests/golden/_ref_shim.py (pacer/pacer/learning/value_pose_net.py); only the inputs and
what it computed are stored.  Keys are `<variant>_<name>` with variant in full / pose / vel / traj; per variant: a seeded Xavier
network's state_dict, the inputs (trajectory of stride 3, one sample with waypoint-1 x = 0 for the epsilon guard; pose; velocity), the
caller's pose after the call (rotated in place in EVERY variant, hidden joints zeroed only where the pose is an input), the value,
the EmLoco loss with its gradients, and the sum-reduction fit of the rollout (amp_continuous_value.py:123-145) with its gradients.
The file is written with fixed zip timestamps: regenerating it gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim  # noqa: E402

VARIANTS = {"full": (True, True), "pose": (True, False), "vel": (False, True), "traj": (False, False)}
B = 9            # not a multiple of four: the narrow kernels' last wave is partly empty


def write_npz(path, arrays):
    """np.savez with fixed zip timestamps (byte-identical output)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, b.getvalue())


def main():
    _ref_shim.install_pacer()
    from learning.value_pose_net import ValuePoseNet
    torch.set_num_threads(1)
    out = {"torch_version": np.array(torch.__version__), "variants": np.array(list(VARIANTS))}
    for seed, (name, (use_pose, use_vel)) in enumerate(VARIANTS.items()):
        g = torch.Generator().manual_seed(100 + seed)
        torch.manual_seed(50 + seed)
        net = ValuePoseNet(use_pose=use_pose, use_vel=use_vel)
        traj = torch.cumsum(torch.randn(B, 13, 3, generator=g) * 0.3 + torch.tensor([0.5, 0.1, 0.0]), dim=1)
        traj[:, 0] = 0
        traj[0, 1, 0] = 0.0              # exercises the epsilon guard on x
        pose = torch.randn(B, 24, 3, generator=g) * 0.3
        vel = torch.randn(B, 2, generator=g)
        target = torch.rand(B, 1, generator=g)
        vel_arg = (lambda: vel.clone()) if use_vel else (lambda: None)
        traj_req = traj.clone().requires_grad_(True)
        pose_in = pose.clone()           # handed to every variant: _rotate_normalization rotates it whether it is an input or not
        value, loss = net.calc_embodied_motion_loss(traj_req, pose_in, vel_arg())
        loss.backward()
        a = {"traj": traj, "pose": pose, "vel": vel, "pose_after_inplace": pose_in, "value": value, "loss": loss,
             "grad_traj": traj_req.grad, "target": target}
        a["state_keys"] = np.array(list(net.state_dict().keys()))
        a.update({k.replace(".", "_"): p for k, p in net.state_dict().items()})
        a.update({"grad_"+ k.replace(".", "_"): p.grad.clone() for k, p in net.named_parameters()})
        net.zero_grad()
        v2 = net(traj.clone(), pose.clone(), vel_arg())
        fit_loss = torch.nn.MSELoss(reduction="sum")(v2, target)
        fit_loss.backward()
        a.update({"fit_value": v2, "fit_loss": fit_loss})
        a.update({"fitgrad_" + k.replace(".", "_"): p.grad.clone() for k, p in net.named_parameters()})
        a["dims"] = np.array([net._network.fc1.in_features, net._network.fc1.out_features, net._network.fc2.out_features,
                              sum(p.numel() for p in net.parameters())], np.int64)
        for k, v in a.items():
            out[name + "_" + k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(HERE, "locoval_variants.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

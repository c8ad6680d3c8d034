"""ValuePoseNet: the Locomotion Value function ("LocoVal").

Mirror of pacer/pacer/learning/value_pose_net.py (class ValuePoseNet :10-159): same constructor flags, same
parameter names (`_network.fc{1,2,3}.{weight,bias}`, so reference checkpoints load), same
`forward / calc_embodied_motion_loss` signatures.  The arithmetic -- yaw normalisation, hidden-joint zeroing,
the MLP, and the whole backward -- is one fused HIP kernel pair per input configuration (:22-50, `use_pose` / `use_vel`):
100->49->24->1 (pose + velocity, emloco_locoval_fwd/bwd), 98->48->24->1 (pose), 28->13->6->1 (velocity), 26->12->6->1 (trajectory
only) through emloco_locoval_variant_fwd/bwd.  `init_pose` / `init_vel` may be None where the variant does not read them.

Bug-compatibility: the reference rotates / zeroes the CALLER's init_pose tensor in place (:97,:141-144), so in the
multi-modal training loop the pose is rotated cumulatively once per mode (train_jta.py:294-296).  `inplace_pose=True`
(default) reproduces that side effect; pass False for the side-effect-free behaviour.
"""
import torch
import torch.nn as nn

from ..predictor.ops import LocoValFn, LocoValVariantFn, locoval_dims, locoval_variant


class ValuePoseNet(nn.Module):
    def __init__(self, use_pose, use_vel, hide_toe=True, hide_spine=True, normalize=True, vru=False, inplace_pose=True, **kwargs):
        super().__init__(**kwargs)
        if not (hide_toe and hide_spine and normalize and not vru):
            raise NotImplementedError("the fused LocoVal kernels implement the networks the reference's entry points build "
                                      "(hide_toe, hide_spine, normalize, 13 waypoints)")
        self.use_pose, self.use_vel, self.hide_toe, self.hide_spine, self.normalize, self.use_vru = bool(use_pose), bool(use_vel), True, True, True, False
        self.inplace_pose = inplace_pose
        self.traj_size, self.pose_size, self.vel_size = 13 * 2, 24 * 3, 2
        self.variant = locoval_variant(self.use_pose, self.use_vel)             # EMLOCO_LOCOVAL_*
        n_in, h1, h2, self.n_param = locoval_dims(self.variant)                  # :43-52
        self._network = nn.Sequential()
        self._network.add_module('fc1', nn.Linear(n_in, h1))
        self._network.add_module('relu1', nn.ReLU())
        self._network.add_module('fc2', nn.Linear(h1, h2))
        self._network.add_module('relu2', nn.ReLU())
        self._network.add_module('fc3', nn.Linear(h2, 1))
        self._network.add_module('sigmoid', nn.Sigmoid())
        for m in self._network:
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)
        self.criterion = nn.MSELoss()

    @property
    def layer_sizes(self):
        """(in, h1, h2) of this variant"""
        return locoval_dims(self.variant)[:3]

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A checkpoint of another input configuration names both shapes instead of torch's per-tensor list."""
        w = state_dict.get("_network.fc1.weight") if hasattr(state_dict, "get") else None
        if w is not None and tuple(w.shape) != tuple(self._network.fc1.weight.shape):
            names = {100: "pose + velocity", 98: "pose", 28: "velocity", 26: "trajectory only"}
            got, want = tuple(w.shape), tuple(self._network.fc1.weight.shape)
            raise RuntimeError(f"LocoVal checkpoint is of another input configuration: its fc1 is {got[1]} -> {got[0]} "
                               f"({names.get(got[1], 'unknown')}), this network's is {want[1]} -> {want[0]} ({names[want[1]]}); "
                               "build the network with the use_pose / use_vel the checkpoint was trained with")
        return super().load_state_dict(state_dict, *args, **kwargs)

    def forward(self, waypoint_traj, init_pose=None, init_vel=None):
        n = self._network
        if self.use_pose:
            assert init_pose is not None, "init_pose should be included"
        if self.use_vel:
            assert init_vel is not None, "init_vel should be included"
        params = (n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias)
        write_back = self.inplace_pose and init_pose is not None and not init_pose.requires_grad
        if self.variant == 3:
            pose_in = init_pose.clone() if self.inplace_pose else init_pose     # the kernel keeps the un-rotated pose for its backward
            value, x100 = LocoValFn.apply(waypoint_traj, pose_in, init_vel, *params)
            rotated = x100[:, 26:98]
        else:
            # the reference rotates the caller's pose in every variant (:96-97) and zeroes the hidden joints where it is an input
            pose_in = init_pose.clone() if (self.use_pose and self.inplace_pose) else init_pose
            value, x, pose_rot = LocoValVariantFn.apply(self.variant, waypoint_traj, pose_in, init_vel, *params,
                                                        write_back and not self.use_pose)
            rotated = x[:, 26:98] if self.use_pose else pose_rot
        if write_back:
            with torch.no_grad():
                init_pose.copy_(rotated.view(-1, 24, 3))
        return value

    net_forward = forward

    def calc_embodied_motion_loss(self, pred_traj, init_pose=None, init_vel=None):
        pred_value = self.forward(pred_traj, init_pose, init_vel)
        loss = self.criterion(pred_value, torch.ones_like(pred_value))
        return pred_value, loss

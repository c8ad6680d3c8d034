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

`refine` is the test-time use of the network (plausibl/test_value_mlp.py:239-274): paths nudged along the value's gradient.
"""
import torch
import torch.nn as nn

from ..predictor.ops import LocoValFn, LocoValVariantFn, locoval_dims, locoval_refine, locoval_variant

HIDDEN_JOINTS = (4, 8, 9, 10, 11)      # value_pose_net.py:141-144 (hide_toe, hide_spine)


def locoval_value_torch(variant, traj, pose, vel, params):
    """value_pose_net.py:73-159 in plain torch for traj (B, 13, >= 2): the value (B,) of one variant, nothing rotated in the caller's
    memory.  The statement `refine_torch` differentiates; the device runs the HIP kernels instead."""
    w1, b1, w2, b2, w3, b3 = params
    B = traj.shape[0]
    x1 = traj[:, 1, 0]
    x1 = torch.where(x1.abs() < 1e-10, torch.full_like(x1, 1e-10), x1)                    # (the guarded x carries no gradient)
    ang = torch.atan2(traj[:, 1, 1], x1)
    c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
    rot = lambda x, y: torch.stack([x * c + y * s, -x * s + y * c], -1)                   # bmm(v, [[c, -s], [s, c]])
    feats = [rot(traj[..., 0], traj[..., 1]).reshape(B, 26)]
    if variant & 2:
        keep = torch.ones(24, dtype=pose.dtype, device=pose.device)
        keep[list(HIDDEN_JOINTS)] = 0
        feats.append((torch.cat([rot(pose[..., 0], pose[..., 1]), pose[..., 2:3]], -1) * keep[None, :, None]).reshape(B, 72))
    if variant & 1:
        feats.append(rot(vel[:, :1], vel[:, 1:2]).reshape(B, 2))
    h = torch.relu(torch.cat(feats, -1) @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    return torch.sigmoid(h @ w3.T + b3)[:, 0]


def refine_torch(variant, traj, pose, vel, params, steps, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, anchor_w=0.0, want_grad0=False):
    """The loop of ops.locoval_refine composed from stock torch in the tensors' own precision: autograd through `locoval_value_torch`
    and torch.optim.Adam on the xy of waypoints 1..12 (plausibl/test_value_mlp.py:239-274).  What ValuePoseNet.refine runs on CPU
    tensors; every row is processed.  Returns (traj_out, value_before, value_after[, grad0])."""
    if want_grad0 and steps < 1:
        raise ValueError("refine_torch: grad0 is the gradient of the first step; steps >= 1")
    traj = traj.detach()
    params = [p.detach() for p in params]
    pose, vel = (pose.detach() if pose is not None else None), (vel.detach() if vel is not None else None)
    with torch.enable_grad():
        free = traj[:, 1:, :2].clone().requires_grad_(True)
        p0 = free.detach().clone()
        whole = lambda: torch.cat([traj[:, :1, :2], free], 1)
        opt = torch.optim.Adam([free], lr=lr, betas=tuple(betas), eps=eps)
        before = locoval_value_torch(variant, whole(), pose, vel, params).detach()
        grad0 = None
        for t in range(steps):
            opt.zero_grad()
            value = locoval_value_torch(variant, whole(), pose, vel, params)
            loss = grad_scale * torch.exp(-value).sum() + anchor_w * ((free - p0) ** 2).sum(-1).mean(-1).sum()
            loss.backward()
            if t == 0:
                grad0 = free.grad.detach().clone()
            opt.step()
        after = locoval_value_torch(variant, whole(), pose, vel, params).detach() if steps else before.clone()
    out = traj.clone()
    out[:, 1:, :2] = free.detach()
    return (out, before, after, grad0) if want_grad0 else (out, before, after)


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

    def refine(self, pred_traj, init_pose=None, init_vel=None, steps=750, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, anchor_w=0.0,
               row_mask=None, want_grad0=False):
        """Nudge the paths pred_traj (B, 13, >= 2) towards a higher value of this network: `steps` Adam steps per row on the xy of waypoints
        1..12, objective grad_scale * exp(-V) + anchor_w / 12 * sum |p - p0|^2 (plausibl/test_value_mlp.py:239-274: 750 steps, lr 1e-4; its
        batch mean over N rows is grad_scale = 1 / N -- the default 1 keeps a row independent of the rows it is launched with).  On the
        device this is ONE launch (ops.locoval_refine); on CPU tensors the plain-torch composition `refine_torch`, in fp32.
        The pose is always the side-effect-free one: `inplace_pose`, the reference's cumulative rotation of the caller's pose from call to
        call, has no meaning inside an optimisation loop, and init_pose / init_vel are never written.  Rows with `row_mask` False, and
        rows with a non-finite coordinate, pose or velocity among what the network reads, come back unchanged with value NaN.
        Returns (traj_out, value_before (B,), value_after (B,)[, grad0 (B, 12, 2)]); no gradient flows to the parameters or the input."""
        n = self._network
        if self.use_pose:
            assert init_pose is not None, "init_pose should be included"
        if self.use_vel:
            assert init_vel is not None, "init_vel should be included"
        params = (n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias)
        B = pred_traj.shape[0]
        pose = init_pose.reshape(B, 24, 3) if self.use_pose else None
        vel = init_vel.reshape(B, 2) if self.use_vel else None
        mask = torch.isfinite(pred_traj[..., :2]).reshape(B, -1).all(1)
        for t in (pose, vel):
            if t is not None:
                mask = mask & torch.isfinite(t).reshape(B, -1).all(1).to(mask.device)
        if row_mask is not None:
            mask = mask & row_mask.to(mask.device).reshape(B).bool()
        kw = dict(lr=lr, betas=betas, eps=eps, grad_scale=grad_scale, anchor_w=anchor_w, want_grad0=want_grad0)
        if pred_traj.is_cuda:
            return locoval_refine(self.variant, pred_traj, pose, vel, params, steps, row_mask=mask, **kw)
        rows = torch.nonzero(mask).flatten()
        out = pred_traj.detach().clone()
        values = [torch.full((B,), float("nan"), dtype=out.dtype) for _ in range(2)]
        grad0 = torch.zeros(B, 12, 2, dtype=out.dtype)
        if len(rows):
            sel = lambda t: None if t is None else t[rows].to(out.dtype)
            got = refine_torch(self.variant, out[rows], sel(pose), sel(vel), [p.to(out.dtype) for p in params], steps, **kw)
            out[rows], values[0][rows], values[1][rows] = got[0], got[1], got[2]
            if want_grad0:
                grad0[rows] = got[3]
        return (out, values[0], values[1], grad0) if want_grad0 else (out, values[0], values[1])

    def calc_embodied_motion_loss(self, pred_traj, init_pose=None, init_vel=None):
        pred_value = self.forward(pred_traj, init_pose, init_vel)
        loss = self.criterion(pred_value, torch.ones_like(pred_value))
        return pred_value, loss

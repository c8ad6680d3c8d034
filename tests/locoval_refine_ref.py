"""TEST INFRASTRUCTURE: the float64 reference of the LocoVal refinement loop (emloco_locoval_refine) and the inputs its tests share.

Written from the formulas of include/emloco_predictor.h with torch autograd, independently of the package's own torch restatement
(emloco_amd/learning/value_pose_net.py: refine_torch), which the CPU tests hold against this one:

    V(p)   value_pose_net.py:73-159: yaw of waypoint 1 (x guarded at 1e-10, the guard a constant), rotation of trajectory, pose and
           velocity by it, joints 4, 8, 9, 10, 11 zeroed, ReLU, ReLU, sigmoid
    L      grad_scale * exp(-V(p)) + anchor_w / 12 * sum_k |p_k - p0_k|^2        per row, p = xy of waypoints 1..12
    Adam   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Inputs: B "walker" paths (speed U[0.4, 2.0] m/s, heading U[0, 2 pi), turn rate N(0, 0.3^2) rad per 0.4 s frame, 2 cm jitter per
waypoint, the origin prepended), pose N(0, 0.3^2), velocity N(0, 1); Xavier-uniform weights with N(0, 0.1^2) biases on fc1 and fc2 so
that units sit on both sides of zero.
"""
import math

import torch

HIDDEN = (4, 8, 9, 10, 11)
VARIANTS = {"full": 3, "pose": 2, "vel": 1, "traj": 0}           # (use_pose << 1) | use_vel
SEED = 2


def dims(variant):
    n_in = 26 + (72 if variant & 2 else 0) + (2 if variant & 1 else 0)
    return n_in, n_in // 2 - 1, (n_in // 2 - 1) // 2


def weights(variant, seed=1):
    """(w1, b1, w2, b2, w3, b3) float64"""
    n_in, h1, h2 = dims(variant)
    g = torch.Generator().manual_seed(seed + 10 * variant)

    def xavier(o, i):
        return (torch.rand(o, i, generator=g, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / (i + o))
    return [xavier(h1, n_in), torch.randn(h1, generator=g, dtype=torch.float64) * 0.1, xavier(h2, h1),
            torch.randn(h2, generator=g, dtype=torch.float64) * 0.1, xavier(1, h2), torch.zeros(1, dtype=torch.float64)]


def walkers(B=64, seed=SEED, stride=2):
    """(traj (B, 13, stride), pose (B, 24, 3), vel (B, 2)) float64; the columns beyond xy carry a marker that must come back."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    speed, heading, turn = 0.4 + 1.6 * r(B), r(B) * 2 * math.pi, 0.3 * n(B)
    pts = [torch.zeros(B, 2, dtype=torch.float64)]
    for _ in range(12):
        heading = heading + turn
        pts.append(pts[-1] + 0.4 * speed[:, None] * torch.stack([heading.cos(), heading.sin()], -1) + 0.02 * n(B, 2))
    xy = torch.stack(pts, 1)
    traj = torch.cat([xy, 7.0 + torch.arange(B * 13 * (stride - 2), dtype=torch.float64).reshape(B, 13, stride - 2)], -1)
    return traj, 0.3 * n(B, 24, 3), n(B, 2)


def special_rows(traj):
    """A copy with row 5's waypoint 1 under the 1e-10 guard (x = 0) and row 9's on the negative x axis (the atan2 branch cut)."""
    t = traj.clone()
    t[5, 1, 0] = 0.0
    t[5, 1, 1] = 0.5
    t[9, 1, 0], t[9, 1, 1] = -0.5, 0.0
    return t


def value(variant, traj, pose, vel, params):
    w1, b1, w2, b2, w3, b3 = params
    B = traj.shape[0]
    x, y = traj[..., 0], traj[..., 1]
    x1 = torch.where(x[:, 1].abs() < 1e-10, torch.full_like(x[:, 1], 1e-10), x[:, 1])
    th = torch.atan2(y[:, 1], x1)
    c, s = th.cos()[:, None], th.sin()[:, None]
    feats = [torch.stack([x * c + y * s, -x * s + y * c], -1).reshape(B, 26)]
    if variant & 2:
        px, py, pz = pose[..., 0], pose[..., 1], pose[..., 2]
        keep = torch.ones(24, dtype=traj.dtype)
        keep[list(HIDDEN)] = 0
        feats.append((torch.stack([px * c + py * s, -px * s + py * c, pz], -1) * keep[None, :, None]).reshape(B, 72))
    if variant & 1:
        feats.append(torch.stack([vel[:, 0] * c[:, 0] + vel[:, 1] * s[:, 0], -vel[:, 0] * s[:, 0] + vel[:, 1] * c[:, 0]], -1))
    h = torch.relu(torch.cat(feats, -1) @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    return torch.sigmoid(h @ w3.T + b3)[:, 0]


def refine(variant, traj, pose, vel, params, steps, lr, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, anchor_w=0.0, row_mask=None):
    """float64: {traj_out, value_before, value_after, grad0 (the gradient at t = 1; None with steps = 0)}; rows with row_mask False
    come back unchanged (their values are still computed here)."""
    f64 = lambda t: None if t is None else t.detach().double()
    traj, pose, vel, params = f64(traj), f64(pose), f64(vel), [f64(p) for p in params]
    B = traj.shape[0]
    on = torch.ones(B, dtype=torch.bool) if row_mask is None else row_mask.bool()
    p0 = traj[:, 1:, :2].clone()
    p = p0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    whole = lambda q: torch.cat([traj[:, :1, :2], q], 1)
    before = value(variant, traj[..., :2], pose, vel, params)
    grad0 = None
    for t in range(1, steps + 1):
        q = p.clone().requires_grad_(True)
        loss = (grad_scale * torch.exp(-value(variant, whole(q), pose, vel, params)) + anchor_w / 12.0 * ((q - p0) ** 2).sum((1, 2))).sum()
        g, = torch.autograd.grad(loss, q)
        if t == 1:
            grad0 = g.clone()
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        step = lr / (1 - betas[0] ** t) * m / (v.sqrt() / math.sqrt(1 - betas[1] ** t) + eps)
        p = torch.where(on[:, None, None], p - step, p)
    out = traj.clone()
    out[:, 1:, :2] = p
    return {"traj_out": out, "value_before": before, "value_after": value(variant, out[..., :2], pose, vel, params), "grad0": grad0}

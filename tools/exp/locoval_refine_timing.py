"""Time the refinement of predicted paths against LocoVal: the fused launch (emloco_locoval_refine) against the composition a caller
had before it -- per step the variant's forward and backward kernels through autograd (ops.LocoValVariantFn, which also fills the
B x n_param parameter-gradient workspace and reduces it) and torch.optim.Adam on the device.

    python tools/exp/locoval_refine_timing.py [--rows 10240] [--steps 750] [--variant 3] [--out profiles/locoval_refine_timing.txt]

B = 10 240 is 512 samples x 20 modes, 750 steps the reference's loop (plausibl/test_value_mlp.py:258).  Median of 5 runs after 2
warm-ups, wall clock around a device synchronisation (the composition is thousands of launches: its time IS host time).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10240)
    ap.add_argument("--steps", type=int, default=750)
    ap.add_argument("--variant", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args(argv)
    from emloco_amd import configure_runtime
    configure_runtime()
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.predictor.ops import LocoValVariantFn
    dev, v, B = torch.device("cuda:0"), a.variant, a.rows
    torch.manual_seed(1)
    net = ValuePoseNet(use_pose=bool(v & 2), use_vel=bool(v & 1), inplace_pose=False).to(dev).eval()
    n = net._network
    with torch.no_grad():
        n.fc1.bias.normal_(0, 0.1); n.fc2.bias.normal_(0, 0.1)
    params = [p.detach() for p in (n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias)]
    g = torch.Generator().manual_seed(2)
    step = 0.4 * (0.4 + 1.6 * torch.rand(B, 1, 1, generator=g)) * torch.nn.functional.normalize(torch.randn(B, 1, 2, generator=g), dim=-1)
    traj = torch.cat([torch.zeros(B, 1, 2), torch.cumsum(step + 0.02 * torch.randn(B, 12, 2, generator=g), 1)], 1).to(dev)
    pose, vel = (0.3 * torch.randn(B, 24, 3, generator=g)).to(dev), torch.randn(B, 2, generator=g).to(dev)

    def fused():
        return net.refine(traj, pose, vel, steps=a.steps, lr=a.lr)[0]

    def composed():
        free = traj[:, 1:].clone().requires_grad_(True)
        opt = torch.optim.Adam([free], lr=a.lr)
        for _ in range(a.steps):
            opt.zero_grad()
            value = LocoValVariantFn.apply(v, torch.cat([traj[:, :1], free], 1), pose if v & 2 else None, vel if v & 1 else None, *params)[0]
            torch.exp(-value).sum().backward()
            opt.step()
        return torch.cat([traj[:, :1], free.detach()], 1)

    def clock(fn):
        times = []
        for r in range(a.warmup + a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times)), min(times), max(times), out
    tf, tf_lo, tf_hi, out_f = clock(fused)
    tc, tc_lo, tc_hi, out_c = clock(composed)
    diff = float((out_f - out_c).abs().max())
    moved = float((out_c - traj).abs().max())
    dims = net.layer_sizes
    flop = 2.0 * B * a.steps * 2 * (dims[0] * dims[1] + dims[1] * dims[2] + dims[2])          # forward + input-gradient products, unfactored
    text = (f"LocoVal refinement, variant {v} ({dims[0]} / {dims[1]} / {dims[2]}), B = {B} rows, {a.steps} Adam steps, lr {a.lr:g}; "
            f"median of {a.runs} runs after {a.warmup} warm-ups, wall clock around a device synchronisation (min .. max)\n"
            f"fused launch (emloco_locoval_refine)            {tf:10.2f} ms   ({tf_lo:.2f} .. {tf_hi:.2f})\n"
            f"composition (LocoValVariantFn + torch Adam)     {tc:10.2f} ms   ({tc_lo:.2f} .. {tc_hi:.2f})\n"
            f"composition / fused                             {tc / tf:10.1f} x\n"
            f"largest |fused - composed| coordinate {diff:.2e} m of up to {moved:.3f} m moved; "
            f"{flop / 1e9:.0f} GFLOP of fp32 products in the unfactored loop\n")
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return tf, tc


if __name__ == "__main__":
    main()

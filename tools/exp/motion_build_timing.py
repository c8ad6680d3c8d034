"""Time one `MotionLib.load_motions` of a training-sized draw, host build against device build.

    python tools/exp/motion_build_timing.py [--envs 4096] [--clips 512] [--shapes 64] [--runs 3] [--no_host] [--host_envs N] [--out profiles/motion_build_timing.txt]

A synthetic pickle in the reference's format: `--clips` smooth random-walk clips of 150-300 frames at 30 fps; `--shapes` skeletons (the
shipped humanoid's joint offsets scaled 0.8 .. 1.25), env j on shape j mod shapes, so that almost every (clip, skeleton) pair of a
draw is distinct, as in a run with shape variation.  The device build is timed `--runs` times after one warm-up (which also
allocates the frame arrays): the whole call by the wall clock around a device synchronisation, upload and kernel from the HIP
events `load_motions` records.  The host build (`clip_cache` per pair, float64) is timed once, on the first `--host_envs` envs of the
same draw when that is given (its time is linear in the number of distinct pairs: the per-pair time is printed).  The largest
difference of each cache array between the two builds is printed with the times.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def synthetic_pickle(n_clips, parent, seed=0):
    from emloco_amd.gym import torch_utils as tu
    g = torch.Generator().manual_seed(seed)
    clips = {}
    for i in range(n_clips):
        T = int(torch.randint(150, 301, (1,), generator=g))
        rv = torch.cumsum(torch.cat([0.3 * torch.randn(1, 24, 3, generator=g), 0.02 * torch.randn(T - 1, 24, 3, generator=g)]), 0)
        lq = tu.exp_map_to_quat(rv.reshape(-1, 3)).view(T, 24, 4)
        gq = torch.zeros_like(lq)
        for b in range(24):
            gq[:, b] = lq[:, b] if parent[b] < 0 else tu.normalize(tu.quat_mul(gq[:, parent[b]], lq[:, b]))
        trans = torch.cumsum(0.02 * torch.randn(T, 3, generator=g), 0) + torch.tensor([0.0, 0.0, 0.9])
        clips[f"clip{i:04d}"] = {"pose_quat_global": gq.numpy(), "root_trans_offset": trans.numpy(), "pose_aa": np.zeros((T, 72), np.float32),
                                 "beta": np.zeros(16, np.float32), "gender": "neutral", "fps": 30}
    return clips


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--host_envs", type=int, default=0, help="time the host build on the first N envs of the draw only (0: all of them)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args(argv)
    from emloco_amd import configure_runtime
    configure_runtime()
    from emloco_amd import _lib
    from emloco_amd.model import smpl_humanoid
    from emloco_amd.utils.motion_lib_smpl import FRAME_KEYS, MotionLib
    _lib.require_device()
    m = smpl_humanoid()
    lt, parent = np.asarray(m.joint_off, np.float64), np.asarray(m.parent)
    shapes = [(lt * s, parent) for s in np.linspace(0.8, 1.25, a.shapes)]
    skels = [shapes[j % a.shapes] for j in range(a.envs)]
    betas = torch.zeros(a.envs, 17)
    clips = synthetic_pickle(a.clips, parent)
    dev = "cuda:0"
    lib = MotionLib(clips, key_body_ids=[7, 3, 22, 17], device=dev, build="device")
    torch.manual_seed(0)
    lib.load_motions(skels, gender_betas=betas)                      # warm-up: allocation of the frame arrays, code load
    torch.cuda.synchronize()
    wall, up, kern = [], [], []
    for r in range(a.runs):
        torch.manual_seed(1 + r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lib.load_motions(skels, gender_betas=betas)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        u, k = lib.build_times()
        up.append(u)
        kern.append(k)
    frames = int(lib.gts.shape[0])
    pairs = len({(i, j % a.shapes) for j, i in enumerate(lib._curr_motion_ids.tolist())})
    med = lambda x: float(np.median(x))
    text = (f"MotionLib.load_motions, {a.envs} envs, {a.clips} clips of 150-300 frames, {a.shapes} shapes: {frames} frames, {pairs} distinct "
            f"(clip, skeleton) pairs in the last draw; {torch.get_num_threads()} host threads\n"
            f"build=device, median of {a.runs} after 1 warm-up (min .. max), reallocations {lib.num_reallocations}:\n"
            f"  whole call, wall clock        {med(wall):10.2f} ms   ({min(wall):.2f} .. {max(wall):.2f})\n"
            f"  concatenate + upload (events) {med(up):10.2f} ms   ({min(up):.2f} .. {max(up):.2f})\n"
            f"  emloco_motion_build (events)  {med(kern):10.3f} ms   ({min(kern):.3f} .. {max(kern):.3f})\n")
    if not a.no_host:
        n = a.host_envs if 0 < a.host_envs < a.envs else a.envs
        ids = lib._curr_motion_ids[:n]
        # the host library on the SAME clips: its clip j is the device draw's clip of env j, taken in order (every env is a pair of its own)
        host_clips = {f"env{j:05d}": clips[f"clip{int(i):04d}"] for j, i in enumerate(ids.tolist())}
        host = MotionLib(host_clips, key_body_ids=[7, 3, 22, 17], device=dev, build="host")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.load_motions(skels[:n], gender_betas=betas[:n], random_sample=False)
        torch.cuda.synchronize()
        th = time.perf_counter() - t0
        rows = int(host.gts.shape[0])
        n_pairs = n
        diffs = ", ".join(f"{k} {float((getattr(host, k) - getattr(lib, k)[:rows]).abs().max()):.1e}" for k in FRAME_KEYS)
        text += (f"build=host on the first {n} envs of that draw ({n_pairs} pairs built), one call, wall clock {th * 1e3:.0f} ms "
                 f"= {th * 1e3 / n_pairs:.2f} ms per pair; at that rate the {pairs} pairs of the whole draw take {th * pairs / n_pairs:.1f} s "
                 f"= {th * 1e3 * pairs / n_pairs / med(wall):.0f} x the device build\n"
                 f"largest |host - device| per array over those envs: {diffs}\n")
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

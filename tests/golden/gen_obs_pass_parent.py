"""Records tests/golden/obs_pass_parent.npz: the inputs of the launches of tests/obs_pass_cases.py and every byte the build BEFORE the
"evaluate once" change of the observation / reset kernels wrote for them.

Run it on that build -- in a checkout of the commit before the change with this file and tests/obs_pass_cases.py copied in, or with that
commit's library in EMLOCO_LIB for the device stage:

    python tests/golden/gen_obs_pass_parent.py --stage emu --work DIR        (any machine: that commit's emulator build)
    python tests/golden/gen_obs_pass_parent.py --stage device --work DIR     (MI355X: that commit's library)
    python tests/golden/gen_obs_pass_parent.py --stage merge --work DIR      (asserts emulator == device byte for byte, writes the file)

or --stage all where both run in one place.  One file serves the emulator test and the device test because the two stages agree.
The inputs are asserted to hold the cases the tests are about (heading signs and quadrants, a mirrored pair, the joint-angle branches, the
slerp branches and blend weights of the history rows) before anything is recorded."""
import argparse
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kernel_refs as R            # noqa: E402
import obs_pass_cases as OC        # noqa: E402


def frame_blend32(inp, mid, time):
    """fp32 restatement of reset_kernels.hip: frame_blend"""
    f = np.float32
    ln, dt, nf = f(inp["motion_len"][mid]), f(inp["motion_dt"][mid]), int(inp["motion_nframes"][mid])
    time = f(time)
    phase = min(max(time / ln, f(0)), f(1))
    time = max(time, f(0))
    i0 = int(f(phase * f(nf - 1)))
    i1 = min(i0 + 1, nf - 1)
    blend = (time - f(i0) * dt) / dt
    s = int(inp["motion_start"][mid])
    return i0 + s, i1 + s, f(blend)


def check_coverage(inp):
    rb, dof = inp["rb_state"], inp["dof_state"]
    hx, hy = OC.heading_xy(rb[:, 0, 3:7])
    gx, gy = OC.heading_xy(rb[:, R.HEAD_BODY, 3:7])
    quad = lambda x, y: {(bool(a > 0), bool(b > 0)) for a, b in zip(x, y)}
    assert len(quad(hx[:4], hy[:4])) == 4 and len(quad(gx[:4], gy[:4])) == 4, "root and head yaw in all four quadrants"
    want = [(1.0, False), (1.0, True), (-1.0, False), (-1.0, True)]
    for e in range(4):
        assert (hx[4 + e], bool(np.signbit(hy[4 + e]))) == want[e] and hy[4 + e] == 0, ("root facing +-x exactly", e, hx[4 + e], hy[4 + e])
        assert (gx[4 + e], bool(np.signbit(gy[4 + e]))) == want[(e + 2) % 4] and gy[4 + e] == 0, ("head facing +-x exactly", e)
    yaw_r, yaw_h = np.arctan2(hy, hx), np.arctan2(gy, gx)
    assert (np.abs(yaw_r - yaw_h) > 0.05).all() and (np.abs(yaw_r + yaw_h) > 0.05).sum() >= 12, "root and head yaw differ"
    assert OC.same_bits(rb[9], OC.mirror_env(rb[8])) and not OC.same_bits(rb[9], rb[8])
    for e in range(OC.E):
        if e not in (8, 9):
            assert np.abs(rb[e] - OC.mirror_env(rb[e])).max() > 0.1, "a pose that is not left / right symmetric"
    ang = np.linalg.norm(dof[:, :, 0].reshape(OC.E, 23, 3).astype(np.float64), axis=-1)
    sub = sorted({d // 3 for d in R.DOF_SUBSET})
    assert all(j in sub for j in (0, 1, 2, 4))
    assert ang[10, 0] == 0 and 0 < ang[10, 1] <= 1e-5 and abs(ang[10, 2] - np.pi) < 1e-6 and 0 < np.pi - ang[10, 4] < 2e-4
    assert ((ang > 1e-2) & (ang < 3.0)).sum() > OC.E * 23 - 8
    # the history rows of the finished envs: blend weights and slerp branches, from the fp32 frame blend
    kinds = {"blend0": 0, "inside": 0, "flip_root": 0, "flip_joint": 0, "par_root": 0, "par_joint": 0, "equal": 0}
    for bi in range(6):
        u = inp["rnd"][bi]
        mid = min(int(np.float32(u[OC.RND_MOTION]) * np.float32(OC.CLIP_FRAMES.__len__())), 1)
        mt = np.float32(u[OC.RND_TIME]) * np.float32(inp["motion_len"][mid])
        for k in range(1, 15):
            f0, f1, w = frame_blend32(inp, mid, mt - np.float32(OC.DT) * np.float32(k))
            kinds["blend0"] += w == 0
            kinds["inside"] += 0 < w < 1
            for name, q, bodies in (("root", inp["grs"], [0]), ("joint", inp["lrs"], range(1, 24))):
                for b in bodies:
                    c = float(np.dot(q[f0, b].astype(np.float64), q[f1, b].astype(np.float64)))
                    if f0 != f1:
                        kinds["flip_" + name] += c < -0.01
                        kinds["par_" + name] += 0 < np.sqrt(max(1 - c * c, 0)) < 0.0009 and abs(c) < 1
                        kinds["equal"] += abs(c) >= 1
    print("history-row coverage:", {k: int(v) for k, v in kinds.items()})
    assert all(v > 0 for v in kinds.values()), kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", choices=("emu", "device", "merge", "all"), default="all")
    ap.add_argument("--work", default=os.path.join(HERE, "_obs_pass_work"))
    ap.add_argument("--out", default=os.path.join(HERE, "obs_pass_parent.npz"))
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    inp = OC.make_inputs()
    check_coverage(inp)
    path = lambda s: os.path.join(a.work, s + ".pkl")
    if a.stage in ("emu", "all"):
        with open(path("emu"), "wb") as f:
            pickle.dump(OC.run_all(OC.EmuExecutor(), inp), f)
    if a.stage in ("device", "all"):
        exe = OC.DeviceExecutor()
        outs = OC.run_all(exe, inp)
        exe.close()
        with open(path("device"), "wb") as f:
            pickle.dump(outs, f)
    if a.stage in ("merge", "all"):
        with open(path("emu"), "rb") as f:
            emu = pickle.load(f)
        with open(path("device"), "rb") as f:
            dev = pickle.load(f)
        assert set(emu) == set(dev)
        for case in emu:
            for name in emu[case]:
                assert OC.same_bits(emu[case][name], dev[case][name]), ("the emulator build and the device build disagree", case, name)
        init = OC.initial_of(inp)
        for case, (n, ids, ring) in OC.CHAIN_CASES.items():                       # the launches did what the cases are about
            o, i0 = dev[case], init(case)
            live = np.setdiff1d(np.arange(n), ids)
            assert np.isfinite(o["obs"]).all() and np.isfinite(o["flip_obs"]).all() and np.isfinite(o["amp"]).all()
            assert (o["motion_ids"][list(ids)] >= 0).all() and (o["motion_ids"][live] == -9).all()
            assert not OC.same_bits(o["amp"][live], i0["amp"][live])
        np.savez_compressed(a.out, **OC.pack(inp, dev, init))
        print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()

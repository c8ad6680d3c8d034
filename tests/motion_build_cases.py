"""Shared inputs, references and the bar of the motion-build tests (tests/test_motion_build_cpu.py on the emulator,
tests/test_gpu_motion_build.py on the device) -- TEST INFRASTRUCTURE ONLY.

The reference is the float64 host build (`clip_cache`); the yardstick for the error is `restatement`, the same arithmetic in float32
torch with the angle taken as 2 atan2(|xyz|, w).  Both are computed once per case and cached."""
import functools
import os

import numpy as np
import torch

from emloco_amd.utils import motion_lib_smpl as M

KEYS = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")
PARENT = np.asarray([-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 11, 14, 15, 16, 17, 11, 19, 20, 21, 22], np.int32)
EDGE_T = (2, 3, 8, 9, 16, 17, 18, 33, 64, 65, 300, 1100)
FIXTURE_TOL = dict(gts=1e-5, grs=1e-7, lrs=1e-6, gvs=1e-4, gavs=5e-3, dvs=5e-3)         # tests/test_motion_lib_cpu.py:27


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_amass.npz"))


def fixture_clips(g=None):
    g = golden() if g is None else g
    return [{"pose_quat_global": g[f"c{i}_pose_quat_global"], "root_trans_offset": g[f"c{i}_root_trans_offset"],
             "pose_aa": g[f"c{i}_pose_aa"], "beta": g[f"c{i}_beta"], "gender": "neutral", "fps": int(g[f"c{i}_fps"])} for i in range(2)]


def _qmul_np(a, b):
    return M._qmul(torch.from_numpy(a), torch.from_numpy(b)).numpy()


def random_clip(T, fps, seed, step=0.02, still=None, far=0.0):
    """A smooth random walk: every joint's rotation vector drifts by N(0, step) per frame, global rotations by composing down the
    tree; `still` = (first, last): those frames repeat frame `first`; `far`: metres added to the root's x."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    rv = np.cumsum(np.concatenate([rng.normal(0, 0.3, (1, 24, 3)), rng.normal(0, step, (T - 1, 24, 3))]), 0)
    lq = R.from_rotvec(rv.reshape(-1, 3)).as_quat().reshape(T, 24, 4)
    gq = np.zeros_like(lq)
    for b in range(24):
        gq[:, b] = lq[:, b] if PARENT[b] < 0 else _qmul_np(gq[:, PARENT[b]], lq[:, b])
    gq /= np.linalg.norm(gq, axis=-1, keepdims=True)
    trans = np.cumsum(rng.normal(0, 0.02, (T, 3)), 0) + np.asarray([far, 0.0, 0.9])
    if still is not None:
        gq[still[0]:still[1] + 1] = gq[still[0]]
        trans[still[0]:still[1] + 1] = trans[still[0]]
    return {"pose_quat_global": gq.astype(np.float32), "root_trans_offset": trans.astype(np.float32),
            "pose_aa": np.zeros((T, 72), np.float32), "beta": np.zeros(16, np.float32), "gender": "neutral", "fps": fps}


def pack(clips, skeletons, skel_ids):
    """The arguments of emloco_motion_build as host arrays: frames of `clips` concatenated, `skeletons` a list of (24, 3) joint offsets."""
    nfr = np.asarray([len(c["pose_quat_global"]) for c in clips], np.int32)
    start = np.concatenate([[0], np.cumsum(nfr[:-1])]).astype(np.int64)
    return dict(n_clips=len(clips), n_skel=len(skeletons), F=int(nfr.sum()),
                quat_global=np.ascontiguousarray(np.concatenate([np.asarray(c["pose_quat_global"], np.float32) for c in clips])),
                root_trans=np.ascontiguousarray(np.concatenate([np.asarray(c["root_trans_offset"], np.float32) for c in clips])),
                frame_start=start, n_frames=nfr, fps=np.asarray([c["fps"] for c in clips], np.float32),
                skel_id=np.asarray(skel_ids, np.int32), local_translation=np.ascontiguousarray(np.stack(skeletons), dtype=np.float32),
                parent=PARENT.copy(), taps=M.gaussian_taps(), clips=clips, skeletons64=np.stack(skeletons).astype(np.float64))


@functools.lru_cache(maxsize=None)
def fixture_case():
    g = golden()
    assert list(g["parent_indices"]) == list(PARENT)
    return pack(fixture_clips(g), [g["local_translation"]], [0, 0])


@functools.lru_cache(maxsize=None)
def edge_case():
    """One launch: EDGE_T frames, three skeletons (joint offsets scaled 0.8 / 1.0 / 1.25), 30 and 60 fps mixed; the 33-frame clip holds a
    run of identical frames, the 65-frame clip's root is 40 m from the origin."""
    lt = golden()["local_translation"].astype(np.float64)
    clips = [random_clip(T, (30, 60)[i % 2], 100 + i, still=(10, 15) if T == 33 else None, far=40.0 if T == 65 else 0.0)
             for i, T in enumerate(EDGE_T)]
    return pack(clips, [lt * 0.8, lt, lt * 1.25], [i % 3 for i in range(len(clips))])


def empty_outputs(case, fill=np.nan):
    F = case["F"]
    return dict(gts=np.full((F, 24, 3), fill, np.float32), grs=np.full((F, 24, 4), fill, np.float32), lrs=np.full((F, 24, 4), fill, np.float32),
                gvs=np.full((F, 24, 3), fill, np.float32), gavs=np.full((F, 24, 3), fill, np.float32), dvs=np.full((F, 69), fill, np.float32))


def _shape(c):
    return {k: (c[k].reshape(c[k].shape[0], 69) if k == "dvs" else c[k]) for k in KEYS}


def reference(case):
    """the float64 host build, clip by clip, concatenated (cached on the case)"""
    if "_ref" not in case:
        parts = [_shape(M.clip_cache(c, case["skeletons64"][s], case["parent"]))
                 for c, s in zip(case["clips"], case["skel_id"])]
        case["_ref"] = {k: torch.cat([p[k] for p in parts]).numpy() for k in KEYS}
    return case["_ref"]


def _angle_axis32(q):
    s = q[..., :3].norm(dim=-1)
    return 2 * torch.atan2(s, q[..., 3]), q[..., :3] / s.unsqueeze(-1).clamp(min=1e-9)


def _filter32(x, taps):
    T = x.shape[0]
    out = torch.zeros_like(x)
    for k in range(17):
        out = out + taps[k] * x[(torch.arange(T) + k - 8).clamp(0, T - 1)]
    return out


def _clip_cache32(clip, lt, parents, taps):
    """`clip_cache` in float32 torch with the atan2 angle: the yardstick, not the product"""
    f32 = torch.float32
    gq = torch.as_tensor(np.asarray(clip["pose_quat_global"]), dtype=f32)
    trans = torch.as_tensor(np.asarray(clip["root_trans_offset"]), dtype=f32)
    dt = torch.tensor(1.0, dtype=f32) / torch.tensor(float(clip["fps"]), dtype=f32)
    T, J, _ = gq.shape
    lt = torch.as_tensor(lt, dtype=f32)
    lq, gp = torch.zeros_like(gq), torch.zeros(T, J, 3, dtype=f32)
    for b in range(J):
        p = int(parents[b])
        if p < 0:
            lq[:, b], gp[:, b] = gq[:, b], trans
        else:
            lq[:, b] = M._qmul_norm(M._qinv(gq[:, p]), gq[:, b])
            gp[:, b] = gp[:, p] + M._qrot(gq[:, p], lt[b].expand(T, 3))
    grad = torch.zeros_like(gp)
    grad[1:-1] = (gp[2:] - gp[:-2]) / 2
    grad[0], grad[-1] = gp[1] - gp[0], gp[-1] - gp[-2]
    gv = _filter32(grad, taps) / dt
    dq = torch.zeros_like(gq)
    dq[..., 3] = 1.0
    dq[:-1] = M._qmul_norm(gq[1:], M._qinv(gq[:-1]))
    ang, ax = _angle_axis32(dq)
    gav = _filter32(ax * ang.unsqueeze(-1) / dt, taps)
    a2, x2 = _angle_axis32(M._qmul_norm(M._qinv(lq[:-1]), lq[1:]))
    dv = (x2 * a2.unsqueeze(-1) / dt)[:, 1:]
    dv = torch.cat([dv, dv[-1:]], 0)
    return dict(gts=gp, grs=gq, lrs=lq, gvs=gv, gavs=gav, dvs=dv)


def restatement(case):
    if "_rest" not in case:
        taps = torch.from_numpy(case["taps"])
        parts = [_shape(_clip_cache32(c, case["local_translation"][s], case["parent"], taps)) for c, s in zip(case["clips"], case["skel_id"])]
        case["_rest"] = {k: torch.cat([p[k] for p in parts]).numpy() for k in KEYS}
    return case["_rest"]


def assert_input_condition(case):
    """every frame-to-frame rotation, global and local, below 2 rad: qnormalize's sign choice stays away from its discontinuity"""
    ref = reference(case)
    for c0, n in zip(case["frame_start"], case["n_frames"]):
        for k in ("grs", "lrs"):
            q = torch.from_numpy(ref[k][c0:c0 + n])
            d = M._qmul_norm(q[1:], M._qinv(q[:-1]))
            angle = 2 * torch.atan2(d[..., :3].norm(dim=-1), d[..., 3])
            assert float(angle.max()) < 2.0, (k, int(c0), float(angle.max()))


def assert_bar(case, out, label):
    """grs bit for bit; the other five arrays within 4x the float32 restatement's own error against the float64 build (2 for the
    order of the same roundings -- the 17-tap sum, the FK chain, FMA -- times 2 for the spread of a maximum over ~1e5 entries)."""
    ref, rest = reference(case), restatement(case)
    assert_input_condition(case)
    assert np.array_equal(out["grs"].view(np.uint32), case["quat_global"].view(np.uint32)), f"{label}: grs is not the input bit for bit"
    errs = {}
    for k in ("gts", "lrs", "gvs", "gavs", "dvs"):
        assert np.isfinite(out[k]).all(), f"{label}: {k} has non-finite entries"
        e = float(np.abs(out[k].astype(np.float64) - ref[k].reshape(out[k].shape)).max())
        y = float(np.abs(rest[k].astype(np.float64) - ref[k]).max())
        errs[k] = (e, y)
        print(f"{label}: {k} max abs error {e:.3e}, float32 restatement {y:.3e}, ratio {e / max(y, 1e-300):.2f}")
    for k, (e, y) in errs.items():
        assert e <= 4 * y, f"{label}: {k} error {e:.3e} above 4x the restatement's {y:.3e}"
    return errs


def assert_fixture(out, label):
    """the tolerances tests/test_motion_lib_cpu.py holds the host build to, against the reference's own loader"""
    g, case = golden(), fixture_case()
    pairs = [(i, k, out[k][c0:c0 + n].reshape(g[f"c{i}_{k}"].shape), g[f"c{i}_{k}"])
             for i, (c0, n) in enumerate(zip(case["frame_start"], case["n_frames"])) for k in KEYS]
    for i, k, got, want in pairs:                        # every figure is printed before the first assertion
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{label}: clip {i} {k} max abs error vs the reference loader {err:.3e} (tolerance {FIXTURE_TOL[k]:g})")
    for i, k, got, want in pairs:
        np.testing.assert_allclose(got, want, rtol=0, atol=FIXTURE_TOL[k], err_msg=f"{label}: clip {i} {k}")

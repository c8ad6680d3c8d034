"""CPU: refinement of predicted paths against LocoVal (emloco_locoval_refine, ValuePoseNet.refine, evaluate_jta --refine_steps).

The kernel itself runs on the device only (tests/test_gpu_locoval_refine.py; it is not among the CPU emulation's sources).  Here:
  * the yardstick's precondition: on the shared inputs (tests/locoval_refine_ref.py) the package's fp32 torch restatement of the loop
    (ValuePoseNet.refine on CPU tensors) stays within 1e-4 lr K of the float64 reference at K = 20, lr = 1e-2, for every variant --
    two decades inside the 1e-3 lr K the kernel is held to;
  * the algebra of the objective (grad_scale = 1 / N is the reference's batch mean, the anchor, what is copied through, masks);
  * evaluate_ade_fde with and without --refine_steps, the collector's pickle through the --pred_path loader;
  * the argument errors of every layer, which all answer before anything is launched.
"""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import locoval_refine_ref as R
from test_traj_densify_cpu import _StubPredictor, _pred_flags

K, LR = 20, 1e-2


def net_of(variant, cls=None, dtype=torch.float32):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    net = (cls or ValuePoseNet)(use_pose=bool(variant & 2), use_vel=bool(variant & 1), inplace_pose=False)
    n = net._network
    with torch.no_grad():
        for p, w in zip((n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias), R.weights(variant)):
            p.copy_(w.to(dtype))
    return net


def params_of(net):
    n = net._network
    return [p.detach() for p in (n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias)]


def inputs32(B=64, stride=2):
    return [t.float() for t in R.walkers(B, stride=stride)]


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", list(R.VARIANTS))
def test_fp32_restatement_tracks_the_float64_reference(name):
    v = R.VARIANTS[name]
    net = net_of(v)
    traj, pose, vel = inputs32()
    out, before, after = net.refine(traj, pose, vel, steps=K, lr=LR)
    ref = R.refine(v, traj, pose, vel, params_of(net), K, LR)
    err = (out.double() - ref["traj_out"]).abs()
    moved = (ref["traj_out"] - traj.double()).abs().max()
    print(f"{name}: max |fp32 - float64| = {float(err.max()):.3e} m (bar {1e-4 * LR * K:.1e}), moved up to {float(moved):.3f} m, "
          f"value {float(before.mean()):.4f} -> {float(after.mean()):.4f}")
    assert float(err.max()) <= 1e-4 * LR * K
    assert float(after.mean()) > float(before.mean()) and float(ref["value_after"].mean()) > float(ref["value_before"].mean())
    assert float(moved) > 0.5 * LR * K                      # the loop moves points by O(lr) per step: the bar is far below the motion
    np.testing.assert_allclose(before.numpy(), ref["value_before"].numpy(), atol=1e-6)
    np.testing.assert_allclose(after.numpy(), ref["value_after"].numpy(), atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ algebra
def test_grad_scale_one_over_n_is_the_references_batch_mean():
    """plausibl/test_value_mlp.py:239-274 as written: exp(-V).mean() over the batch, torch.optim.Adam on the flattened trajectories."""
    v, N = 3, 64
    net = net_of(v)
    traj, pose, vel = inputs32(N)
    params64 = [p.double() for p in params_of(net)]
    free = traj[:, 1:, :2].double().flatten().clone().requires_grad_(True)
    opt = torch.optim.Adam([free], lr=LR)
    for _ in range(K):
        opt.zero_grad()
        whole = torch.cat([traj[:, :1, :2].double(), free.reshape(N, 12, 2)], 1)
        torch.exp(-R.value(v, whole, pose.double(), vel.double(), params64)).mean().backward()
        opt.step()
    want = free.detach().reshape(N, 12, 2)
    ref = R.refine(v, traj, pose, vel, params64, K, LR, grad_scale=1.0 / N)
    assert float((ref["traj_out"][:, 1:] - want).abs().max()) <= 1e-9
    out = net.refine(traj, pose, vel, steps=K, lr=LR, grad_scale=1.0 / N)[0]
    assert float((out[:, 1:].double() - want).abs().max()) <= 1e-4 * LR * K
    # with the scale 1 the rows are independent of the batch they are in: the mean couples them only through eps
    alone = net.refine(traj[7:8], pose[7:8], vel[7:8], steps=K, lr=LR)[0]
    among = net.refine(traj, pose, vel, steps=K, lr=LR)[0][7:8]
    assert float((alone - among).abs().max()) <= 1e-6


def test_anchor_holds_the_path_back():
    v = 3
    net = net_of(v)
    traj, pose, vel = inputs32()
    shift = lambda w: float((net.refine(traj, pose, vel, steps=K, lr=LR, anchor_w=w)[0] - traj).abs().mean())
    free, held = shift(0.0), shift(5.0)
    assert 0 < held < free, (held, free)
    ref = R.refine(v, traj, pose, vel, params_of(net), K, LR, anchor_w=5.0)
    out = net.refine(traj, pose, vel, steps=K, lr=LR, anchor_w=5.0)[0]
    assert float((out.double() - ref["traj_out"]).abs().max()) <= 1e-4 * LR * K


@pytest.mark.parametrize("name", list(R.VARIANTS))
def test_origin_extra_columns_masked_and_non_finite_rows_come_back_unchanged(name):
    v = R.VARIANTS[name]
    net = net_of(v)
    traj, pose, vel = inputs32(12, stride=3)
    traj[:, 0, :2] = torch.tensor([0.25, -0.5])              # waypoint 0 is copied through whatever it holds
    traj[3, 6, 1] = float("nan")
    pose[4, 2, 0] = float("inf")
    vel[5, 1] = float("nan")
    mask = torch.ones(12, dtype=torch.bool)
    mask[[0, 11]] = False
    pose_in, vel_in = pose.clone(), vel.clone()
    out, before, after, grad0 = net.refine(traj, pose, vel, steps=5, lr=LR, row_mask=mask, want_grad0=True)
    assert torch.equal(torch.nan_to_num(pose), torch.nan_to_num(pose_in)) and torch.equal(torch.nan_to_num(vel), torch.nan_to_num(vel_in))      # read only
    skipped = [0, 11, 3] + ([4] if v & 2 else []) + ([5] if v & 1 else [])
    for i in range(12):
        same = torch.equal(torch.nan_to_num(out[i], nan=-9.0), torch.nan_to_num(traj[i], nan=-9.0))
        assert same == (i in skipped), i
        assert bool(torch.isnan(before[i])) == bool(torch.isnan(after[i])) == (i in skipped), i
    assert torch.equal(out[:, 0], traj[:, 0]) and torch.equal(out[:, :, 2], traj[:, :, 2])
    assert float(grad0[skipped].abs().max()) == 0 and float(grad0[1].abs().max()) > 0
    on = [i for i in range(12) if i not in skipped]
    ref = R.refine(v, traj[on], pose[on], vel[on], params_of(net), 5, LR)
    assert float((out[on].double() - ref["traj_out"]).abs().max()) <= 1e-4 * LR * 5
    np.testing.assert_allclose(grad0[on].numpy(), ref["grad0"].numpy(), atol=1e-5 * float(ref["grad0"].abs().max()))
    # steps = 0: the paths as they are, equal values
    out0, b0, a0 = net.refine(traj, pose, vel, steps=0)
    assert torch.equal(torch.nan_to_num(out0), torch.nan_to_num(traj)) and torch.equal(torch.nan_to_num(b0), torch.nan_to_num(a0))


# ------------------------------------------------------------------------------------------------------------ the evaluation
def _cpu_value_net(variant=3):
    """ValuePoseNet whose forward is the package's plain-torch statement (the HIP forward needs a device); refine is the product's."""
    from emloco_amd.learning.value_pose_net import ValuePoseNet, locoval_value_torch

    class CpuValueNet(ValuePoseNet):
        def forward(self, traj, pose=None, vel=None):
            return locoval_value_torch(self.variant, traj, pose, vel, params_of(self))[:, None]
    return net_of(variant, CpuValueNet).eval()


def _evaluate(tmp_path, collector=None, valuenet="net", M=4, N=7, **kw):
    from torch.utils.data import DataLoader
    from emloco_amd.predictor import evaluate_jta as EV
    from emloco_amd.predictor.dataset_jta import collate_batch, create_dataset, write_synthetic_split
    if not os.path.isdir(os.path.join(str(tmp_path), "jta_all_visual_cues")):
        write_synthetic_split(str(tmp_path), "test", N, max_people=3, seed=3)
    ds = create_dataset("jta_all_visual_cues", None, split="test", track_size=21, track_cutoff=9, preprocessed=True, root=str(tmp_path))
    config = {"DEVICE": "cpu", "TRAIN": {"input_track_size": 9, "output_track_size": 12}, "MODEL": {"value_threshold": 0.5},
              "DATA": {"train_datasets": ["jta_all_visual_cues"]}}
    loader = DataLoader(ds, batch_size=3, num_workers=0, shuffle=False, collate_fn=collate_batch)
    net = _cpu_value_net() if valuenet == "net" else valuenet
    return EV.evaluate_ade_fde(_StubPredictor(M), net, "test", "traj+all", loader, 3, config, dataset="jta", pred_trajs=collector,
                               random_ids=torch.arange(N) % M, **kw)


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype, k
        else:
            assert type(a[k]) is type(b[k]) and (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])), k


def test_refine_steps_zero_changes_nothing(tmp_path):
    from emloco_amd.predictor import evaluate_jta as EV
    tables = []
    for kw in ({}, dict(refine_steps=0, refine_lr=0.5, refine_anchor=2.0, refine_modes="best")):
        col = EV.PredTrajCollector("all")
        res = _evaluate(tmp_path, col, **kw)
        tables.append((res, open(col.save(str(tmp_path / f"t{len(tables)}.pkl")), "rb").read()))
    _same(tables[0][0], tables[1][0])
    assert tables[0][1] == tables[1][1]                                            # the pickle, byte for byte
    assert "value_mean" in tables[0][0] and "ade_value" in tables[0][0] and not any(k.startswith("refine") for k in tables[0][0])
    a = EV.build_arg_parser().parse_args([])
    assert (a.refine_steps, a.refine_lr, a.refine_anchor, a.refine_modes) == (0, 1e-4, 0.0, "all")


def test_refine_steps_three_scores_the_refined_paths_and_keeps_the_unrefined_figures(tmp_path):
    from emloco_amd.env.util.traj_generator import TrajGenerator, load_pred_traj_data
    from emloco_amd.predictor import evaluate_jta as EV
    plain = _evaluate(tmp_path, reference_inplace_pose=False)
    lr = 2e-3
    col = EV.PredTrajCollector("all")
    res = _evaluate(tmp_path, col, refine_steps=3, refine_lr=lr, reference_inplace_pose=False)
    assert list(res)[:len(plain)] == list(plain)
    assert list(res)[len(plain):] == ["refine_steps", "ade_unrefined", "fde_unrefined", "value_mean_unrefined", "refine_shift_mean", "refine_shift_max"]
    assert res["refine_steps"] == 3 and res["ade_unrefined"] == plain["ade"] and res["fde_unrefined"] == plain["fde"]
    assert res["value_mean_unrefined"] == plain["value_mean"] and res["value_mean"] > plain["value_mean"]
    assert res["ade"] != plain["ade"] and res["ade_random"] != plain["ade_random"]
    assert 0 < res["refine_shift_mean"] <= res["refine_shift_max"] <= 3 * lr * 1.01
    # best: one mode per sample moves, so a smaller share of the paths; an anchor is passed through
    best = _evaluate(tmp_path, refine_steps=3, refine_lr=lr, refine_modes="best", refine_anchor=1.0, reference_inplace_pose=False)
    assert plain["value_mean"] < best["value_mean"] < res["value_mean"] and best["refine_shift_max"] <= 3 * lr * 1.01
    # the pickle: the new fields, and the --pred_path loader and generator take it
    path = col.save(str(tmp_path / "refined.pkl"))
    table = pickle.load(open(path, "rb"))
    assert sorted(table) == list(range(7 * 4))
    for e in table.values():
        assert set(e) == {"coord_dense", "sample", "mode", "ade", "locoval", "locoval_unrefined", "refined"} and e["refined"] is True
        assert e["coord_dense"].shape == (101, 3) and 0 < e["locoval_unrefined"] < e["locoval"] < 1
    assert sorted(load_pred_traj_data(path)) == sorted(table)
    tg = TrajGenerator(7, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, flags=_pred_flags(False), pred_traj_data=path)
    tg.reset(torch.arange(7), torch.zeros(7, 3), torch.zeros(7, 3), draws=dict(tg._draw(7, 101), pred_rids=list(range(7))))
    np.testing.assert_allclose(tg._verts[4].numpy()[:, :2], (table[4]["coord_dense"] - table[4]["coord_dense"][0])[:, :2], atol=2e-5)


# ------------------------------------------------------------------------------------------------------------ errors, the ABI
def test_refine_without_a_value_network_names_the_missing_flag(tmp_path):
    from emloco_amd.predictor import evaluate_jta as EV
    with pytest.raises(ValueError, match="--valueloss"):
        _evaluate(tmp_path, valuenet=None, refine_steps=2)
    args = EV.build_arg_parser().parse_args(["--exp_name", "x", "--refine_steps", "5"])
    with pytest.raises(SystemExit, match="--valueloss"):
        EV.run(args)
    with pytest.raises(ValueError, match="refine_modes"):
        _evaluate(tmp_path, refine_steps=1, refine_modes="some")
    with pytest.raises(ValueError, match="steps >= 1"):
        net_of(0).refine(inputs32(2)[0], steps=0, want_grad0=True)


def test_prototype_is_bound_from_the_header():
    from emloco_amd import _abi
    restype, argtypes = _abi.prototypes()["emloco_locoval_refine"]
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    assert restype is ci and argtypes == [ci, ci, vp, ci] + [vp] * 9 + [ci] + [cf] * 6 + [vp] * 5


def bad_argument_cases(call, good):
    """Every refusal of include/emloco_predictor.h: `call(**overrides)` calls emloco_locoval_refine with `good` except the overrides
    and returns its code.  Shared with the device test; none of these launches anything."""
    nan, inf = float("nan"), float("inf")
    cases = [dict(variant=-1), dict(variant=4), dict(B=0), dict(ts=1), dict(n_steps=-1), dict(n_steps=100001), dict(lr=0.0), dict(lr=-1e-3),
             dict(lr=nan), dict(lr=inf), dict(eps=0.0), dict(eps=nan), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=nan),
             dict(traj_out=good["traj"]), dict(pose=None), dict(vel=None)]
    cases += [{k: None} for k in ("traj", "w1", "b1", "w2", "b2", "w3", "b3", "traj_out", "value_before", "value_after")]
    for c in cases:
        assert call(**c) == -1, c
    assert call(variant=0, pose=None, vel=None, B=0) == -1 and call(variant=1, pose=None, vel=None) == -1 and call(variant=2, pose=None) == -1
    return len(cases)


def test_bad_arguments_are_refused_before_any_launch():
    from emloco_amd import _lib as L
    lib = L.load()
    host = np.zeros(4096, np.float32)                         # never read: every case below is refused on the host
    other = np.zeros(4096, np.float32)
    good = dict(variant=3, B=4, traj=host.ctypes.data, ts=2, pose=host.ctypes.data, vel=host.ctypes.data, w1=host.ctypes.data,
                b1=host.ctypes.data, w2=host.ctypes.data, b2=host.ctypes.data, w3=host.ctypes.data, b3=host.ctypes.data, row_mask=None,
                n_steps=3, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, anchor_w=0.0, traj_out=other.ctypes.data,
                value_before=other.ctypes.data, value_after=other.ctypes.data, grad0=None, stream=None)

    def call(**over):
        return lib.emloco_locoval_refine(*{**good, **over}.values())
    assert bad_argument_cases(call, good) >= 29
    assert call(traj_out=host.ctypes.data + 4 * (4 * 13 * 2 - 1)) == -1          # overlapping by one float is aliasing too

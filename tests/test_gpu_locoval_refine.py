"""GPU: emloco_locoval_refine (emloco_amd/csrc/locoval_refine.h) on the MI355X, variants 0..3 throughout.

  1. steps = 0: traj_out is traj, both values are the bits of emloco_locoval_variant_fwd (B in {1, 5, 67}, stride in {2, 3});
  2. grad0 against the float64 reference (tests/locoval_refine_ref.py), error relative to max |g| over the batch.  The bar is
     measured in the run: the deviation of emloco_locoval_variant_bwd's d traj (dvalue = -exp(-V), the composition a caller had before
     this kernel) from float64 on the same inputs, times 4 (another summation order, the factored first layer).  Row 5 has waypoint 1
     under the 1e-10 guard, row 9 on the negative x axis.  Measured on an MI355X (existing backward kernel -> refinement kernel):
     traj 1.59e-7 -> 1.59e-7, vel 2.51e-7 -> 2.07e-7, pose 3.31e-7 -> 4.16e-7, full 3.98e-7 -> 1.37e-7;
  3. 20 steps at lr 1e-2 against float64: every coordinate within 1e-3 lr K = 2e-4 m, at most 2 of 64 rows exempt (a ReLU unit
     crossing zero under another rounding; the fp32 torch restatement exempts none, tests/test_locoval_refine_cpu.py); value_after is
     the forward kernel's value of traj_out; once more with anchor_w = 0.5 (measured: 1.0e-6 .. 2.8e-6 m, no row over the bar);
  4. rows do not depend on the launch they are in, launches repeat, masked rows are left alone;
  5. bad arguments;
  6. evaluate_ade_fde with --refine_steps 5 in-process equals ValuePoseNet.refine applied by hand to the same predictions.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import locoval_refine_ref as R  # noqa: E402
from test_locoval_refine_cpu import bad_argument_cases, net_of, params_of  # noqa: E402

DEV = "cuda:0"
K, LR = 20, 1e-2
VARIANTS = sorted(R.VARIANTS.values())


def _inputs(B=64, stride=2, special=False):
    traj, pose, vel = R.walkers(max(B, 64), stride=stride)
    if special:
        traj = R.special_rows(traj)
    return [t[:B].float().to(DEV).contiguous() for t in (traj, pose, vel)]


def _forward(net, traj, pose, vel):
    """emloco_locoval_variant_fwd through the package's autograd function: (B,) value"""
    from emloco_amd.predictor.ops import LocoValVariantFn
    with torch.no_grad():
        return LocoValVariantFn.apply(net.variant, traj, pose if net.variant & 2 else None, vel if net.variant & 1 else None, *params_of(net))[0].reshape(-1)


@pytest.fixture(scope="module")
def nets():
    return {v: net_of(v).to(DEV).eval() for v in VARIANTS}


@pytest.fixture(scope="module")
def reference(nets):
    """float64, computed once: {(variant, anchor_w): refine(...)} on the 64 walkers, and grad0 on the walkers with the special rows"""
    out = {}
    for v in VARIANTS:
        p = [w.cpu() for w in params_of(nets[v])]
        traj, pose, vel = [t.cpu() for t in _inputs()]
        for aw in (0.0, 0.5):
            out[v, aw] = R.refine(v, traj, pose, vel, p, K, LR, anchor_w=aw)
        straj = _inputs(special=True)[0].cpu()
        out[v, "grad0"] = R.refine(v, straj, pose, vel, p, 1, LR)["grad0"]
    return out


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("v", VARIANTS)
def test_zero_steps_copy_the_paths_and_give_the_forward_kernels_value(nets, v):
    for B in (1, 5, 67):
        for stride in (2, 3):
            traj, pose, vel = _inputs(B, stride)
            out, before, after = nets[v].refine(traj, pose, vel, steps=0)
            want = _forward(nets[v], traj, pose, vel)
            assert out.data_ptr() != traj.data_ptr() and out.cpu().numpy().tobytes() == traj.cpu().numpy().tobytes(), (B, stride)
            assert before.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() == after.cpu().numpy().tobytes(), (B, stride)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("v", VARIANTS)
def test_first_gradient_within_four_times_the_backward_kernels_error(nets, reference, v):
    """Measured on an MI355X, largest |error| / largest |float64 g| over the batch, existing backward kernel -> this kernel (bar = 4 x
    the first): traj 1.59e-7 -> 1.59e-7, vel 2.51e-7 -> 2.07e-7, pose 3.31e-7 -> 4.16e-7, full 3.98e-7 -> 1.37e-7."""
    from emloco_amd.predictor.ops import LocoValVariantFn
    net = nets[v]
    traj, pose, vel = _inputs(special=True)
    assert float(traj[5, 1, 0].abs()) < 1e-10 and float(traj[9, 1, 0]) < 0 and float(traj[9, 1, 1]) == 0
    g64 = reference[v, "grad0"]
    scale = float(g64.abs().max())
    leaf = traj.clone().requires_grad_(True)
    value = LocoValVariantFn.apply(v, leaf, pose if v & 2 else None, vel if v & 1 else None, *params_of(net))[0]
    torch.exp(-value).sum().backward()
    composed = float((leaf.grad[:, 1:, :2].double().cpu() - g64).abs().max()) / scale
    grad0 = net.refine(traj, pose, vel, steps=1, lr=LR, want_grad0=True)[3]
    fused = float((grad0.double().cpu() - g64).abs().max()) / scale
    print(f"grad0 variant {v}: backward kernel {composed:.3e}, refinement kernel {fused:.3e}, bar {4 * composed:.3e} (of max |g| = {scale:.3e})")
    assert 0 < composed < 1e-5
    assert fused <= 4 * composed


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("aw", [0.0, 0.5])
@pytest.mark.parametrize("v", VARIANTS)
def test_twenty_steps_track_the_float64_reference(nets, reference, v, aw):
    net = nets[v]
    traj, pose, vel = _inputs()
    out, before, after = net.refine(traj, pose, vel, steps=K, lr=LR, anchor_w=aw)
    ref = reference[v, aw]
    err = (out.double().cpu() - ref["traj_out"]).abs().reshape(64, -1).max(1)[0]
    off = int((err > 1e-3 * LR * K).sum())
    print(f"variant {v} anchor {aw}: max |kernel - float64| = {float(err.max()):.3e} m, rows over {1e-3 * LR * K:.0e}: {off} of 64; "
          f"value {float(before.mean()):.4f} -> {float(after.mean()):.4f}")
    assert off <= 2
    assert float(np.sort(err.numpy())[-3]) <= 1e-3 * LR * K                        # every row but the exempt ones
    assert after.cpu().numpy().tobytes() == _forward(net, out, pose, vel).cpu().numpy().tobytes()
    assert before.cpu().numpy().tobytes() == _forward(net, traj, pose, vel).cpu().numpy().tobytes()
    assert float(after.mean()) > float(before.mean())
    assert torch.equal(out[:, 0], traj[:, 0])


# ------------------------------------------------------------------------------------------------------------ 4
def _raw(v, net, traj, pose, vel, mask, value_fill):
    """the C entry point with caller-filled value arrays"""
    from emloco_amd.predictor import ops
    B = traj.shape[0]
    out = torch.full_like(traj, -3.0)
    before, after = torch.full((B,), value_fill, device=DEV), torch.full((B,), value_fill, device=DEV)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ps = [p.contiguous() for p in params_of(net)]
    rc = ops._lib().emloco_locoval_refine(v, B, P(traj), traj.shape[-1], P(pose), P(vel), *[P(p) for p in ps], P(mask), K, LR, 0.9, 0.999, 1e-8, 1.0,
                                          0.0, P(out), P(before), P(after), None, ops._st(traj))
    assert rc == 0
    torch.cuda.synchronize()
    return out, before, after


@pytest.mark.parametrize("v", VARIANTS)
def test_rows_are_independent_launches_repeat_and_masked_rows_are_left_alone(nets, v):
    net = nets[v]
    traj, pose, vel = _inputs(67, stride=3)
    whole = net.refine(traj, pose, vel, steps=K, lr=LR)
    again = net.refine(traj, pose, vel, steps=K, lr=LR)
    for a, b in zip(whole, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for i in (0, 17, 66):
        alone = net.refine(traj[i:i + 1].contiguous(), pose[i:i + 1].contiguous(), vel[i:i + 1].contiguous(), steps=K, lr=LR)
        for a, b in zip(whole, alone):
            assert a[i:i + 1].cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), i
    mask = torch.ones(67, dtype=torch.uint8, device=DEV)
    mask[[1, 16, 17, 64]] = 0
    on = mask.bool().cpu()
    out, before, after = [t.cpu() for t in _raw(v, net, traj, pose if v & 2 else None, vel if v & 1 else None, mask, -7.5)]
    assert torch.equal(out[~on], traj.cpu()[~on]) and bool((before[~on] == -7.5).all()) and bool((after[~on] == -7.5).all())
    for got, want in zip((out, before, after), whole):
        assert got[on].numpy().tobytes() == want.cpu()[on].numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------ 5
def test_bad_arguments_return_minus_one(nets):
    from emloco_amd.predictor import ops
    net = nets[3]
    traj, pose, vel = _inputs(4)
    out, vb, va = torch.full_like(traj, -3.0), torch.full((4,), -7.5, device=DEV), torch.full((4,), -7.5, device=DEV)
    ps = [p.contiguous() for p in params_of(net)]
    good = dict(variant=3, B=4, traj=traj.data_ptr(), ts=2, pose=pose.data_ptr(), vel=vel.data_ptr(),
                **{k: p.data_ptr() for k, p in zip(("w1", "b1", "w2", "b2", "w3", "b3"), ps)}, row_mask=None, n_steps=3, lr=1e-4, beta1=0.9,
                beta2=0.999, eps=1e-8, grad_scale=1.0, anchor_w=0.0, traj_out=out.data_ptr(), value_before=vb.data_ptr(),
                value_after=va.data_ptr(), grad0=None, stream=None)

    def call(**over):
        return ops._lib().emloco_locoval_refine(*{**good, **over}.values())
    bad_argument_cases(call, good)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((vb == -7.5).all()) and bool((va == -7.5).all())       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != -3.0).all()) and bool((va != -7.5).all())
    with pytest.raises(ValueError, match="steps >= 1"):
        ops.locoval_refine(3, traj, pose, vel, ps, 0, want_grad0=True)


# ------------------------------------------------------------------------------------------------------------ 6
def test_evaluate_with_refine_steps_equals_refine_applied_by_hand(tmp_path):
    from torch.utils.data import DataLoader
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from emloco_amd.predictor import evaluate_jta as EV
    from emloco_amd.predictor.dataset_jta import collate_batch, create_dataset, write_synthetic_split
    from emloco_amd.predictor.model_jta import TransMotionJTA
    N, M, steps, lr = 12, 20, 5, 1e-3
    write_synthetic_split(str(tmp_path), "test", N, max_people=3, seed=3)
    ds = create_dataset("jta_all_visual_cues", None, split="test", track_size=21, track_cutoff=9, preprocessed=True, root=str(tmp_path))
    config = {"DEVICE": DEV, "MULTI_MODAL": True, "NOISY_TRAJ": 0, "TRAIN": {"input_track_size": 9, "output_track_size": 12},
              "MODEL": {"value_threshold": 0.5}, "DATA": {"train_datasets": ["jta_all_visual_cues"]}}
    torch.manual_seed(4)
    model = TransMotionJTA(tok_dim=453, nhid=128, nhead=4, dim_feedfwd=64, nlayers_local=2, nlayers_global=2, nmode=M, output_scale=1,
                           obs_and_pred=21, num_tokens=49, device=DEV, multi_modal=True).to(DEV).eval()
    vnet = ValuePoseNet(True, True).to(DEV).eval()
    seen, inner = [], EV.inference
    replay = []

    def recording(*a, **kw):                                  # the predictor's forward need not repeat bit for bit from run to run:
        seen.append(inner(*a, **kw).clone())                  # the plain run records its predictions, the refining run scores the same ones
        return seen[-1].clone()

    def replaying(*a, **kw):
        return replay.pop(0).clone()
    loader = lambda: DataLoader(ds, batch_size=5, num_workers=0, shuffle=False, collate_fn=collate_batch)
    ids = torch.arange(N) % M
    kw = dict(dataset="jta", random_ids=ids, reference_inplace_pose=False)
    try:
        EV.inference = recording
        plain = EV.evaluate_ade_fde(model, vnet, "test", "traj+all", loader(), 5, config, **kw)
        EV.inference, replay = replaying, list(seen)
        col = EV.PredTrajCollector("best")
        res = EV.evaluate_ade_fde(model, vnet, "test", "traj+all", loader(), 5, config, pred_trajs=col, refine_steps=steps, refine_lr=lr, **kw)
    finally:
        EV.inference = inner
    assert len(seen) == 3 and not replay and seen[0].reshape(5, 12, -1, 2).shape[2] == M
    assert res["refine_steps"] == steps and res["ade_unrefined"] == plain["ade"] and res["value_mean_unrefined"] == plain["value_mean"]
    assert res["value_mean"] >= res["value_mean_unrefined"]
    assert 0 < res["refine_shift_mean"] <= res["refine_shift_max"] <= steps * lr * 1.01
    # by hand: the same predictions through ValuePoseNet.refine, scored by a fresh accumulator
    acc = EV.EvalAccumulator(0.5, reference_inplace_pose=False)
    shifts, off = [], 0
    for (joints, masks, pad), pred in zip(loader(), seen):
        from emloco_amd.predictor.train_jta import batch_process_coords
        B = joints.shape[0]
        ij, _, oj, _, _ = batch_process_coords(joints, masks, pad.to(DEV), config, "traj+all")
        pose = joints[:, 0, 8, 3:27, :3].to(DEV).float().clone()
        pose[..., 2] = -pose[..., 2]
        vel = ((ij[:, 8, 0, :2] - ij[:, 7, 0, :2]) * 2.5).to(DEV).float()
        p = pred.reshape(B, 12, M, 2).float().permute(0, 2, 1, 3)                                   # (B, M, 12, 2)
        traj = torch.cat([torch.zeros(B, M, 1, 2, device=DEV), p], 2).reshape(B * M, 13, 2).contiguous()
        out, _, after = vnet.refine(traj, pose[:, None].expand(B, M, 24, 3).reshape(B * M, 24, 3), vel[:, None].expand(B, M, 2).reshape(B * M, 2),
                                    steps=steps, lr=lr)
        shifts.append((out - traj)[:, 1:].abs().double().reshape(-1))
        refined = out[:, 1:].reshape(B, M, 12, 2).permute(0, 2, 1, 3).reshape(pred.shape)
        acc.update(ij, oj, refined, joints[:, 0, 8, 3:27, :3], vnet, ids[off:off + B], "jta")
        off += B
    want = acc.summary()
    for k, val in want.items():
        if isinstance(val, np.ndarray):
            np.testing.assert_array_equal(res[k], val, err_msg=k)
        else:
            assert res[k] == val, k
    shifts = torch.cat(shifts)
    assert res["refine_shift_max"] == float(shifts.max()) and abs(res["refine_shift_mean"] - float(shifts.mean())) <= 1e-12
    assert len(col.entries) == N and all(e["refined"] is True and e["locoval"] >= e["locoval_unrefined"] - 1e-6 for e in col.entries.values())

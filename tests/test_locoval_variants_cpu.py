"""CPU: the four LocoVal input configurations (value_pose_net.py:22-50) against the reference's own ValuePoseNet.

Fixture tests/golden/locoval_variants.npz comes from the reference's class on the CPU (tests/golden/gen_golden_locoval_variants.py).
Here:
  * `restate`, a plain-torch statement of the network of one variant (test infrastructure; the product runs it as HIP kernels),
    reproduces the fixture;
  * the kernels of emloco_amd/csrc/locoval_variants.h, compiled for the CPU through tests/emu/hip/ and launched through the product's
    own dispatch (tests/emu/emu_predictor.cpp), give the fixture's values, in-place pose and gradients at the tolerances of the
    full network's device test (tests/test_gpu_predictor.py:90-97);
  * the sparse `row_weight` / `slot` / `count` modes, batches that do not fill a wave, the full network through the variant entry
    points (the old entry points' bits), checkpoints and host-side errors.
"""
import os

import numpy as np
import pytest
import torch

import emu
from locoval_harness import DIMS, _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "locoval_variants.npz")
VARIANTS = {"full": 3, "pose": 2, "vel": 1, "traj": 0}           # (use_pose << 1) | use_vel
PARAM_KEYS = ("_network_fc1_weight", "_network_fc1_bias", "_network_fc2_weight", "_network_fc2_bias", "_network_fc3_weight", "_network_fc3_bias")
HIDDEN = (4, 8, 9, 10, 11)
VALUE_TOL = dict(rtol=1e-5, atol=1e-6)          # value and in-place pose
GRAD_TOL = dict(rtol=2e-4, atol=1e-7)           # all gradients


def fixture(name=None):
    fx = dict(np.load(FIXTURE))
    if name is None:
        return fx
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


def restate(variant, traj, pose, vel, params):
    """value_pose_net.py:73-147 in plain torch, any dtype: returns (value [B, 1], the caller's pose after the call)."""
    w1, b1, w2, b2, w3, b3 = params
    B = traj.shape[0]
    x1 = traj[:, 1, 0]
    x1 = torch.where(x1.abs() < 1e-10, torch.full_like(x1, 1e-10), x1)
    ang = torch.atan2(traj[:, 1, 1], x1)
    c, s = torch.cos(ang), torch.sin(ang)
    R = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], 1)
    feats = [torch.bmm(traj[..., :2], R).reshape(B, 26)]
    pose_after = None
    if pose is not None:
        pose_after = torch.cat([torch.bmm(pose[..., :2], R), pose[..., 2:]], -1)
        if variant & 2:
            keep = torch.ones(24, dtype=pose.dtype, device=pose.device)
            keep[list(HIDDEN)] = 0
            pose_after = pose_after * keep[None, :, None]
            feats.append(pose_after.reshape(B, 72))
    if variant & 1:
        feats.append(torch.bmm(vel[:, None, :], R)[:, 0])
    h = torch.relu(torch.cat(feats, -1) @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    return torch.sigmoid(h @ w3.T + b3), pose_after


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(VARIANTS))
def test_restatement_reproduces_the_reference(name):
    fx, v = fixture(name), VARIANTS[name]
    t = lambda a: torch.from_numpy(np.array(a))
    params = [t(fx[k]).requires_grad_(True) for k in PARAM_KEYS]
    traj = t(fx["traj"]).requires_grad_(True)
    value, pose_after = restate(v, traj, t(fx["pose"]), t(fx["vel"]), params)
    np.testing.assert_allclose(value.detach().numpy(), fx["value"], **VALUE_TOL)
    np.testing.assert_allclose(pose_after.detach().numpy(), fx["pose_after_inplace"], **VALUE_TOL)
    ((value - 1) ** 2).mean().backward()
    np.testing.assert_allclose(traj.grad.numpy(), fx["grad_traj"], **GRAD_TOL)
    for k, p in zip(PARAM_KEYS, params):
        np.testing.assert_allclose(p.grad.numpy(), fx["grad_" + k], **GRAD_TOL)
    assert tuple(fx["dims"]) == DIMS[v]
    # the fixture's own coverage: the epsilon guard, a pose that is rotated but not zeroed where it is not an input
    assert fx["traj"][0, 1, 0] == 0.0 and fx["traj"].shape[-1] == 3
    zeroed = bool((fx["pose_after_inplace"][:, list(HIDDEN)] == 0).all())
    assert zeroed == bool(v & 2) and not np.allclose(fx["pose_after_inplace"][:, 0], fx["pose"][:, 0])


# ------------------------------------------------------------------------------------------------------------ the kernels, emulated
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


class Run:
    """One forward (+ backward) of a variant through the emulated kernels; `old=True`: the full network's own entry points."""

    def __init__(self, variant, params, traj, pose, vel, row_weight=None, fill=None, pose_rot=False, old=False):
        self.lib, self.v, self.old = emu.lib(), variant, old
        n_in, h1, h2, self.n_param = DIMS[variant]
        self.B, self.ts = traj.shape[0], traj.shape[-1]
        self.params = [_f32(p) for p in params]
        self.traj, self.pose, self.vel = _f32(traj), _f32(pose), _f32(vel)
        mk = (lambda *s: np.full(s, fill, np.float32)) if fill is not None else (lambda *s: np.zeros(s, np.float32))
        self.value, self.x, self.h1, self.h2, self.ang = mk(self.B), mk(self.B, n_in), mk(self.B, h1), mk(self.B, h2), mk(self.B)
        self.pose_rot = mk(self.B, 24, 3) if pose_rot else None
        self.forward(row_weight)

    def forward(self, row_weight=None):
        rw = _f32(row_weight)
        out = [_ptr(a) for a in (self.value, self.x, self.h1, self.h2, self.ang)]
        if self.old:
            rc = self.lib.emu_locoval_fwd(self.B, _ptr(self.traj), self.ts, _ptr(self.pose), _ptr(self.vel), *[_ptr(p) for p in self.params],
                                          *out, _ptr(rw))
        else:
            rc = self.lib.emu_locoval_variant_fwd_rows(self.v, self.B, _ptr(self.traj), self.ts, _ptr(self.pose), _ptr(self.vel),
                                                       *[_ptr(p) for p in self.params], *out, _ptr(self.pose_rot), _ptr(rw))
        assert rc == 0

    def backward(self, dvalue, slot=None, count=None, fill=0.0):
        dv = _f32(dvalue)
        self.dparams, self.dtraj = np.full(self.n_param, fill, np.float32), np.full(self.traj.shape, fill, np.float32)
        ws = np.zeros(self.B * self.n_param, np.float32)
        w1, _b1, w2, _b2, w3, _b3 = self.params
        args = [self.B, _ptr(self.traj), self.ts, _ptr(self.pose), _ptr(self.vel), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(self.value), _ptr(self.x),
                _ptr(self.h1), _ptr(self.h2), _ptr(self.ang), _ptr(dv), _ptr(slot), _ptr(count), _ptr(self.dparams), _ptr(self.dtraj), _ptr(ws)]
        rc = self.lib.emu_locoval_bwd(*args) if self.old else self.lib.emu_locoval_variant_bwd_rows(self.v, *args)
        assert rc == 0
        return self

    def split(self):
        n_in, h1, h2, _ = DIMS[self.v]
        sizes = [h1 * n_in, h1, h2 * h1, h2, h2, 1]
        shapes = [(h1, n_in), (h1,), (h2, h1), (h2,), (1, h2), (1,)]
        parts = np.split(self.dparams, np.cumsum(sizes)[:-1])
        return [p.reshape(s) for p, s in zip(parts, shapes)]


def _inputs(fx, v):
    """what the variant reads (the others NULL)"""
    return fx["traj"], (fx["pose"] if v & 2 else None), (fx["vel"] if v & 1 else None)


def test_variant_dims_query():
    from emloco_amd.predictor.ops import locoval_dims, locoval_variant
    for v, want in DIMS.items():
        d = np.zeros(4, np.int32)
        assert emu.lib().emu_locoval_variant_dims(v, _ptr(d)) == 0 and tuple(d) == want == locoval_dims(v)
    assert emu.lib().emu_locoval_variant_dims(4, _ptr(np.zeros(4, np.int32))) != 0
    assert [locoval_variant(p, v) for p, v in ((1, 1), (1, 0), (0, 1), (0, 0))] == [3, 2, 1, 0]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_kernels_match_the_reference(name):
    fx, v = fixture(name), VARIANTS[name]
    params = [fx[k] for k in PARAM_KEYS]
    B = fx["traj"].shape[0]
    assert B % 4 != 0
    # the pose is handed over in every variant: rotated in place where it is not an input, rotated and zeroed where it is
    traj, pose, vel = _inputs(fx, v)
    r = Run(v, params, traj, fx["pose"], vel, pose_rot=not (v & 2))
    np.testing.assert_allclose(r.value.reshape(B, 1), fx["value"], **VALUE_TOL)
    pose_after = r.x[:, 26:98].reshape(B, 24, 3) if v & 2 else r.pose_rot
    np.testing.assert_allclose(pose_after, fx["pose_after_inplace"], **VALUE_TOL)
    if not v & 2:                                               # ... and the value does not depend on it
        assert np.array_equal(Run(v, params, traj, None, vel).value, r.value)
    # EmLoco loss: MSE to 1, mean over the batch
    r.backward(2.0 * (r.value - 1.0) / B)
    np.testing.assert_allclose(r.dtraj, fx["grad_traj"], **GRAD_TOL)
    for k, g in zip(PARAM_KEYS, r.split()):
        np.testing.assert_allclose(g, fx["grad_" + k], **GRAD_TOL, err_msg=k)
    # the rollout's fit: sum-MSE to a target
    np.testing.assert_allclose(r.value.reshape(B, 1), fx["fit_value"], **VALUE_TOL)
    r.backward(2.0 * (r.value - fx["target"].reshape(B)))
    for k, g in zip(PARAM_KEYS, r.split()):
        np.testing.assert_allclose(g, fx["fitgrad_" + k], **GRAD_TOL, err_msg=k)
    fit_loss = float(((r.value.astype(np.float64) - fx["target"].reshape(B)) ** 2).sum())
    np.testing.assert_allclose(fit_loss, float(fx["fit_loss"]), rtol=1e-5)


def _random_batch(B, seed, ts=3):
    g = torch.Generator().manual_seed(seed)
    traj = torch.cumsum(torch.randn(B, 13, ts, generator=g) * 0.3 + 0.2, dim=1)
    traj[:, 0] = 0
    return traj.numpy(), (torch.randn(B, 24, 3, generator=g) * 0.3).numpy(), torch.randn(B, 2, generator=g).numpy()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_rows_mode_touches_only_the_ranked_rows(name):
    fx, v = fixture(name), VARIANTS[name]
    params = [fx[k] for k in PARAM_KEYS]
    B = 37
    traj, pose, vel = _random_batch(B, 7 + v)
    pose, vel = (pose if v & 2 else None), (vel if v & 1 else None)
    weight = np.zeros(B, np.float32)
    weight[[2, 3, 17, 20, 36]] = 1.0                           # most rows left out; two in one wave, the batch's last row
    on = weight != 0
    dense = Run(v, params, traj, pose, vel)
    rows = Run(v, params, traj, pose, vel, row_weight=weight, fill=-7.5)
    for a, b in ((rows.value, dense.value), (rows.x, dense.x), (rows.h1, dense.h1), (rows.h2, dense.h2), (rows.ang, dense.ang)):
        assert np.array_equal(a[on], b[on]) and (a[~on] == -7.5).all()
    # ranks from the product's own fit-gradient kernel, as the rollout's fit takes them
    target = np.linspace(0.1, 0.9, B).astype(np.float32)
    dvalue, tail, slot = np.zeros(B, np.float32), np.zeros(2, np.float32), np.zeros(B, np.int32)
    assert emu.lib().emu_locoval_fit_grad(B, _ptr(dense.value), _ptr(target), _ptr(weight), _ptr(dvalue), _ptr(tail), _ptr(slot)) == 0
    assert tail[1] == on.sum() and list(slot[on]) == list(range(int(on.sum()))) and (slot[~on] == -1).all() and (dvalue[~on] == 0).all()
    sparse = dense.backward(dvalue, slot=slot, count=tail[1:].copy(), fill=-7.5)
    sp_dparams, sp_dtraj = sparse.dparams.copy(), sparse.dtraj.copy()
    full = dense.backward(dvalue)                               # dense, zero dvalue elsewhere
    assert np.array_equal(sp_dparams, full.dparams)
    assert np.array_equal(sp_dtraj[on], full.dtraj[on]) and (sp_dtraj[~on] == -7.5).all() and (full.dtraj[~on] == 0).all()
    assert np.abs(full.dparams).max() > 0


@pytest.mark.parametrize("mode", ["dense", "rows"])
def test_full_variant_through_the_new_entry_points_gives_the_old_bits(mode):
    fx = fixture("full")
    params = [fx[k] for k in PARAM_KEYS]
    B = 21
    traj, pose, vel = _random_batch(B, 3)
    weight = None
    if mode == "rows":
        weight = np.zeros(B, np.float32)
        weight[[0, 5, 6, 20]] = 1.0
    new = Run(3, params, traj, pose, vel, row_weight=weight, fill=2.5)
    old = Run(3, params, traj, pose, vel, row_weight=weight, fill=2.5, old=True)
    for k in ("value", "x", "h1", "h2", "ang"):
        assert getattr(new, k).tobytes() == getattr(old, k).tobytes(), k
    dvalue = np.linspace(-1, 1, B).astype(np.float32)
    slot = count = None
    if mode == "rows":
        new.forward(), old.forward()                            # activations of every row for the backward
        slot = np.where(weight != 0, np.cumsum(weight != 0) - 1, -1).astype(np.int32)
        count = np.array([float((weight != 0).sum())], np.float32)
        dvalue = dvalue * weight
    new.backward(dvalue, slot, count, fill=2.5), old.backward(dvalue, slot, count, fill=2.5)
    assert new.dparams.tobytes() == old.dparams.tobytes() and new.dtraj.tobytes() == old.dtraj.tobytes()
    assert np.abs(new.dparams).max() > 0


@pytest.mark.parametrize("name", ["vel", "traj", "pose"])
def test_batches_that_do_not_fill_a_wave(name):
    """Four samples share a wave and sixteen a workgroup in the narrow kernels: a sample's results do not depend on its neighbours, on
    the batch size or on where the batch ends; checked against the float64 restatement as well."""
    fx, v = fixture(name), VARIANTS[name]
    params = [fx[k] for k in PARAM_KEYS]
    Bmax = 35
    traj, pose, vel = _random_batch(Bmax, 11 + v, ts=2)         # stride 2: the tightest trajectory layout
    traj[4, 1, 0] = 0.0                                         # the epsilon guard inside a packed wave
    dvalue = np.linspace(-1, 1, Bmax).astype(np.float32)
    sel = lambda a, n: None if a is None else a[:n]
    pose_in, vel_in = (pose if v & 2 else None), (vel if v & 1 else None)
    big = Run(v, params, traj, pose_in, vel_in).backward(dvalue)
    t64 = lambda a: torch.from_numpy(np.array(a)).double()
    p64 = [t64(p).requires_grad_(True) for p in params]
    tr64 = t64(traj).requires_grad_(True)
    value64, _ = restate(v, tr64, t64(pose), t64(vel), p64)
    (value64.reshape(-1) * t64(dvalue)).sum().backward()
    np.testing.assert_allclose(big.value, value64.detach().numpy().reshape(-1), **VALUE_TOL)
    np.testing.assert_allclose(big.dtraj, tr64.grad.numpy(), **GRAD_TOL)
    for g, p in zip(big.split(), p64):
        np.testing.assert_allclose(g, p.grad.numpy(), **GRAD_TOL)
    for n in (1, 2, 3, 5, 16, 17, 18):
        r = Run(v, params, traj[:n], sel(pose_in, n), sel(vel_in, n), fill=9.0).backward(dvalue[:n], fill=9.0)
        for k in ("value", "x", "h1", "h2", "ang", "dtraj"):
            assert getattr(r, k).tobytes() == getattr(big, k)[:n].tobytes(), (k, n)
        assert np.isfinite(r.dparams).all()
        if n == 1:                                              # a batch of one: its parameter gradient is that sample's share
            one64 = [t64(p).requires_grad_(True) for p in params]
            v1, _ = restate(v, t64(traj[:1]), t64(pose[:1]), t64(vel[:1]), one64)
            (v1.reshape(-1) * t64(dvalue[:1])).sum().backward()
            for g, p in zip(r.split(), one64):
                np.testing.assert_allclose(g, p.grad.numpy(), **GRAD_TOL)


# ------------------------------------------------------------------------------------------------------------ checkpoints, host errors
@pytest.mark.parametrize("name", list(VARIANTS))
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    fx, v = fixture(name), VARIANTS[name]
    net = ValuePoseNet(use_pose=bool(v & 2), use_vel=bool(v & 1))
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in fx["state_keys"]]
    for k in sd:
        assert tuple(sd[k].shape) == fx[k.replace(".", "_")].shape, k
    assert sum(p.numel() for p in net.parameters()) == DIMS[v][3] == net.n_param and net.layer_sizes == DIMS[v][:3]
    ref = {str(k): torch.from_numpy(fx[str(k).replace(".", "_")]) for k in fx["state_keys"]}
    net.load_state_dict(ref, strict=True)                       # the reference's checkpoint of this variant
    assert torch.equal(net._network.fc1.weight, ref["_network.fc1.weight"])


def test_checkpoint_of_another_variant_fails_naming_both_shapes():
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    vel_net = ValuePoseNet(use_pose=False, use_vel=True)
    for p, v, txt in ((True, True, "100 -> 49"), (True, False, "98 -> 48"), (False, False, "26 -> 12")):
        with pytest.raises(RuntimeError) as e:
            vel_net.load_state_dict(ValuePoseNet(use_pose=p, use_vel=v).state_dict())
        assert txt in str(e.value) and "28 -> 13" in str(e.value), str(e.value)


def test_unsupported_flags_still_raise():
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    for kw in (dict(hide_toe=False), dict(hide_spine=False), dict(normalize=False), dict(vru=True)):
        with pytest.raises(NotImplementedError):
            ValuePoseNet(use_pose=False, use_vel=False, **kw)


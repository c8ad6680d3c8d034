"""GPU: the reduced-input LocoVal networks (pose / vel / traj; emloco_amd/csrc/locoval_variants.h) on the MI355X.

  (a) ValuePoseNet of every variant against the reference's fixture (tests/golden/locoval_variants.npz) at the tolerances of the full
      network's test (tests/test_gpu_predictor.py:90-97), and the kernels against float64 torch at B = 4096;
  (b) LocoValRollout of the three new variants against a per-step stock-torch fit on the kernels' captured inputs;
  (c) the `--test` player with a velocity-only and a trajectory-only checkpoint;
  (d) train_jta --not_pose and evaluate_jta --no_pose from the shipped yaml;
  (e) forward-rows + backward-rows of all four variants timed in one process.
The stock-torch statement of the networks (`restate`, `TorchVariantNet`) is test infrastructure.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from locoval_harness import DIMS  # noqa: E402
from test_locoval_variants_cpu import GRAD_TOL, VALUE_TOL, VARIANTS, fixture, restate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]
NEW = ["pose", "vel", "traj"]


def _flags(v):
    return (["--input_init_pose"] if v & 2 else []) + (["--input_init_vel"] if v & 1 else [])


class TorchVariantNet(torch.nn.Module):
    """Stock torch: the network of one variant with nn.Linear layers under the reference's parameter names."""

    def __init__(self, variant):
        super().__init__()
        n_in, h1, h2, _ = DIMS[variant]
        self.variant = variant
        self._network = torch.nn.Sequential()
        self._network.add_module("fc1", torch.nn.Linear(n_in, h1))
        self._network.add_module("fc2", torch.nn.Linear(h1, h2))
        self._network.add_module("fc3", torch.nn.Linear(h2, 1))

    def forward(self, traj, pose, vel):
        n = self._network
        return restate(self.variant, traj, pose, vel, (n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias))[0]


def _net(name, dev, seed=None, **kw):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    v = VARIANTS[name]
    if seed is not None:
        torch.manual_seed(seed)
    return ValuePoseNet(use_pose=bool(v & 2), use_vel=bool(v & 1), **kw).to(dev)


# ------------------------------------------------------------------------------------------------ (a) device against the fixture
@pytest.mark.parametrize("name", list(VARIANTS))
def test_value_pose_net_matches_the_reference_fixture(name):
    fx, v, dev = fixture(name), VARIANTS[name], "cuda:0"
    net = _net(name, dev)
    net.load_state_dict({k: torch.from_numpy(fx[k.replace(".", "_")]) for k in net.state_dict()}, strict=True)
    traj = torch.from_numpy(fx["traj"]).to(dev).requires_grad_(True)
    pose = torch.from_numpy(fx["pose"]).to(dev)
    vel = torch.from_numpy(fx["vel"]).to(dev) if v & 1 else None
    value, loss = net.calc_embodied_motion_loss(traj, pose, vel)
    np.testing.assert_allclose(value.detach().cpu().numpy(), fx["value"], **VALUE_TOL)
    np.testing.assert_allclose(pose.cpu().numpy(), fx["pose_after_inplace"], **VALUE_TOL)      # rotated in place in every variant
    np.testing.assert_allclose(float(loss.detach()), float(fx["loss"]), rtol=1e-5)
    loss.backward()
    np.testing.assert_allclose(traj.grad.cpu().numpy(), fx["grad_traj"], **GRAD_TOL)
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), fx["grad_" + k.replace(".", "_")], **GRAD_TOL, err_msg=k)
    # the rollout's sum-reduction fit; the variants that do not read the pose run without one
    net.zero_grad()
    v2 = net(torch.from_numpy(fx["traj"]).to(dev), torch.from_numpy(fx["pose"]).to(dev) if v & 2 else None, vel)
    np.testing.assert_allclose(v2.detach().cpu().numpy(), fx["fit_value"], **VALUE_TOL)
    torch.nn.MSELoss(reduction="sum")(v2, torch.from_numpy(fx["target"]).to(dev)).backward()
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), fx["fitgrad_" + k.replace(".", "_")], **GRAD_TOL, err_msg=k)


def _embed_in_full(net, dev):
    """The full (100 / 49 / 24) network that computes the SAME function as the reduced network `net`: its weights at the inputs and
    units `net` has, exact zeros elsewhere (a zero weight adds an exact zero to every sum; a unit with zero weights and bias stays at
    relu(0) = 0 and passes no gradient).  Returns the network and, per parameter, the index of `net`'s entries inside it."""
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    n_in, h1, h2, _ = DIMS[net.variant]
    cols = list(range(26)) + (list(range(26, 98)) if net.variant & 2 else []) + ([98, 99] if net.variant & 1 else [])
    cols = torch.tensor(cols, device=dev)
    full = ValuePoseNet(True, True, inplace_pose=False).to(dev)
    src, dst = net._network, full._network
    with torch.no_grad():
        for p in full.parameters():
            p.zero_()
        dst.fc1.weight[:h1, cols] = src.fc1.weight
        dst.fc1.bias[:h1] = src.fc1.bias
        dst.fc2.weight[:h2, :h1] = src.fc2.weight
        dst.fc2.bias[:h2] = src.fc2.bias
        dst.fc3.weight[:, :h2] = src.fc3.weight
        dst.fc3.bias.copy_(src.fc3.bias)
    pick = [lambda g: g[:h1][:, cols], lambda g: g[:h1], lambda g: g[:h2, :h1], lambda g: g[:h2], lambda g: g[:, :h2], lambda g: g]
    return full, pick


def _float64_errors(name, B=4096, seed=17):
    """Largest error of value / d traj / d parameters against float64 torch, each relative to the largest float64 entry, at B = 4096
    with random inputs: of the variant's kernels (`variant`) and of the full network's existing kernels (`full`) on the same inputs
    AND the same function -- the variant's weights embedded in a full network (`_embed_in_full`).  How large such an error is depends
    on the function as much as on the kernel (cancellation in the batch sums, a first waypoint near the origin in the angle's
    gradient: between two random networks the same kernel's figure moves by 2-5 x), so the full kernels are measured on the function
    the variant computes; what is left between the two figures is the kernels' summation order and length."""
    v, dev = VARIANTS[name], "cuda:0"
    net = _net(name, dev, seed=seed + v, inplace_pose=False)
    g = torch.Generator().manual_seed(seed)
    traj = torch.cumsum(torch.randn(B, 13, 3, generator=g) * 0.3 + torch.tensor([0.5, 0.1, 0.0]), dim=1)
    traj[:, 0] = 0
    pose, vel, dvalue = torch.randn(B, 24, 3, generator=g) * 0.3, torch.randn(B, 2, generator=g), torch.randn(B, 1, generator=g)
    ref = TorchVariantNet(v).double().to(dev)
    ref.load_state_dict({k: p.detach().double() for k, p in net.state_dict().items()})
    t64 = traj.double().to(dev).requires_grad_(True)
    value64 = ref(t64, pose.double().to(dev), vel.double().to(dev))
    (value64 * dvalue.double().to(dev)).sum().backward()
    gp64 = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())

    def errors(model, pick):
        t32 = traj.to(dev).requires_grad_(True)
        value = model(t32, pose.to(dev), vel.to(dev))
        (value * dvalue.to(dev)).sum().backward()
        gp = torch.cat([f(p.grad).reshape(-1) for f, p in zip(pick, model.parameters())])
        return {"value": rel(value.detach(), value64.detach()), "grad_traj": rel(t32.grad, t64.grad), "grad_params": rel(gp, gp64)}
    out = {"variant": errors(net, [lambda g_: g_] * 6)}
    out["full"] = out["variant"] if v == 3 else errors(*_embed_in_full(net, dev))
    return out


@pytest.fixture(scope="module")
def float64_errors():
    return {name: _float64_errors(name) for name in VARIANTS}


def test_variant_kernels_against_float64_within_twice_the_full_kernels_error(float64_errors):
    """Bar: what the full network's existing kernels show against float64 on the same inputs and the same function in this run
    (`_float64_errors`), times 2 (the margin covers the variants' different summation lengths)."""
    print("float64 errors:", json.dumps(float64_errors))
    for name in VARIANTS:
        assert all(0 < e < 1e-4 for e in float64_errors[name]["full"].values()), (name, float64_errors[name])
    for name in NEW:
        got, full = float64_errors[name]["variant"], float64_errors[name]["full"]
        for k, e in got.items():
            assert e <= 2.0 * full[k], (name, k, e, full[k])


# ------------------------------------------------------------------------------------------------ (b) the rollout fit per variant
def _make_env(num_envs, flags):
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", *ENV_ARGS, *flags])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    return args, RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))


@pytest.mark.parametrize("name", NEW)
def test_rollout_fits_the_variant_network_like_a_per_step_torch_fit(name):
    """LocoValRollout(use_pose, use_vel) as `run.py` builds it from its flags, 128 envs, 6 epochs of 8 steps with natural resets.  The
    staged inputs of every fit (trajectory, pose, velocity, target, weight) are copied as the fit reads them; a stock-torch network
    of the same variant is fitted on them step by step (autograd of MSELoss(reduction='sum'), torch.optim.AdamW(1e-3, wd 1e-4), the
    epoch's learning rate) and after EVERY epoch the fit counters are equal, loss and parameters agree at the tolerances of the
    repository's kernels-against-torch rollout comparison (tests/test_gpu_dist.py:296-299: loss 1e-5 relative, parameters
    rtol 1e-4 / atol 1e-5; the comparisons of tests/test_gpu_env.py between two schedules of the SAME kernels are bit-equal, which
    autograd's own summation order cannot be)."""
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    v, E = VARIANTS[name], 128
    args, env = _make_env(E, _flags(v))
    task = env.env.task
    dev = task.device
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    pool = torch.randn(8, E, 69, device=dev, generator=g) * 0.3
    k = [0]

    def pol(obs):
        k[0] += 1
        return pool[k[0] % 8]
    torch.manual_seed(5)
    agent = LocoValRollout(env, use_pose=args.input_init_pose, use_vel=args.input_init_vel, horizon_length=8, policy=pol, overlap_reset=False,
                           warmup_epochs=3, max_epochs=40)
    n_param = DIMS[v][3]
    assert agent.valuenet.variant == v and agent.bucket.flat.numel() == n_param + 2 and agent.bucket.grads.numel() == n_param
    assert agent._fz["ws"].numel() == E * n_param and agent._fz["m"].numel() == n_param and agent._fz["x100"].shape == (E, DIMS[v][0])
    ref = TorchVariantNet(v).to(dev)
    ref.load_state_dict({k_: p.detach().clone() for k_, p in agent.valuenet.state_dict().items()})
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-4)
    captured, inner = [], agent._fit_launches

    def capturing(st, stage=None):
        z = dict(agent._fz)
        if stage is not None:
            z.update(stage)
        captured.append(tuple(z[n].clone() for n in ("traj13", "pose", "vel", "target", "weight")) + (float(agent.vnet_optimizer.param_groups[0]["lr"]),))
        inner(st, stage)
    agent._fit_launches = capturing
    fits = episodes = 0
    last_loss = 0.0
    for epoch in range(6):
        loss = agent.play_steps()                          # (reads the loss: flushes and waits for the fit stream)
        assert len(captured) == 8
        for traj13, pose, vel, target, weight, lr in captured:
            on = weight != 0
            n = int(on.sum())
            if n == 0:
                continue                                   # the gated AdamW leaves the network alone
            for grp in opt.param_groups:
                grp["lr"] = lr
            opt.zero_grad()
            pred = ref(traj13[on], pose[on], vel[on]).reshape(-1)
            step_loss = torch.nn.MSELoss(reduction="sum")(pred, target[on])
            step_loss.backward()
            opt.step()
            fits, episodes, last_loss = fits + 1, episodes + n, float(step_loss) / n
        captured.clear()
        assert agent.vnet_fits == fits and agent.fitted_episodes == episodes, (epoch, agent.vnet_fits, fits, agent.fitted_episodes, episodes)
        assert abs(float(loss) - last_loss) <= 1e-5 * max(1.0, abs(last_loss)), (epoch, float(loss), last_loss)
        for (kn, p), q in zip(agent.valuenet.named_parameters(), ref.parameters()):
            assert torch.allclose(p, q, rtol=1e-4, atol=1e-5), (epoch, kn, float((p - q).abs().max()))
    assert episodes > 5 and fits > 3
    agent.detach()


# ------------------------------------------------------------------------------------------------ (c) the --test player
@pytest.mark.parametrize("name", ["vel", "traj"])
def test_player_records_the_variant_networks_values(name, tmp_path):
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    v, E = VARIANTS[name], 64
    _args, env = _make_env(E, _flags(v))
    task = env.env.task
    dev = torch.device(task.device)
    torch.manual_seed(21)
    bundle = AMPPolicyBundle(task, deterministic=True)
    vnet = _net(name, dev, seed=11).eval()
    ev = LocoValEvaluator(env, bundle, vnet, games_num=2 * E)
    assert ev._x100.shape == (E, DIMS[v][0]) and ev._h1.shape == (E, DIMS[v][1])
    ref = TorchVariantNet(v).to(dev)
    ref.load_state_dict({k: p.detach().clone() for k, p in vnet.state_dict().items()})
    firsts, inner = [[] for _ in range(E)], ev._forward

    def capturing(st):
        b = ev._b
        with torch.no_grad():
            vals = ref(b["traj13"], b["pose"], b["vel"]).reshape(-1).cpu().numpy()
        for e in torch.nonzero(b["row_mask"]).flatten().tolist():      # the rows whose game takes its first step
            firsts[e].append(vals[e])
        inner(st)
    ev._forward = capturing
    rep = ev.run(say=None)
    got = ev.records()
    assert rep["games"] == 2 * E == len(got) and rep["shortfall"] == 0
    want = np.array([firsts[e][g] for e, g in zip(got["env"], got["game"])], np.float32)
    np.testing.assert_allclose(got["value"], want, rtol=1e-5)
    assert np.isfinite(got["value"]).all() and got["value"].std() > 0


@pytest.mark.parametrize("name", ["vel", "traj"])
def test_run_test_cli_with_a_reduced_checkpoint_prints_the_report(name, tmp_path):
    v = VARIANTS[name]
    path = str(tmp_path / "locoval.pth")
    torch.save({k: p.cpu() for k, p in _net(name, "cpu", seed=11).state_dict().items()}, path)
    out = str(tmp_path / "eval.json")
    base = [sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "32", "--seed", "1", *ENV_ARGS, "--policy_random_init",
            "--valuenet_path", path, "--games_num", "32", "--eval_out", out]
    p = subprocess.run(base + _flags(v), cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    for head in ("av reward: ", "av_loc: ", "std_loc: ", "Correlation: ", " Total reward: ", "Loc reward: ", "Pow reward: ", "Disc reward: "):
        assert any(ln.startswith(head) for ln in lines), head
    assert json.load(open(out))["games"] == 32
    # a flag that contradicts the checkpoint: the message names both shapes
    p = subprocess.run(base + ["--input_init_pose"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    n_in, h1 = DIMS[v][:2]
    assert p.returncode != 0 and f"{n_in} -> {h1}" in p.stderr and ("98 -> 48" in p.stderr or "100 -> 49" in p.stderr), p.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ (d) training / evaluation entry points
def test_train_jta_not_pose_and_evaluate_jta_no_pose_from_the_shipped_yaml(tmp_path):
    from torch.utils.data import DataLoader
    from emloco_amd.predictor.dataset_jta import collate_batch, create_dataset, write_synthetic_split
    from emloco_amd.predictor.model_jta import TransMotionJTA
    from emloco_amd.predictor.train_jta import EmLocoTrainer, evaluate_loss, load_checkpoint, save_checkpoint, train_epoch
    data, out = str(tmp_path / "data"), str(tmp_path / "experiments")
    for split, n in (("train", 24), ("valid", 12), ("test", 12)):
        write_synthetic_split(data, split, n, max_people=3, seed=len(split))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "emloco_amd.predictor.train_jta", "--exp_name", "v0", "--cfg", "configs/jta_all_visual_cues.yaml",
                        "--valueloss_w", "1.0", "--not_pose", "--dry-run", "--multi_modal", "--data_root", data, "--out_root", out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log = r.stderr + r.stdout
    assert "'USE_POSE': False" in log and "'USE_VELOCITY': True" in log
    assert np.isfinite(float(log.split("Train Loss: ")[1].split()[0]))
    assert os.path.exists(os.path.join(out, "JTA", "v0", "checkpoints", "best_val_checkpoint.pth.tar"))
    r = subprocess.run([sys.executable, "-m", "emloco_amd.predictor.evaluate_jta", "--exp_name", "v0", "--valueloss", "--multi_modal", "--no_pose",
                        "--filter_threshold", "0.5", "--data_root", data, "--out_root", out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log = r.stderr + r.stdout
    assert "Total samples: 12" in log and "ADE with Value sampling" in log
    assert np.isfinite(float(log.split("ADE: ")[1].split()[0]))
    # a few steps with the velocity-only network as the frozen loss: finite and decreasing; the checkpoint round-trips
    dev = "cuda:0"
    ds = create_dataset("jta_all_visual_cues", split="train", preprocessed=True, root=data)
    dl = DataLoader(ds, batch_size=4, collate_fn=collate_batch, shuffle=False)
    cfg = {"DEVICE": dev, "MULTI_MODAL": False, "USE_FRAME_MASK": False, "NOISY_TRAJ": 0, "OUTPUT": {"ckpt_dir": str(tmp_path)},
           "TRAIN": {"input_track_size": 9, "output_track_size": 12, "lr": 1e-3, "lr_decay": 1, "lr_drop": True, "epochs": 10,
                     "max_grad_norm": 1.0, "valuenet_weight": 1.0}}
    torch.manual_seed(0)
    mk = lambda: TransMotionJTA(tok_dim=453, nhid=128, nhead=4, dim_feedfwd=64, nlayers_local=1, nlayers_global=1, nmode=4, output_scale=1,
                                obs_and_pred=21, num_tokens=49, device=dev).to(dev)
    model = mk()
    trainer = EmLocoTrainer(model, _net("vel", dev, seed=3), cfg)
    losses = [train_epoch(trainer, dl, epoch) for epoch in range(4)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    l1 = evaluate_loss(model, dl, cfg)
    path = save_checkpoint(model, trainer.optimizer, 4, cfg, "checkpoint.pth.tar")
    m2 = mk()
    assert load_checkpoint(m2, path, strict=True) == 4
    assert abs(evaluate_loss(m2, dl, cfg) - l1) <= 1e-5 * max(1.0, l1)


# ------------------------------------------------------------------------------------------------ (e) timing
def _time_variants(rounds=40, warmup=5, B=4096):
    """forward-rows + backward-rows with every row active, all four variants interleaved in one process: median of `rounds` HIP-event
    timings each, in microseconds."""
    from emloco_amd.predictor import ops
    lib, dev = ops._lib(), torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    traj = torch.cumsum(torch.randn(B, 13, 3, generator=g) * 0.3 + 0.2, dim=1).to(dev)
    pose, vel = (torch.randn(B, 24, 3, generator=g) * 0.3).to(dev), torch.randn(B, 2, generator=g).to(dev)
    weight = torch.ones(B, device=dev)
    slot = torch.arange(B, dtype=torch.int32, device=dev)
    count = torch.full((1,), float(B), device=dev)
    dvalue = torch.randn(B, generator=g).to(dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    runs = {}
    for name, v in VARIANTS.items():
        n_in, h1, h2, n_param = DIMS[v]
        net = _net(name, dev, seed=5 + v)
        n = net._network
        w = [n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias]
        f = lambda *s: torch.zeros(*s, device=dev)
        z = dict(value=f(B), x=f(B, n_in), h1=f(B, h1), h2=f(B, h2), ang=f(B), dparams=f(n_param), dtraj=f(B, 13, 3), ws=f(B * n_param))

        def run(v=v, w=w, z=z):
            a = [B, P(traj), 3, P(pose), P(vel)]
            out = [P(z["value"]), P(z["x"]), P(z["h1"]), P(z["h2"]), P(z["ang"])]
            tail = [P(z["value"]), P(z["x"]), P(z["h1"]), P(z["h2"]), P(z["ang"]), P(dvalue), P(slot), P(count), P(z["dparams"]), P(z["dtraj"]),
                    P(z["ws"]), None]
            if v == 3:                                     # the full network through its own entry points, as the rollout calls them
                ops._chk(lib.emloco_locoval_fwd_rows(*a, *[P(t) for t in w], *out, P(weight), None), "fwd")
                ops._chk(lib.emloco_locoval_bwd_rows(*a, P(w[0]), P(w[2]), P(w[4]), *tail), "bwd")
            else:
                ops._chk(lib.emloco_locoval_variant_fwd_rows(v, *a, *[P(t) for t in w], *out, None, P(weight), None), "fwd")
                ops._chk(lib.emloco_locoval_variant_bwd_rows(v, *a, P(w[0]), P(w[2]), P(w[4]), *tail), "bwd")
        runs[name] = run
    times = {name: [] for name in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        for r in range(warmup + rounds):
            for name, run in runs.items():
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if r >= warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: float(np.median(t)) for name, t in times.items()}, {name: (float(np.min(t)), float(np.max(t))) for name, t in times.items()}


def test_no_reduced_variant_takes_longer_than_the_full_network(float64_errors, tmp_path):
    med, spread = _time_variants()
    lines = ["LocoVal forward-rows + backward-rows, B = 4096, every row active; HIP events, 5 warm-up rounds, median of 40 (min .. max),",
             "the four variants interleaved in one process.  float64 errors: largest |kernel - float64 torch| over largest |float64| of value /",
             "d traj / d parameters at B = 4096; in brackets the full network's kernels on the same inputs and the same function.",
             "variant   in   h1   h2  params    median us   (min .. max)        err value              err d traj             err d params"]
    for name, v in VARIANTS.items():
        e, f = float64_errors[name]["variant"], float64_errors[name]["full"]
        lines.append(f"{name:7s} {DIMS[v][0]:4d} {DIMS[v][1]:4d} {DIMS[v][2]:4d} {DIMS[v][3]:7d} {med[name]:12.1f}   ({spread[name][0]:.1f} .. {spread[name][1]:.1f})   "
                     + "   ".join(f"{e[k]:.2e} [{f[k]:.2e}]" for k in ("value", "grad_traj", "grad_params")))
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("EMLOCO_LOCOVAL_VARIANTS_TABLE") or str(tmp_path / "locoval_variants.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)
    for name in NEW:
        assert med[name] <= med["full"], (name, med)

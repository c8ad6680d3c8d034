"""GPU: the backward of the CNN policy's convolution trunk.  The kernels (emloco_cnn_trunk_backward) bit for bit against their CPU
emulation and within the float64 bar on the cases of tests/test_cnn_trunk_backward_cpu.py; the network module with
`enable_trunk_backward()` against a float64 CPU evaluation of a copy of itself; AMPAgent's loss and every gradient on the CNN network
against a plain-torch restatement (F.conv2d / F.linear in float64 on the CPU, the discriminator's gradient penalty by true double
backward); two training epochs with the captured optimiser step on a crowd task, and the checkpoint they write played by the bundle.
Bars: the float64 bar of the CPU tests for the kernel; `rel=3e-4, abs_=1e-6` of a tensor's largest value for gradients that pass the
GEMM backward (two bf16 pieces), the bar tests/test_gpu_policy.py holds agent gradients to; the loss to 1e-4 relative."""
import copy
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

import cnn_policy_cases as K
import emu_cnn_bwd as E
import test_cnn_trunk_backward_cpu as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


class DeviceBackend(E.CnnBwdHost):
    """CnnBwdHost with every array on the device: dparams and the workspace travel whole, guard words included, so a write outside them
    shows in what is read back."""

    def launch(self, rows, res, ch, layers, f4, obs, lead, ldx, mean, var, normalize, params, dout, lddo, dout_off, dp_whole, ws_whole, ws_floats):
        from emloco_amd import _lib as L
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        assert dp_whole.dtype == np.uint32 and dp_whole.size == params.size + 2 * E.GUARD and ws_whole.size == ws_floats + 2 * E.GUARD
        d_obs, d_mean, d_var, d_par, d_dout = up(obs), up(mean), up(var), up(params), up(dout)
        d_dp, d_ws = up(dp_whole.view(np.int32)), up(ws_whole.view(np.int32))
        lib = L.require_device()
        rc = lib.emloco_cnn_trunk_backward(rows, res, ch, layers, *f4, d_obs.data_ptr() + 4 * lead, ldx, d_mean.data_ptr(), d_var.data_ptr(),
                                           C.c_float(E.EPS), C.c_float(E.CLIP), normalize, d_par.data_ptr(), d_dout.data_ptr(), lddo, dout_off,
                                           d_dp.data_ptr() + 4 * E.GUARD, d_ws.data_ptr() + 4 * E.GUARD, ws_floats,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "emloco_cnn_trunk_backward")
        torch.cuda.synchronize()
        np.copyto(dp_whole, d_dp.cpu().numpy().view(np.uint32))
        np.copyto(ws_whole, d_ws.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", T.NAMES)
def test_kernel_on_device_equals_emulator(name):
    dev = T.check_case(DeviceBackend, name)                    # against float64, guards intact, the workspace's tail untouched
    emu = T.check_case(E.EmuBackend, name)                     # the same grid: the ABI's rule
    assert np.array_equal(T.bits(dev), T.bits(emu))


# ------------------------------------------------------------------ the module
_TRAINED = ("_task_actor_cnn.", "_cnn_mlp.", "actor_mlp.", "mu.")


def test_module_gradients_on_device_match_float64():
    g = K.load("cnn_policy_net_r16")
    net, rms = K.build_from(g, DEV)
    obs = torch.from_numpy(g["obs"]).to(DEV)
    with torch.no_grad():
        nobs = rms(obs)
    with pytest.raises(NotImplementedError, match="the CNN trunk's backward is not built"):
        net.eval_actor(nobs)                                    # off at construction
    assert net.enable_trunk_backward() is net
    net.eval_actor(nobs)[0].square().mean().backward()
    n64 = copy.deepcopy(net).to("cpu").double()
    n64.zero_grad()
    for p in n64.parameters():
        p.grad = None
    n64.eval_actor(nobs.cpu().double())[0].square().mean().backward()
    ref = dict(n64.named_parameters())
    seen = 0
    for k, p in net.named_parameters():
        if k.startswith(_TRAINED):
            assert p.grad is not None, k
            K.close(p.grad.cpu(), ref[k].grad, rel=3e-4, abs_=1e-6, what=f"grad {k}")
            seen += 1
        elif k.startswith("_task_critic_cnn."):
            assert p.grad is None and ref[k].grad is None, k
    assert seen == 6 + 4 + 4 + 2
    with pytest.raises(NotImplementedError, match="requires grad"):
        net._trunk(nobs[:, int(g["sizes"][0]) + int(g["traj"]):].contiguous().requires_grad_())
    net.enable_trunk_backward(False)
    with pytest.raises(NotImplementedError, match="the CNN trunk's backward is not built"):
        net.eval_actor(nobs)
    with torch.no_grad():
        assert torch.isfinite(net.eval_actor(nobs)[0]).all()   # under no_grad nothing changed


# ------------------------------------------------------------------ the agent's loss and gradients
class _FakeTask:
    """just enough of the task interface for AMPAgent's constructor and losses (no simulator): tests/test_gpu_policy.py's, with the
    crowd sensor's task observation at 16 x 16 x 3"""
    def __init__(self, E=8, dev=DEV):
        self.num_envs, self.device, self.num_actions = E, dev, 69
        self._num_amp_obs_steps = 2
        self.motion_sym_loss = True
        self.cfg = {"env": {}}
        self.left_to_right_index_action = [4, 5, 6, 7, 0, 1, 2, 3, 8, 9, 10, 11, 12, 18, 19, 20, 21, 22, 13, 14, 15, 16, 17]
        self.task = self

    def get_obs_size(self): return 1166
    def get_self_obs_size(self): return 368
    def get_num_amp_obs(self): return 412
    def get_task_obs_size_detail(self): return {"traj": 30, "heightmap_velocity": 3 * 16 * 16}
    def fetch_amp_obs_demo(self, n): return torch.randn(n, 412, device=self.device)


def _cnn_cfg():
    import yaml
    from emloco_amd.learning.amp_policy import CNN_CFG
    return yaml.safe_load(open(CNN_CFG))


def test_agent_loss_and_gradients_match_plain_torch_double_backward(monkeypatch):
    from emloco_amd.learning.amp_agent import AMPAgent, amp_dropout_mask
    from emloco_amd.learning.amp_network_sept_cnn_builder import AMPSeptCNNBuilder
    monkeypatch.setenv("EMLOCO_PPO_GRAPH", "0")
    cfg = _cnn_cfg()
    cfg["params"]["network"]["mlp"]["units"] = [96, 48]
    cfg["params"]["network"]["disc"]["units"] = [80, 40]
    cfg["params"]["config"].update(horizon_length=4, minibatch_size=16, amp_minibatch_size=16, amp_batch_size=32, amp_obs_demo_buffer_size=64,
                                   amp_replay_buffer_size=64, mini_epochs=1)
    agent = AMPAgent(_FakeTask(8), cfg)
    net = agent.a2c_network
    assert isinstance(net, AMPSeptCNNBuilder.Network) and net._trunk_backward and (net.res, net.channels) == (16, 3)
    torch.manual_seed(1)
    with torch.no_grad():
        for p in net.parameters():
            if p.requires_grad:
                p.add_(torch.randn_like(p) * 0.05)
    agent.set_eval()                                   # keep the running statistics fixed for the comparison
    B, W = 16, 1166
    d = {"obs": torch.randn(B, W, device=DEV), "flip_obs": torch.randn(B, W, device=DEV), "next_obses": torch.randn(B, W, device=DEV),
         "actions": torch.randn(B, 69, device=DEV) * 0.3, "old_logp_actions": torch.randn(B, device=DEV) * 0.1 + 30,
         "advantages": torch.randn(B, device=DEV), "old_values": torch.randn(B, 1, device=DEV), "returns": torch.randn(B, 1, device=DEV),
         "mu": torch.randn(B, 69, device=DEV) * 0.1, "sigma": torch.full((B, 69), math.exp(-2.9), device=DEV),
         "amp_obs": torch.randn(B, 412, device=DEV), "amp_obs_replay": torch.randn(B, 412, device=DEV), "amp_obs_demo": torch.randn(B, 412, device=DEV)}
    masks = amp_dropout_mask(B, 2, 206, device=DEV)
    loss, info, mu, sigma = agent.compute_loss(d, dropout_masks=masks)
    agent.bucket.zero()
    loss.backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters() if p.requires_grad}

    # ---- plain torch restatement in float64 on the CPU (F.conv2d / F.linear, autograd double backward)
    F = torch.nn.functional
    P = {k: p.detach().cpu().double().requires_grad_(p.requires_grad) for k, p in net.named_parameters()}
    d = {k: v.cpu().double() for k, v in d.items()}
    masks = masks.cpu().double()

    def mlp(x, name, n):
        for i in range(n):
            x = F.relu(F.linear(x, P[f"{name}.{2 * i}.weight"], P[f"{name}.{2 * i}.bias"]))
        return x

    def task(x):                                        # traj | map, the map (B, 16, 16, 3) channel last
        t = x[:, 30:].reshape(x.shape[0], 16, 16, 3).permute(0, 3, 1, 2)
        for i in range(3):
            t = F.relu(F.conv2d(t, P[f"_task_actor_cnn.{2 * i}.weight"], P[f"_task_actor_cnn.{2 * i}.bias"], stride=2, padding=1))
        return torch.cat([mlp(t.reshape(x.shape[0], -1), "_cnn_mlp", 2), x[:, :30]], 1)

    def actor(x):
        return F.linear(mlp(torch.cat([x[:, :368], task(x[:, 368:])], 1), "actor_mlp", 2), P["mu.weight"], P["mu.bias"])

    def critic(x):
        return F.linear(mlp(torch.cat([x[:, :368], task(x[:, 368:])], 1), "critic_mlp", 2), P["value.weight"], P["value.bias"])

    def disc(x):
        return F.linear(mlp(x, "_disc_mlp", 2), P["_disc_logits.weight"], P["_disc_logits.bias"])

    obs = d["obs"]                                      # statistics are at their initial (0, 1) values: normalisation = clamp
    eps = float(np.float32(1e-5))
    nrm = lambda x: torch.clamp(x / math.sqrt(1 + eps), -5, 5)
    mu_r = actor(nrm(obs))
    logstd = P["sigma"]
    sig = torch.exp(logstd)
    nlp = 0.5 * (((d["actions"] - mu_r) / sig) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * 69 + logstd.sum(-1) + mu_r.sum(-1) * 0
    ratio = torch.exp(d["old_logp_actions"] - nlp)
    a_loss = torch.max(-d["advantages"] * ratio, -d["advantages"] * torch.clamp(ratio, 0.8, 1.2)).mean()
    c_loss = ((d["returns"] - critic(nrm(obs))) ** 2).mean()
    b_loss = (torch.clamp_max(mu_r + 1, 0) ** 2 + torch.clamp_min(mu_r - 1, 0) ** 2).sum(-1).mean()
    demo = nrm(d["amp_obs_demo"]).requires_grad_(True)
    agent_logit = torch.cat([disc(nrm(d["amp_obs"]) * masks[..., 0]), disc(nrm(d["amp_obs_replay"]) * masks[..., 1])], 0)
    demo_logit = disc(demo * masks[..., 2])
    bce = torch.nn.BCEWithLogitsLoss()
    dl = 0.5 * (bce(agent_logit, torch.zeros_like(agent_logit)) + bce(demo_logit, torch.ones_like(demo_logit)))
    dl = dl + 0.01 * (P["_disc_logits.weight"] ** 2).sum()
    (gx,) = torch.autograd.grad(demo_logit, demo, grad_outputs=torch.ones_like(demo_logit), create_graph=True, retain_graph=True)
    dl = dl + 5 * gx.pow(2).sum(-1).mean()
    dl = dl + 0.0001 * sum((P[k] ** 2).sum() for k in ("_disc_mlp.0.weight", "_disc_mlp.2.weight", "_disc_logits.weight"))
    flip_a = actor(nrm(d["flip_obs"]))
    orig_a = (actor(nrm(d["next_obses"])).view(B, -1, 3) * torch.tensor([-1.0, 1.0, -1.0], dtype=torch.float64))[:, agent.task.left_to_right_index_action]
    s_loss = ((orig_a.reshape(B, -1) - flip_a) ** 2).mean(-1).mean() * 50
    ref = a_loss + 5 * c_loss + 10 * b_loss + 5 * dl + s_loss
    ref.backward()
    print(f"loss {loss.item():.7e}, plain torch {ref.item():.7e}")
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item()), (loss.item(), ref.item())
    assert any(k.startswith("_task_actor_cnn.") for k in got) and any(k.startswith("_task_critic_cnn.") for k in got)
    for k, gk in got.items():
        if k.startswith("_task_critic_cnn."):           # built for the checkpoints' sake, never evaluated: its slice of the bucket stays zero
            assert P[k].grad is None and (gk == 0).all(), k
        else:
            K.close(gk.cpu(), P[k].grad, rel=3e-4, abs_=1e-6, what=f"grad {k}")


# ------------------------------------------------------------------ end to end, the captured optimiser step
def _seed(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


def _make_crowd_env(num_envs):
    import emloco_amd
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", "--small_terrain", "--cfg_env", cfg_env])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(dict(num_env_group=16))
    return create_rlgpu_env(args, cfg, cfg_train)


def test_two_training_epochs_on_a_crowd_task_and_the_checkpoint_plays(tmp_path):
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.run import RLGPUEnv
    _seed(3)
    raw = _make_crowd_env(64)
    cfg = _cnn_cfg()
    cfg["params"]["network"]["mlp"]["units"] = [256, 128]
    cfg["params"]["network"]["disc"]["units"] = [128, 64]
    cfg["params"]["config"].update(horizon_length=8, minibatch_size=128, amp_minibatch_size=128, amp_batch_size=64,
                                   amp_obs_demo_buffer_size=512, amp_replay_buffer_size=512, mini_epochs=2)
    agent = AMPAgent(RLGPUEnv(raw), cfg)
    net = agent.a2c_network
    assert agent.use_graph and (net.res, net.channels) == (64, 3) and net._trunk_backward
    names = ("_task_actor_cnn.0.weight", "_cnn_mlp.0.weight", "mu.weight", "_task_critic_cnn.0.weight")
    before = {k: net.state_dict()[k].detach().clone() for k in names}
    for _ in range(2):
        info = agent.train_epoch()
    assert all(np.isfinite(v) for k, v in info.items() if isinstance(v, float)), info
    after = net.state_dict()
    for k in names[:3]:
        assert not torch.equal(before[k], after[k]), k
    assert torch.equal(before[names[3]], after[names[3]])
    assert all(torch.isfinite(p).all() for p in net.parameters())
    # the file this writes is the file --test plays
    path = str(tmp_path / "cnn_policy")
    agent.save(path)
    _seed(22)                                                      # another initialisation: the checkpoint decides
    bundle = AMPPolicyBundle(raw.task, cfg_train=cfg, checkpoint=path + ".pth", deterministic=True)       # (load_state_dict(strict=True) inside)
    assert list(bundle.a2c_network.state_dict()) == list(net.state_dict())
    obs = raw.task.obs_buf.detach().clone()
    assert torch.isfinite(obs).all()
    agent.set_eval()
    with torch.no_grad():
        mu = net.eval_actor(agent.running_mean_std(obs))[0]
    K.close(bundle.policy(obs).cpu(), mu.clamp(-1.0, 1.0).cpu(), what="the bundle's policy against the agent's own network")

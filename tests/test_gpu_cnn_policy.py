"""GPU: the CNN policy of the crowd sensor.  The trunk kernel (emloco_cnn_trunk) bit for bit against its CPU emulation on the cases of
tests/test_cnn_trunk_cpu.py; the network module on the device and the frozen runner against the reference's fixtures
(tests/golden/gen_golden_cnn_policy.py) and, at the shipped shape, against a float64 evaluation of the same weights; the policy bundle
on a crowd task and on the default task; a LocoVal rollout with the CNN policy acting.  Bars: `close` of tests/cnn_policy_cases.py
(1e-4 of the tensor's max + 1e-5, the bar of tests/test_gpu_policy.py for this network family)."""
import copy
import ctypes as C
import os
import random

import numpy as np
import pytest

import cnn_policy_cases as K
import emu_cnn
import test_cnn_trunk_cpu as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


class DeviceBackend(emu_cnn.CnnHost):
    """CnnHost with every array on the device: the guarded output travels whole, so a write outside it shows in the guard words read back."""

    def launch(self, rows, res, ch, layers, f4, obs, lead, ldx, mean, var, normalize, params, out, ldo, out_off):
        from emloco_amd import _lib as L
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        whole = out.base if out.base is not None else out
        while whole.base is not None:
            whole = whole.base
        assert whole.dtype == np.uint32 and whole.size == rows * ldo + 2 * emu_cnn.GUARD
        d_obs, d_mean, d_var, d_par, d_whole = up(obs), up(mean), up(var), up(params), up(whole.view(np.int32))
        lib = L.require_device()
        rc = lib.emloco_cnn_trunk(rows, res, ch, layers, *f4, d_obs.data_ptr() + 4 * lead, ldx, d_mean.data_ptr(), d_var.data_ptr(),
                                  C.c_float(emu_cnn.EPS), C.c_float(emu_cnn.CLIP), normalize, d_par.data_ptr(),
                                  d_whole.data_ptr() + 4 * emu_cnn.GUARD, ldo, out_off, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "emloco_cnn_trunk")
        torch.cuda.synchronize()
        np.copyto(whole, d_whole.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", T.NAMES)
def test_kernel_on_device_equals_emulator(name):
    dev = T.check_case(DeviceBackend, name)                    # against float64, columns around the features and guards untouched
    emu = T.check_case(emu_cnn.EmuBackend, name)
    assert np.array_equal(dev.view(np.uint32), emu.view(np.uint32))


def test_kernel_normalisation_off_on_device():
    c, _, _ = T.reference("r16c3")
    width = c["ch"] * c["res"] ** 2
    pre = c["obs"].copy()
    y = (pre[:, c["lead"]:c["lead"] + width] - c["mean"]) / np.sqrt(c["var"] + np.float32(emu_cnn.EPS))
    pre[:, c["lead"]:c["lead"] + width] = np.minimum(np.maximum(y, np.float32(-emu_cnn.CLIP)), np.float32(emu_cnn.CLIP))
    b = DeviceBackend(c)
    on, off = b.run(), b.run(normalize=False, obs=pre)
    assert on[1] and on[2] and off[1] and off[2] and np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))


# ------------------------------------------------------------------ the module and the frozen runner against the reference's fixtures
@pytest.mark.parametrize("name", K.FIXTURES)
def test_module_and_runner_match_the_reference_fixture(name):
    from emloco_amd.learning.policy_runner import CnnFrozenPolicy
    g = K.load(name)
    net, rms = K.build_from(g, DEV)
    assert list(net.state_dict()) == [str(k) for k in g["keys"]]
    obs = torch.from_numpy(g["obs"]).to(DEV)
    with torch.no_grad():
        nobs = rms(obs)
        K.close(nobs.cpu(), g["norm_obs"], rel=2e-6, abs_=2e-6, what="normalised obs")
        K.close(net.eval_task(nobs[:, int(g["sizes"][0]):]).cpu(), g["task_out"], what="task embedding")
        mu, sigma = net.eval_actor(nobs)
        K.close(mu.cpu(), g["mu"], what="mu")
        assert np.array_equal(sigma.cpu().numpy(), g["sigma"])
        K.close(net.eval_critic(nobs).cpu(), g["value"], what="value")
        K.close(net.eval_disc(torch.from_numpy(g["amp_obs"]).to(DEV)).cpu(), g["disc_logits"], what="disc logits")
        out = net({"obs": nobs})
        assert len(out) == 4 and out[3] is None
    with pytest.raises(NotImplementedError, match="the CNN trunk's backward is not built"):
        net.eval_actor(nobs)                                    # grad enabled, device tensor
    fp = CnnFrozenPolicy(net, rms, obs.shape[0], DEV)
    K.close(fp.act_mean(obs).cpu(), g["mu"], what="frozen mu")
    assert (fp.actor_in[:, fp.actor_in_size:] == 0).all()


def _float64_mu(net, rms, obs):
    """eval_actor(running_mean_std(obs)) in float64 on the CPU with the module's own weights"""
    n64 = copy.deepcopy(net).to("cpu").double()
    x = obs.detach().cpu().double()
    x = ((x - rms.running_mean.cpu()) / torch.sqrt(rms.running_var.cpu() + float(np.float32(rms.epsilon)))).clamp(-5.0, 5.0)
    with torch.no_grad():
        return n64.eval_actor(x)[0]


def test_runner_at_the_shipped_shape():
    from emloco_amd.learning.policy_runner import CnnFrozenPolicy
    E, traj, map_size = 8, 30, 3 * 64 * 64
    torch.manual_seed(11)
    net, rms = K.build(DEV, K.params(), 368, traj, "heightmap_velocity", map_size)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bias"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(DEV))
        rms.running_mean.copy_(torch.randn(rms.running_mean.shape, generator=g, dtype=torch.float64) * 0.3)
        rms.running_var.copy_(torch.rand(rms.running_var.shape, generator=g, dtype=torch.float64) * 2.0 + 0.05)
    obs = (torch.randn(E, 368 + traj + map_size, generator=g) * 1.5)
    obs[0, :4], obs[1, 370:375], obs[2, 500:520], obs[E - 1, -5:] = 40.0, -40.0, 40.0, -40.0
    obs = obs.to(DEV)
    fp = CnnFrozenPolicy(net, rms, E, DEV)
    assert fp.actor_in.shape == (E, 656) and fp.actor_in_size == 654 and fp.cnn_feat.shape == (E, 1024)
    assert fp.flops_per_env == 2 * (2_097_152 + 1024 * 512 + 512 * 256 + 656 * 2048 + 2048 * 1024 + 1024 * 69)
    ref = _float64_mu(net, rms, obs)
    mu = fp.act_mean(obs)
    K.close(mu.cpu(), ref, what="frozen mu, 64 x 64 x 3")
    with torch.no_grad():
        K.close(net.eval_actor(rms(obs))[0].cpu(), ref, what="module mu, 64 x 64 x 3")
    det = fp.act(obs, deterministic=True).clone()
    gen = torch.Generator(device=DEV).manual_seed(5)
    sto = fp.act(obs, deterministic=False, generator=gen)
    assert sto.abs().max() <= 1.0 and det.abs().max() <= 1.0 and not torch.equal(sto, det)
    fp.mu_b[::2] += 3.0                                         # push half of the means past the clamp
    fp.mu_b[1::2] -= 3.0
    det = fp.act(obs, deterministic=True)
    assert det.abs().max() <= 1.0 and (det == 1.0).any() and (det == -1.0).any()


# ------------------------------------------------------------------ the bundle on tasks
def _seed(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


def _make_env(num_envs, env_cfg, cfg_env=None, small=True):
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    argv = ["--num_envs", str(num_envs), "--seed", "3"] + (["--small_terrain"] if small else []) + ([] if cfg_env is None else ["--cfg_env", cfg_env])
    args = get_args(argv)
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(env_cfg)
    return create_rlgpu_env(args, cfg, cfg_train)


def _cnn_cfg():
    import yaml
    from emloco_amd.learning.amp_policy import CNN_CFG
    return yaml.safe_load(open(CNN_CFG))


def _bundle_checks(env, E, tmp_path):
    """the CNN bundle on a task: classes, policy against the module path, a strict checkpoint round trip, four steps"""
    from emloco_amd.learning.amp_network_sept_cnn_builder import AMPSeptCNNBuilder
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.policy_runner import CnnFrozenPolicy
    t = env.task
    _seed(21)
    bundle = AMPPolicyBundle(t, cfg_train=_cnn_cfg(), deterministic=True)
    assert isinstance(bundle.a2c_network, AMPSeptCNNBuilder.Network) and type(bundle.frozen) is CnnFrozenPolicy
    env.reset(torch.arange(E, device=t.device))
    obs, _, _, _ = env.step(torch.zeros(E, 69, device=t.device))
    act = bundle.policy(obs).clone()
    with torch.no_grad():
        mu = bundle.a2c_network.eval_actor(bundle.running_mean_std(obs))[0]
    K.close(act.cpu(), mu.clamp(-1.0, 1.0).cpu(), what="policy(obs) against the module path")
    assert torch.isfinite(bundle.eval_critic(obs)).all()
    path = str(tmp_path / "policy.pth")
    torch.save({"model": {"a2c_network." + k: v.cpu() for k, v in bundle.a2c_network.state_dict().items()},
                "running_mean_std": bundle.running_mean_std.state_dict(), "amp_input_mean_std": bundle.amp_input_mean_std.state_dict()}, path)
    _seed(22)                                                      # another initialisation: the checkpoint decides
    again = AMPPolicyBundle(t, cfg_train=_cnn_cfg(), checkpoint=path, deterministic=True)         # (load_state_dict(strict=True) inside)
    assert torch.equal(again.policy(obs), act)
    for _ in range(4):
        a = bundle.policy(obs)
        obs, _, _, _ = env.step(a)
        assert torch.isfinite(obs).all() and torch.isfinite(a).all()
    return bundle


@pytest.fixture(scope="module")
def crowd_env():
    import emloco_amd
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    _seed(3)
    return _make_env(64, dict(num_env_group=16), cfg_env=cfg_env)


def test_bundle_on_a_crowd_task(crowd_env, tmp_path):
    b = _bundle_checks(crowd_env, 64, tmp_path)
    assert (b.frozen.res, b.frozen.channels, b.frozen.actor_in_size) == (64, 3, 654)


def test_bundle_on_the_default_task(tmp_path):
    _seed(3)
    b = _bundle_checks(_make_env(16, {}), 16, tmp_path)
    assert (b.frozen.res, b.frozen.channels, b.frozen.cnn_layers) == (32, 1, [])          # the reference's `heightmap` branch: no _cnn_mlp


def test_locoval_rollout_with_the_cnn_policy(crowd_env):
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    from emloco_amd.run import RLGPUEnv
    _seed(31)
    bundle = AMPPolicyBundle(crowd_env.task, cfg_train=_cnn_cfg())
    agent = LocoValRollout(RLGPUEnv(crowd_env), horizon_length=2, policy=bundle.policy, disc_reward=bundle.disc_reward,
                           inversion_penalty_scale=float(bundle.config.get("inversion_penalty_scale", 0.3)))
    loss = agent.play_steps()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and torch.isfinite(crowd_env.task.obs_buf).all()

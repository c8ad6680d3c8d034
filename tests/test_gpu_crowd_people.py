"""GPU: the group observation on the device -- every case of tests/test_crowd_people_cpu.py through emloco_task_crowd_people, bit-equal
to the emulator's output; the task with group_obs beside a twin without; the sept network's people branch and its frozen runner
against float64; run.py on pacer_group_obs.yaml as subprocesses (noise actions, frozen policy, --test, --train_policy)."""
import copy
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import emu_crowd_people as EP  # noqa: E402
import test_crowd_people_cpu as T  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DeviceBackend(EP.PeopleHost):
    """PeopleHost with every array on the device: the guarded arrays travel whole, so a write outside a buffer shows in the guard
    words read back."""

    def sync_in(self):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self._dev = {k: up(a) for k, a in self.inputs.items()}
        for k, w in self.whole.items():
            self._dev[k] = up(w.view(np.int32))

    def sync_out(self):
        torch.cuda.synchronize()
        for k, w in self.whole.items():
            np.copyto(w, self._dev[k].cpu().numpy().view(np.uint32))

    def ptr(self, name):
        return self._dev[name].data_ptr() + (4 * EP.GUARD if name in self.whole else 0)

    def _call(self, s, ids, n):
        from emloco_amd import _lib as L
        lib = L.require_device()
        L.check(lib.emloco_task_crowd_people(C.byref(s), ids, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emloco_task_crowd_people")


def _cases():
    g = EP.golden()
    out = [("fixture_" + n, g[n + "_rb"], int(g[n + "_group_size"]), None) for n in g["cases"]]
    out += [(n, *EP.CASES[n](), None) for n in sorted(EP.CASES)]
    rb, gs = EP.CASES["nan_root"]()
    return out + [("id_list", rb, gs, EP.ID_LIST)]


@pytest.mark.parametrize("name,rb,gs,ids", _cases(), ids=[c[0] for c in _cases()])
def test_device_equals_emulator(name, rb, gs, ids):
    dev, again, emu = (B(len(rb), gs).run(rb, ids) for B in (DeviceBackend, DeviceBackend, EP.EmuBackend))
    assert dev.written_bytes() == emu.written_bytes(), "the device and the emulator give the same bytes"
    assert dev.written_bytes() == again.written_bytes(), "two device runs give the same bytes"
    assert dev.guards() and again.guards()
    if ids is None:
        T.check_case(dev, rb, gs)


def test_device_refusals_reach_the_caller():
    from emloco_amd import _lib as L
    lib = L.require_device()
    h = DeviceBackend(12, 6)
    h.sync_in()
    s = h.struct()
    s.group_size = 4
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.emloco_task_crowd_people(C.byref(s), None, 0, st) == -1
    with pytest.raises(L.EmlocoError, match="emloco_task_crowd_people.*group_size < 6"):
        L.check(lib.emloco_task_crowd_people(C.byref(s), None, 0, st), "emloco_task_crowd_people")
    with pytest.raises(L.EmlocoError, match="null structure"):
        L.check(lib.emloco_task_crowd_people(None, None, 0, st), "emloco_task_crowd_people")
    h.sync_out()
    assert h.guards() and h.written_bytes() == EP.EmuBackend(12, 6).written_bytes()          # nothing was written


# ------------------------------------------------------------------ the task
def _seed(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


def _make_env(num_envs, env_cfg):
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", "--small_terrain"])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(env_cfg)
    return create_rlgpu_env(args, cfg, cfg_train)


def _block_check(t, gs):
    E = t.num_envs
    rb = t._rigid_body_state.view(E, 24, 13).cpu().numpy()
    rows, flip, _ = EP.people_f64(rb, gs)
    got, gotf = t.obs_buf[:, -165:].cpu().numpy(), t._flip_obs_buf[:, -165:].cpu().numpy()
    err = max(np.abs(got - rows).max(), np.abs(gotf - flip).max())
    assert err <= EP.BAR, err
    return got


def test_task_with_group_obs_beside_a_twin_without():
    """16 envs in groups of 8: a reset and three steps.  This test fails on the parent commit, where the constructor raises
    NotImplementedError for group_obs: True."""
    from emloco_amd import _lib as L
    E, gs = 16, 8
    front = L.SELF_OBS + 2 * L.TRAJ_SAMPLES + 1024
    keys = ("_rigid_body_state", "rew_buf", "reset_buf", "obs_buf", "_flip_obs_buf")
    tasks = []
    for env_cfg in (dict(divide_group=True, num_env_group=gs, group_obs=True), dict(divide_group=True, num_env_group=gs, disable_group_obs=True)):
        _seed(3)
        env = _make_env(E, env_cfg)
        t = env.task
        tasks.append(t)
        _seed(100)
        env.reset(torch.arange(E, device=t.device))
        t._snap = [{k: getattr(t, k).clone() for k in keys}]
        if t is tasks[0]:
            seen = [_block_check(t, gs)]
        for k in range(3):
            _seed(200 + k)
            env.step(torch.zeros(E, 69, device=t.device))
            t._snap.append({k: getattr(t, k).clone() for k in keys})
            if t is tasks[0]:
                seen.append(_block_check(t, gs))
    torch.cuda.synchronize()
    a, b = tasks
    assert a._crowd_mode and b._crowd_mode and a._group_obs and not b._group_obs and not a._crowd.stamps and not b._crowd.stamps
    assert a.num_obs == front + 165 and b.num_obs == front and a.obs_buf.shape == a._flip_obs_buf.shape == (E, front + 165)
    assert a.get_task_obs_size() == 30 + 1024 + 165
    assert list(a.get_task_obs_size_detail().items()) == [("traj", 30), ("heightmap", 1024), ("people", 165)]
    assert list(b.get_task_obs_size_detail().items()) == [("traj", 30), ("heightmap", 1024)]
    for sa, sb in zip(a._snap, b._snap):
        for k in ("_rigid_body_state", "rew_buf", "reset_buf"):
            assert torch.equal(sa[k], sb[k]), k
        for k in ("obs_buf", "_flip_obs_buf"):
            assert torch.equal(sa[k][:, :front], sb[k]), k
    assert all(np.abs(s).max() > 0.1 for s in seen) and not np.array_equal(seen[0], seen[-1])       # somebody is within 10 m, and moves
    flipped = a._flip_obs_buf[:, -165:].view(E, 55, 3)
    normal = a.obs_buf[:, -165:].view(E, 55, 3)
    assert torch.equal(flipped[..., 0], normal[..., 0]) and torch.equal(flipped[..., 1], -normal[..., 1]) and torch.equal(flipped[..., 2], normal[..., 2])
    # a reset of two envs rewrites those two rows only
    before, before_f = a.obs_buf.clone(), a._flip_obs_buf.clone()
    _seed(300)
    a.reset(torch.tensor([1, 14], device=a.device))
    torch.cuda.synchronize()
    rest = [e for e in range(E) if e not in (1, 14)]
    assert torch.equal(a.obs_buf[rest], before[rest]) and torch.equal(a._flip_obs_buf[rest], before_f[rest])
    assert not torch.equal(a.obs_buf[[1, 14], -165:], before[[1, 14], -165:])
    rb = a._rigid_body_state.view(E, 24, 13).cpu().numpy()
    rows, _, _ = EP.people_f64(rb, gs)
    assert np.abs(a.obs_buf[[1, 14], -165:].cpu().numpy() - rows[[1, 14]]).max() <= EP.BAR


def test_task_refusals():
    with pytest.raises(NotImplementedError, match="group_obs.*at least 6"):
        _make_env(10, dict(divide_group=True, num_env_group=5, group_obs=True))


# ------------------------------------------------------------------ the network
def _device_network(seed=3):
    net, rms = T._network(seed=seed)
    with torch.no_grad():
        for m in list(net._point_net) + list(net._task_mlp):
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    return net, rms


def _err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


@pytest.mark.parametrize("rows", [1, 16, 17])
def test_network_on_device_against_float64(rows):
    """Forward and the gradients of every parameter on the path (`_point_net`, `_task_mlp`, both trunks, both heads) at 1, 16 and 17
    rows -- the point-net sees 5, 80 and 85 rows: a single partial tile, the workload's shape, a ragged tail -- the device module
    against its own evaluation in float64 on the CPU.  The people columns carry the workload's edges (tests/people_training_cases.py:
    rows whose five neighbours are all zeros, one with a single neighbour, one the normalisation clamps, the rest in metres); over
    those columns the moments repeat per neighbour, so that the all-zero rows tie exactly in every arithmetic.  The bar is five times
    what stock torch fp32 (the same module on the CPU) shows against float64 on the same inputs, per quantity; the test prints both.
    Measured on one MI355X at 16 rows before the rows and the parameter list were widened: mu 2.6e-7 (stock 1.7e-7), value 1.1e-7
    (1.1e-7), the six `_point_net` gradients 3.5e-8 .. 1.6e-7 (stock 2.4e-8 .. 1.0e-7).  With the process-wide two-piece gradient
    GEMMs `_point_net.0.weight` came out 2.0e-6 off, 29 times stock: the people network therefore evaluates under
    ops.backward_pieces_for(3).  Widened, on one MI355X: every quantity at every row count within 2.0 times stock (value.weight at 16
    rows 3.2e-6 / 1.6e-6), most below stock; the bias gradients that are exact in float32 (value.bias; mu.bias at one row) are exact on
    the device."""
    import people_training_cases as PC
    net, rms = _device_network()
    with torch.no_grad():
        rms.running_mean.copy_(PC.tile_people(rms.running_mean))
        rms.running_var.copy_(PC.tile_people(rms.running_var))
    g = torch.Generator().manual_seed(7)
    raw = PC.people_edges(torch.randn(rows, T.SELF + T.TRAJ + T.MAP + T.PEOPLE, generator=g) * 2, g)
    obs = rms(raw)
    w = torch.randn(rows, T.ACTIONS, generator=g)
    names = [n for n, q in net.named_parameters() if q.requires_grad and not n.startswith("_disc_")]
    assert {n.split(".")[0] for n in names} == {"_point_net", "_task_mlp", "actor_mlp", "critic_mlp", "mu", "value"}

    def evaluate(module, mean_std, x, wt):
        module.running_mean, module.running_var = mean_std.running_mean, mean_std.running_var
        mu, _ = module.eval_actor(x)
        value = module.eval_critic(x)
        p = dict(module.named_parameters())
        grads = torch.autograd.grad((mu * wt).sum() + value.sum(), [p[n] for n in names])
        return [mu, value] + list(grads)

    n64, r64 = copy.deepcopy(net).double(), copy.deepcopy(rms).double()
    ref = evaluate(n64, r64, obs.double(), w.double())
    cpu32 = evaluate(copy.deepcopy(net), copy.deepcopy(rms), obs, w)
    ndev, rdev = copy.deepcopy(net).to(DEV), copy.deepcopy(rms).to(DEV)
    dev = evaluate(ndev, rdev, obs.to(DEV), w.to(DEV))
    missed = []
    for what, r, c, d in zip(["mu", "value"] + names, ref, cpu32, dev):
        stock, got = _err(c, r), _err(d, r)
        print(f"{what}: stock torch fp32 against float64 {stock:.3e}, device {got:.3e}, bar {5 * stock:.3e}")
        if not got <= 5 * stock:
            missed.append((what, stock, got))
    assert not missed, missed


def test_frozen_runner_against_the_module():
    """PeopleFrozenPolicy.act_mean against eval_actor(running_mean_std(obs)) of the module, at the bar of tests/test_gpu_policy.py's
    frozen-policy test (1e-5 + 1e-4 of the largest value); rows with values the normalisation clamps.  Measured: 3.0e-7, bar 5.9e-5."""
    from emloco_amd.learning.policy_runner import PeopleFrozenPolicy
    net, rms = _device_network(seed=4)
    net, rms = net.to(DEV), rms.to(DEV)
    net.running_mean, net.running_var = rms.running_mean, rms.running_var
    E = 16
    torch.manual_seed(8)
    obs = torch.randn(E, T.SELF + T.TRAJ + T.MAP + T.PEOPLE) * 2
    obs[0, -165:-150], obs[1, -5:], obs[2, 500:520] = 40.0, -40.0, 40.0
    obs = obs.to(DEV)
    fp = PeopleFrozenPolicy(net, rms, E, DEV)
    assert fp.actor_in.shape == (E, 368 + 256 + 64) and fp.task_in.shape == (E, 1220) and fp.point_in.shape == (5 * E, 36)
    assert fp.flops_per_env == 2 * (1220 * 512 + 512 * 256 + 688 * 2048 + 2048 * 1024 + 1024 * 69 + 5 * (36 * 32 + 32 * 64 + 64 * 64))
    mu = fp.act_mean(obs)
    with torch.no_grad():
        ref = net.eval_actor(rms(obs))[0]
    tol = 1e-5 + 1e-4 * float(ref.abs().max())
    print(f"frozen mu against the module: {_err(mu, ref):.3e}, bar {tol:.3e}")
    assert _err(mu, ref) <= tol
    assert (fp.point_in[:, 33:] == 0).all() and (fp.task_in[:, 1219:] == 0).all()
    a = fp.act(obs, deterministic=True)
    assert float(a.abs().max()) <= 1.0


# ------------------------------------------------------------------ the entry point
def _cfg_env(tmp_path):
    """pacer_group_obs.yaml with num_env_group 8"""
    import yaml
    import emloco_amd
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group_obs.yaml")))
    cfg["env"]["num_env_group"] = 8
    path = str(tmp_path / "pacer_group_obs_8.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    return path


def _run(tmp_path, *extra):
    cmd = [sys.executable, "-m", "emloco_amd.run", "--cfg_env", _cfg_env(tmp_path), "--num_envs", "16", "--seed", "3", "--small_terrain",
           "--input_init_pose", "--input_init_vel", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("mode", ["noise", "frozen"])
def test_run_locoval_loop_as_a_subprocess(tmp_path, mode):
    out = _run(tmp_path, "--experiment", "e", "--network_path", str(tmp_path), "--max_iterations", "2", "--save_freq", "1",
               *(["--policy_random_init"] if mode == "frozen" else []))
    assert len([ln for ln in out.splitlines() if ln.startswith("Ep: ")]) == 2
    log = [json.loads(ln) for ln in open(tmp_path / "e_log.jsonl")]
    assert [r["epoch"] for r in log] == [1, 2] and os.path.exists(tmp_path / "e_valuenet.pth")


def test_run_test_as_a_subprocess(tmp_path):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    _seed(5)
    vnet = str(tmp_path / "locoval.pth")
    torch.save(ValuePoseNet(use_pose=True, use_vel=True).state_dict(), vnet)
    rep = str(tmp_path / "report.json")
    _run(tmp_path, "--test", "--policy_random_init", "--valuenet_path", vnet, "--games_num", "16", "--max_steps", "200", "--eval_out", rep)
    assert json.load(open(rep))["games"] > 0


def test_run_train_policy_as_a_subprocess(tmp_path):
    out = _run(tmp_path, "--train_policy", "--experiment", "p", "--network_path", str(tmp_path), "--max_iterations", "2", "--save_freq", "1")
    assert len([ln for ln in out.splitlines() if ln.startswith("Ep: ")]) == 2
    log = [json.loads(ln) for ln in open(tmp_path / "p_log.jsonl")]
    assert [r["epoch"] for r in log] == [1, 2]
    saved = [f for f in os.listdir(tmp_path) if f.startswith("p") and f.endswith(".pth")]
    assert saved
    sd = torch.load(tmp_path / sorted(saved)[0], map_location="cpu")
    assert any(k.endswith("_point_net.4.weight") for k in sd["model"])

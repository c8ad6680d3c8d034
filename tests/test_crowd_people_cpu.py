"""CPU-only: the group observation (include/emloco_task.h: EmlocoCrowdPeople) -- its kernels on the emulator against the reference's
fixture and a float64 restatement, the entry point's refusals, and the host logic around it: the task's sizes, the entry point's
refusal table, the point-net branch of the sept network."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import emu_crowd_people as EP
from emloco_amd import _abi, _lib as L


@pytest.fixture(scope="module")
def golden():
    return EP.golden()


def emu_run(rb, gs, env_ids=None, **kw):
    h = EP.EmuBackend(len(rb), gs)
    return h.run(rb, env_ids, **kw)


def check_case(h, rb, gs, bar=EP.BAR):
    """rows, mirrored rows and neighbours of a finished host against the float64 restatement; guards and the bytes around the block"""
    rows, flip, nbs = EP.people_f64(rb, gs)
    assert np.array_equal(h.neighbours(), nbs)
    assert np.abs(h.block("obs") - rows).max() <= bar and np.abs(h.block("flip_obs") - flip).max() <= bar
    masked = rows.reshape(len(rb), 55, 3)
    assert np.array_equal(h.block("obs").reshape(len(rb), 55, 3)[(masked == 0).all(-1)], masked[(masked == 0).all(-1)])     # zeros are exact
    fresh = EP.EmuBackend(h.E, h.gs)
    for name in ("obs", "flip_obs"):
        keep = np.ones(h.stride, bool)
        keep[h.col:h.col + EP.WIDTH] = False
        assert np.array_equal(h.rows(name)[:, keep], fresh.rows(name)[:, keep])
    assert h.guards()


def test_fixture_meets_its_conditions(golden):
    """what tests/golden/gen_golden_crowd_people.py asserts when it draws, again on the committed file"""
    assert list(golden["cases"]) == ["a", "b"]
    for name, n_env, gs in (("a", 16, 8), ("b", 12, 6)):
        rb = golden[name + "_rb"]
        assert rb.shape == (n_env, 24, 13) and int(golden[name + "_group_size"]) == gs and golden[name + "_rows"].shape == (n_env, 165)
        root = rb[:, 0, :3].astype(np.float64)
        d = np.array([[np.linalg.norm(root[m] - root[e]) for m in range((e // gs) * gs, (e // gs + 1) * gs) if m != e] for e in range(n_env)])
        s = np.sort(d, axis=1)
        assert np.diff(s, axis=1).min() >= 1e-4 and np.abs(d - 10.0).min() >= 1e-3
        masked = (s[:, :5] > 10).sum(1)
        if name == "a":
            other = np.array([min(np.linalg.norm(root[m] - root[e]) for m in range(n_env) if m // gs != e // gs) for e in range(n_env)])
            assert masked[5] == 5 and (other < s[:, 4]).any()
        else:
            assert [masked[e] for e in (6, 8, 9, 11)] == [2, 2, 2, 2]
        tilt = 2 * np.arcsin(np.linalg.norm(rb[:, 0, 3:5].astype(np.float64), axis=1))
        assert tilt.max() > 0.05 and tilt.max() <= 0.2 + 1e-6              # the heading is not the whole rotation


def test_emulator_against_the_reference_fixture(golden):
    """Both rows of both cases against the reference's own output.  The reference's fp32 rows differ from the float64 restatement
    (emu_crowd_people.people_f64) by at most 1.3099935e-06 on the committed fixture (re-measured here); the bar is four times that,
    5.239974e-06: the kernel may sum the rotation in another order than torch, and each reordering costs about an ulp of a 10 m value,
    9.5e-7."""
    worst_ref, worst = 0.0, 0.0
    for name in golden["cases"]:
        rb, gs = golden[name + "_rb"], int(golden[name + "_group_size"])
        rows, flip, nbs = EP.people_f64(rb, gs)
        worst_ref = max(worst_ref, np.abs(golden[name + "_rows"] - rows).max(), np.abs(golden[name + "_flip"] - flip).max())
        h = emu_run(rb, gs)
        worst = max(worst, np.abs(h.block("obs") - golden[name + "_rows"]).max(), np.abs(h.block("flip_obs") - golden[name + "_flip"]).max())
        assert np.array_equal(h.block("obs") == 0, golden[name + "_rows"] == 0)           # the same neighbours are masked
    print(f"reference fp32 against float64: {worst_ref:.7e}; emulator against the reference: {worst:.7e}; bar {EP.BAR:.7e}")
    assert worst_ref == pytest.approx(EP.REF_ERR, rel=1e-6)
    assert worst <= EP.BAR


@pytest.mark.parametrize("name", ["a", "b"])
def test_neighbours_equal_the_float64_restatement_on_the_fixture(golden, name):
    rb, gs = golden[name + "_rb"], int(golden[name + "_group_size"])
    check_case(emu_run(rb, gs), rb, gs)


@pytest.mark.parametrize("name", sorted(EP.CASES))
def test_shapes_the_fixture_cannot_reach(name):
    rb, gs = EP.CASES[name]()
    h = emu_run(rb, gs)
    check_case(h, rb, gs)
    nbs = h.neighbours()
    if name == "all_equal":
        for e in range(len(rb)):
            g0 = (e // gs) * gs
            assert nbs[e].tolist() == [m for m in range(g0, g0 + gs) if m != e][:5]
    if name == "nan_root":
        assert all(3 not in nbs[e] for e in range(6, 18))
        for e in (0, 1, 2, 4, 5):                                 # five others exist, the NaN member is the last of them and masked
            assert nbs[e][4] == 3 and not h.block("obs")[e, 120:150].any() and not h.block("obs")[e, 162:165].any()
            assert h.block("obs")[e, :120].all()
        assert not h.block("obs")[3].any()                        # its own distances are all non-finite: everybody masked
    assert emu_run(rb, gs, grid=1).written_bytes() == h.written_bytes()                  # the grid does not matter


def test_id_list_rewrites_its_rows_only():
    rb, gs = EP.CASES["nan_root"]()
    rb[3, 0, 0] = 21.0
    full = emu_run(rb, gs)
    h = emu_run(rb, gs, EP.ID_LIST)
    fresh = EP.EmuBackend(len(rb), gs)
    listed = [e for e in EP.ID_LIST if e >= 0]
    for name in ("obs", "flip_obs"):
        want = fresh.rows(name)
        want[listed] = full.rows(name)[listed]
        assert np.array_equal(h.rows(name), want)
    want_nb = fresh.neighbours()
    want_nb[listed] = full.neighbours()[listed]
    assert np.array_equal(h.neighbours(), want_nb) and h.guards()
    none = emu_run(rb, gs, [])
    assert none.written_bytes() == fresh.written_bytes()


def test_without_a_neighbour_table():
    rb, gs = EP.CASES["all_equal"]()
    h = EP.EmuBackend(len(rb), gs, neighbours=False).run(rb)
    assert (h.neighbours() == -1).all() and h.block("obs").tobytes() == emu_run(rb, gs).block("obs").tobytes()


def test_refusals_by_name():
    h = EP.EmuBackend(12, 6)
    ok = h.struct()
    assert EP.emu_refusal(ok) == ""

    def changed(**kw):
        s = h.struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    assert EP.emu_refusal(None) == "null structure"
    for field in ("rb_state", "roots_ws", "obs", "flip_obs"):
        assert EP.emu_refusal(changed(**{field: None})) == "null " + field
    assert EP.emu_refusal(changed(group_size=4, n_env=12)) == "group_size < 6"
    assert EP.emu_refusal(changed(group_size=5, n_env=10)) == "group_size < 6"
    assert EP.emu_refusal(changed(n_env=13)) == "n_env is not a multiple of group_size"
    assert EP.emu_refusal(changed(n_env=0)) == "n_env is not a multiple of group_size"
    assert EP.emu_refusal(changed(col=h.stride - 164)) == "col + 165 > obs_stride"
    assert EP.emu_refusal(changed(col=-1)) == "col + 165 > obs_stride"
    assert EP.emu_refusal(changed(col=h.stride - 165)) == ""
    assert EP.emu_refusal(ok, n=-1) == "n < 0"
    assert h.guards()


def test_header_constants_and_mirror():
    """the constants of the header, the structure's mirror in _lib.py (size as the compiler lays it out: 4 ints, 5 pointers)"""
    text = open(os.path.join(_abi.INCLUDE, "emloco_task.h")).read()
    assert "#define EMLOCO_PEOPLE_BODIES {0, 1, 5, 9, 3, 7, 16, 21, 18, 23}" in text and "#define EMLOCO_PEOPLE_FAR 10.0f" in text
    assert (L.PEOPLE_TOPK, L.PEOPLE_JOINTS, L.PEOPLE_WIDTH, L.PEOPLE_FAR) == (5, 10, 165, 10.0) and L.PEOPLE_BODIES == EP.BODIES
    assert C.sizeof(L.CrowdPeople) == 16 + 5 * 8
    assert [f for f, _ in L.CrowdPeople._fields_] == ["n_env", "group_size", "obs_stride", "col", "rb_state", "roots_ws", "obs", "flip_obs",
                                                      "neighbours"]


# ---------------------------------------------------------------------------------------------- host logic, no device
def test_config_block_and_group_refusal():
    from emloco_amd import crowd_people as CP
    assert CP.config_block(dict(group_obs=True, divide_group=True))
    assert not CP.config_block(dict(group_obs=True))                                        # adds nothing without groups, as in the reference
    assert not CP.config_block(dict(group_obs=True, divide_group=False))
    assert not CP.config_block(dict(group_obs=True, divide_group=True, disable_group_obs=True))
    assert not CP.config_block(dict(divide_group=True))
    assert CP.group_refusal(6) is None and CP.group_refusal(512) is None
    for gs in (1, 4, 5):
        assert "group_obs" in CP.group_refusal(gs) and "at least 6" in CP.group_refusal(gs)


def _task(env_cfg, res=32):
    """the task object as `T.__new__(T)` gives it, with the attributes its constructor derives from cfg["env"] ahead of the simulator"""
    from emloco_amd import crowd_people as CP
    from emloco_amd.env.tasks.humanoid_pedestrain_terrain import HumanoidPedestrianTerrainCrowd as T
    t = T.__new__(T)
    t._enable_task_obs, t._num_traj_samples, t.terrain_obs, t.num_height_points = True, 15, True, res * res
    t.velocity_map = bool(env_cfg.get("velocity_map", False))
    t._group_obs = CP.config_block(env_cfg)
    return t


def test_task_sizes_and_detail():
    on = _task(dict(group_obs=True, divide_group=True))
    assert on.get_task_obs_size() == 30 + 1024 + 165
    assert list(on.get_task_obs_size_detail().items()) == [("traj", 30), ("heightmap", 1024), ("people", 165)]
    vel = _task(dict(group_obs=True, divide_group=True, velocity_map=True), res=8)
    assert list(vel.get_task_obs_size_detail().items()) == [("traj", 30), ("heightmap_velocity", 192), ("people", 165)]
    for cfg in (dict(group_obs=True, divide_group=True, disable_group_obs=True), dict(group_obs=True, divide_group=False), dict(divide_group=True)):
        off = _task(cfg)
        assert off.get_task_obs_size() == 30 + 1024 and list(off.get_task_obs_size_detail()) == ["traj", "heightmap"]


def test_shipped_configuration():
    import yaml
    import emloco_amd
    d = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg")
    obs, group = (yaml.safe_load(open(os.path.join(d, f))) for f in ("pacer_group_obs.yaml", "pacer_group.yaml"))
    changed = dict(group_obs=True, velocity_map=False, sensor_res=32, sensor_extent=2)
    assert obs["sim"] == group["sim"] and obs["env"] == {**group["env"], **changed}


def test_entry_point_gate():
    import yaml
    import emloco_amd
    from emloco_amd import run
    d = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg")
    people, crowd, plain = (yaml.safe_load(open(os.path.join(d, f)))["env"] for f in ("pacer_group_obs.yaml", "pacer_group.yaml", "pacer.yaml"))
    flag_sets = [dict(use_policy=True, train_policy=False, test=False), dict(use_policy=False, train_policy=True, test=False),
                 dict(use_policy=True, train_policy=False, test=True), dict(use_policy=True, train_policy=True, test=False)]
    for f in flag_sets:
        for sept in ("amp_sept", "amp_sept_value"):
            assert run.crowd_policy_refusal(people, sept, **f) is None                      # new: the sept network reads a group
            assert "amp_network_sept_cnn_builder" in run.crowd_policy_refusal(crowd, sept, **f)         # unchanged
            assert run.crowd_policy_refusal(plain, sept, **f) is None
            assert run.crowd_policy_refusal(dict(people, disable_group_obs=True), sept, **f)            # stamps off, block off: a crowd map again
            assert "velocity_map" in run.crowd_policy_refusal(dict(people, velocity_map=True), sept, **f)
        for cb in (False, True):
            text = run.crowd_policy_refusal(people, "amp_sept_cnn", cnn_backward=cb, **f)
            assert text and "people" in text and "group_obs" in text
        assert "amp_people" in run.crowd_policy_refusal(people, "amp_people", **f)
        assert (run.crowd_policy_refusal(crowd, "amp_sept_cnn", **f) is None) == (not f["train_policy"])                # unchanged
    assert run.crowd_policy_refusal(people, None, use_policy=False, train_policy=False, test=False) is None


# ---------------------------------------------------------------------------------------------- the network on the CPU
SELF, TRAJ, MAP, PEOPLE, ACTIONS = 368, 30, 1024, 165, 69


def _network(seed=0, detail=None):
    import collections
    import yaml
    from emloco_amd.learning.amp_network_sept_builder import AMPSeptBuilder
    from emloco_amd.learning.amp_policy import DEFAULT_CFG
    from emloco_amd.utils.running_mean_std import RunningMeanStd
    torch.manual_seed(seed)
    detail = detail or collections.OrderedDict([("traj", TRAJ), ("heightmap", MAP), ("people", PEOPLE)])
    task = sum(detail.values())
    rms = RunningMeanStd((SELF + task,)).eval()
    with torch.no_grad():
        rms.running_mean.copy_(torch.randn(SELF + task) * 0.5)
        rms.running_var.copy_(torch.rand(SELF + task) * 2 + 0.25)
    b = AMPSeptBuilder()
    b.load(yaml.safe_load(open(DEFAULT_CFG))["params"]["network"])
    net = b.build("amp", actions_num=ACTIONS, input_shape=(SELF + task,), num_seqs=1, value_size=1, amp_input_shape=(3090,),
                  self_obs_size=SELF, task_obs_size=task, task_obs_size_detail=detail, mean_std=rms)
    return net, rms


def _restated(net, rms, obs):
    """eval_actor / eval_critic of the people network in plain torch, written from the module docstring"""
    F = torch.nn.functional
    p = dict(net.named_parameters())

    def mlp(prefix, x, last_relu=True):
        idx = sorted({int(k.split(".")[1]) for k in p if k.startswith(prefix + ".")})
        for n, i in enumerate(idx):
            x = F.linear(x, p[f"{prefix}.{i}.weight"], p[f"{prefix}.{i}.bias"])
            if last_relu or n < len(idx) - 1:
                x = torch.relu(x)
        return x

    self_obs, task = obs[:, :SELF], obs[:, SELF:]
    lo = SELF + TRAJ + MAP
    std, mean = torch.sqrt(rms.running_var[lo:]).to(obs.dtype), rms.running_mean[lo:].to(obs.dtype)
    pts = (task[:, TRAJ + MAP:] * std + mean).view(-1, 5, 33)
    feat = mlp("_point_net", pts, last_relu=False).max(dim=1)[0]
    x = torch.cat([self_obs, mlp("_task_mlp", task[:, :TRAJ + MAP]), feat], dim=-1)
    mu = F.linear(mlp("actor_mlp", x), p["mu.weight"], p["mu.bias"])
    value = F.linear(mlp("critic_mlp", x), p["value.weight"], p["value.bias"])
    return mu, value


def test_network_shapes_and_reference_keys():
    net, rms = _network()
    assert net.actor_mlp[0].in_features == net.critic_mlp[0].in_features == SELF + 256 + 64
    assert [tuple(m.weight.shape) for m in net._point_net if isinstance(m, torch.nn.Linear)] == [(32, 33), (64, 32), (64, 64)]
    assert all(not m.bias.any() for m in net._point_net if isinstance(m, torch.nn.Linear))
    assert net._task_mlp[0].in_features == TRAJ + MAP
    keys = set(net.state_dict())
    assert {f"_point_net.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")} <= keys
    # a state dict under the reference's key names (amp_network_sept_builder.py / amp_network_builder.py / network_builder.py)
    ref_keys = ["sigma"] + [f"{m}.{i}.{w}" for m in ("actor_mlp", "critic_mlp", "_disc_mlp", "_task_mlp") for i in (0, 2) for w in ("weight", "bias")]
    ref_keys += [f"{m}.{w}" for m in ("value", "mu", "_disc_logits") for w in ("weight", "bias")]
    ref_keys += [f"_point_net.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
    assert sorted(ref_keys) == sorted(keys)
    other, _ = _network(seed=5)
    sd = {k: other.state_dict()[k].clone() for k in ref_keys}
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net._point_net[4].weight, other._point_net[4].weight)
    plain, _ = _network(detail=__import__("collections").OrderedDict([("traj", TRAJ), ("heightmap", MAP)]))
    assert not plain.has_people and not hasattr(plain, "_point_net") and plain.actor_mlp[0].in_features == SELF + 256


def test_network_forward_and_gradients_against_plain_torch():
    net, rms = _network(seed=3)
    with torch.no_grad():                                   # zero biases would hide a bias that is not applied
        for m in list(net._point_net) + list(net._task_mlp):
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    obs = rms(torch.randn(16, SELF + TRAJ + MAP + PEOPLE) * 2)
    mu, sigma = net.eval_actor(obs)
    value = net.eval_critic(obs)
    mu_r, value_r = _restated(net, rms, obs)
    assert mu.shape == (16, ACTIONS) and value.shape == (16, 1) and sigma.shape == mu.shape
    assert torch.allclose(mu, mu_r, rtol=1e-5, atol=1e-6) and torch.allclose(value, value_r, rtol=1e-5, atol=1e-6)
    params = [q for n, q in net.named_parameters() if n.startswith(("_point_net.", "_task_mlp."))]
    w = torch.randn(16, ACTIONS)
    got = torch.autograd.grad((mu * w).sum() + value.sum(), params)
    want = torch.autograd.grad((mu_r * w).sum() + value_r.sum(), params)
    for g, r in zip(got, want):
        assert g.abs().max() > 0 and torch.allclose(g, r, rtol=1e-4, atol=1e-6 * float(r.abs().max()))
    # the people columns reach the output only through the point-net, the map only through the task MLP
    moved = obs.clone()
    moved[:, SELF + TRAJ + MAP:] += 0.5
    assert not torch.equal(net.eval_actor(moved)[0], mu)
    assert torch.equal(net.eval_task(moved[:, SELF:])[:, :256], net.eval_task(obs[:, SELF:])[:, :256])


def test_cnn_network_refuses_a_people_block():
    import collections
    import yaml
    from emloco_amd.learning.amp_network_sept_cnn_builder import AMPSeptCNNBuilder
    from emloco_amd.learning.amp_policy import CNN_CFG, PeopleFrozenPolicy, runner_class
    from emloco_amd.learning.policy_runner import FrozenPolicy
    b = AMPSeptCNNBuilder()
    b.load(yaml.safe_load(open(CNN_CFG))["params"]["network"])
    detail = collections.OrderedDict([("traj", TRAJ), ("heightmap", MAP), ("people", PEOPLE)])
    with pytest.raises(NotImplementedError, match="people"):
        b.build("amp", actions_num=ACTIONS, input_shape=(SELF + 1219,), num_seqs=1, value_size=1, amp_input_shape=(3090,), self_obs_size=SELF,
                task_obs_size=1219, task_obs_size_detail=detail, mean_std=None)
    net, _ = _network()
    plain = types.SimpleNamespace(has_people=False)
    assert runner_class("amp_sept", net) is runner_class("amp_sept_value", net) is PeopleFrozenPolicy
    assert runner_class("amp_sept", plain) is FrozenPolicy and issubclass(PeopleFrozenPolicy, FrozenPolicy)
    assert PeopleFrozenPolicy.act is FrozenPolicy.act and PeopleFrozenPolicy._linear is FrozenPolicy._linear

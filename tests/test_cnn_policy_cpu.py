"""CPU-only: the CNN policy network of the crowd sensor (emloco_amd/learning/amp_network_sept_cnn_builder.py, its torch path on host
tensors) against the fixtures of the reference's own AMPSeptCNNBuilder.Network (tests/golden/gen_golden_cnn_policy.py); its refusals;
the choice of builder and runner by `params.network.name`; run.py's gate for policies on a crowd configuration.
The kernel path of the same module and the frozen runner are tests/test_gpu_cnn_policy.py."""
import argparse
import os

import pytest
import torch

import cnn_policy_cases as K
import emloco_amd

CROWD_ENV = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
PLAIN_ENV = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer.yaml")


@pytest.mark.parametrize("name", K.FIXTURES)
def test_module_on_the_host_matches_the_reference_fixture(name):
    g = K.load(name)
    net, rms = K.build_from(g, "cpu")
    assert list(net.state_dict()) == [str(k) for k in g["keys"]] == [k[3:] for k in g if k.startswith("sd.")]      # same keys, same order
    assert ("_cnn_mlp.0.weight" in net.state_dict()) == (int(g["res"]) != 32) and not hasattr(net, "_task_mlp")
    nobs = torch.from_numpy(g["norm_obs"])
    with torch.no_grad():
        K.close(net.eval_task(nobs[:, int(g["sizes"][0]):]), g["task_out"], what="task embedding")
        mu, sigma = net.eval_actor(nobs)
        K.close(mu, g["mu"], what="mu")
        assert (sigma.numpy() == g["sigma"]).all()
        K.close(net.eval_critic(nobs), g["value"], what="value")
        K.close(net.eval_disc(torch.from_numpy(g["amp_obs"])), g["disc_logits"], what="disc logits")


def test_the_host_path_differentiates():
    g = K.load("cnn_policy_net_r16")
    net, _ = K.build_from(g, "cpu")
    nobs = torch.from_numpy(g["norm_obs"])
    net.eval_actor(nobs)[0].square().mean().backward()              # grad enabled: only the device trunk refuses (tests/test_gpu_cnn_policy.py)
    assert net._task_actor_cnn[0].weight.grad.abs().max() > 0
    assert net._task_critic_cnn[0].weight.grad is None               # built for the checkpoints' sake, never evaluated


def test_input_width_is_self_plus_embedding_plus_path():
    net, _ = K.build("cpu", K.params(), 368, 30, "heightmap_velocity", 3 * 64 * 64)
    assert net.actor_mlp[0].in_features == net.critic_mlp[0].in_features == 368 + 256 + 30
    assert (net.res, net.channels, net.features, net.has_cnn_mlp) == (64, 3, 1024, True)
    assert [tuple(m.weight.shape) for m in net._cnn_mlp if isinstance(m, torch.nn.Linear)] == [(512, 1024), (256, 512)]
    net, _ = K.build("cpu", K.params(), 368, 30, "heightmap", 1024)
    assert (net.res, net.channels, net.features, net.has_cnn_mlp) == (32, 1, 256, False) and not hasattr(net, "_cnn_mlp")


def test_width_refusal_names_both_numbers():
    with pytest.raises(NotImplementedError, match=r"256 features.*units\[-1\] is 128"):
        K.build("cpu", K.params(task_units=(512, 128)), 368, 30, "heightmap_velocity", 3 * 64 * 64)
    with pytest.raises(NotImplementedError, match=r"64 features.*units\[-1\] is 256"):           # res 32, two layers of 16 -> 16 * 2 * 2
        p = K.params()
        p["task_cnn"]["convs"] = p["task_cnn"]["convs"] + [dict(p["task_cnn"]["convs"][0])]
        K.build("cpu", p, 368, 30, "heightmap", 1024)


def _with(**change):
    p = K.params()
    p["task_cnn"].update(change)
    return p


def _conv(**change):
    return dict({"filters": 16, "kernel_size": 4, "strides": 2, "padding": 1}, **change)


@pytest.mark.parametrize("net_params,word", [
    (_with(type="coord_conv2d"), "coord_conv2d"), (_with(type="conv1d"), "conv1d"),
    (_with(convs=[]), "convs"), (_with(convs=[_conv()] * 5), "convs"), (_with(convs=[_conv(kernel_size=3)] * 3), "convs"),
    (_with(convs=[_conv(strides=1)] * 3), "convs"), (_with(convs=[_conv(padding=0)] * 3), "convs"), (_with(convs=[_conv(filters=32)] * 3), "convs"),
    (_with(activation="elu"), "activation"), (dict(K.params(), normalization="layer_norm"), "layer_norm")])
def test_refusals_by_name(net_params, word):
    with pytest.raises(NotImplementedError, match=word):
        K.build("cpu", net_params, 368, 30, "heightmap", 1024)


def test_map_shape_refusals():
    with pytest.raises(NotImplementedError, match="not square"):
        K.build("cpu", K.params(), 368, 30, "heightmap", 1000)
    with pytest.raises(NotImplementedError, match="halve"):
        K.build("cpu", K.params(), 368, 30, "heightmap", 20 * 20)
    with pytest.raises(NotImplementedError, match="halve"):
        K.build("cpu", _with(convs=[_conv()] * 4), 368, 30, "heightmap", 24 * 24)


def test_network_name_chooses_builder_and_runner():
    from emloco_amd.learning import amp_policy as P
    from emloco_amd.learning.amp_network_sept_builder import AMPSeptBuilder
    from emloco_amd.learning.amp_network_sept_cnn_builder import AMPSeptCNNBuilder
    from emloco_amd.learning.policy_runner import CnnFrozenPolicy, FrozenPolicy
    assert P.network_classes("amp_sept") == P.network_classes("amp_sept_value") == (AMPSeptBuilder, FrozenPolicy)
    assert P.network_classes("amp_sept_cnn") == (AMPSeptCNNBuilder, CnnFrozenPolicy)
    assert issubclass(CnnFrozenPolicy, FrozenPolicy) and CnnFrozenPolicy.act is FrozenPolicy.act and CnnFrozenPolicy._linear is FrozenPolicy._linear
    with pytest.raises(NotImplementedError, match="amp_people"):
        P.network_classes("amp_people")
    import yaml
    assert yaml.safe_load(open(P.CNN_CFG))["params"]["network"]["name"] == "amp_sept_cnn"
    assert yaml.safe_load(open(P.DEFAULT_CFG))["params"]["network"]["name"] in P.NETWORKS


def test_gate_for_every_flag_set():
    import yaml
    from emloco_amd import run
    crowd, plain = yaml.safe_load(open(CROWD_ENV))["env"], yaml.safe_load(open(PLAIN_ENV))["env"]
    flag_sets = [dict(use_policy=True, train_policy=False, test=False), dict(use_policy=False, train_policy=True, test=False),
                 dict(use_policy=True, train_policy=False, test=True), dict(use_policy=True, train_policy=True, test=False)]
    for f in flag_sets:
        for sept in ("amp_sept", "amp_sept_value"):
            text = run.crowd_policy_refusal(crowd, sept, **f)                   # the default network cannot read the rows: all flag sets
            assert text and "amp_network_sept_cnn_builder" in text and "amp_humanoid_smpl_cnn_task.yaml" in text
            assert run.crowd_policy_refusal(plain, sept, **f) is None
        text = run.crowd_policy_refusal(crowd, "amp_sept_cnn", **f)
        if f["train_policy"]:
            assert text and "backward is not built" in text and "amp_network_sept_cnn_builder" in text
            assert "backward is not built" in run.crowd_policy_refusal(plain, "amp_sept_cnn", **f)
        else:
            assert text is None and run.crowd_policy_refusal(plain, "amp_sept_cnn", **f) is None      # the reference's `heightmap` branch
        assert "amp_people" in run.crowd_policy_refusal(plain, "amp_people", **f)
    assert run.crowd_policy_refusal(crowd, None, use_policy=False, train_policy=False, test=False) is None      # the noise-action loop


def test_run_stops_or_passes_the_gate_by_cfg_train(tmp_path):
    from emloco_amd import run
    from emloco_amd.learning.amp_policy import CNN_CFG
    base = ["--cfg_env", CROWD_ENV, "--num_envs", "64"]
    with pytest.raises(SystemExit, match="amp_humanoid_smpl_cnn_task.yaml"):
        run.main(base + ["--policy_random_init"])
    with pytest.raises(SystemExit, match="backward is not built"):
        run.main(base + ["--cfg_train", CNN_CFG, "--train_policy"])
    with pytest.raises(SystemExit, match="cannot read"):
        run.main(base + ["--cfg_train", str(tmp_path / "absent.yaml"), "--policy_random_init"])
    args = argparse.Namespace(cfg_train=CNN_CFG)
    assert run.load_policy_cfg(args)["params"]["network"]["name"] == "amp_sept_cnn"
    assert run.load_policy_cfg(argparse.Namespace(cfg_train=""))["params"]["network"]["name"] == "amp_sept_value"

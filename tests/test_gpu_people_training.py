"""GPU: the training step of the people network -- AMPAgent on a task whose observation carries the group observation's `people`
block -- against the float64 restatement of tests/people_training_cases.py: the loss and every gradient with non-trivial statistics,
the three-piece gradient GEMMs, the forms of the step, which statistics the network reads in training mode, the arms, and the
captured step with its checkpoint and frozen runner on pacer_group_obs.yaml."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import people_training_cases as C  # noqa: E402

DEV = "cuda:0"
NON_DISC = ("_point_net.", "_task_mlp.", "actor_mlp.", "critic_mlp.", "mu.", "value.")


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items() if not k.startswith("_")}


def _device_gradients(agent, dd, masks):
    loss, info, _, _ = agent.compute_loss(dd, dropout_masks=masks)
    agent.bucket.zero()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in agent.a2c_network.named_parameters() if p.requires_grad}
    return float(loss), {k: float(v) for k, v in info.items()}, grads


def _close(a, b, rel, abs_, what):
    err, tol = C.max_err(a, b), abs_ + rel * float(b.detach().abs().max())
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


@pytest.fixture(scope="module")
def eval_step():
    """the default form of the step in eval mode with the moments of `draw_statistics`: the agent, its inputs, its loss and gradients,
    the float64 restatement's"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("EMLOCO_PPO_GRAPH", "0")
        agent = C.make_agent(DEV)
    d, masks, stats, ref, grads64 = C.case(agent.a2c_network, training=False)
    C.set_agent_statistics(agent, stats)
    agent.set_eval()
    dd, dm = _to_dev(d), masks.to(DEV)
    loss, info, got = _device_gradients(agent, dd, dm)
    return dict(agent=agent, d=d, masks=masks, stats=stats, ref=ref, grads64=grads64, dd=dd, dm=dm, loss=loss, info=info, got=got)


def test_loss_and_every_gradient_against_float64(eval_step):
    """compute_loss + backward of the default form (stacked actor, direct-gradient accumulation, fused heads), eval mode, uneven
    statistics in all three normalisers, against the float64 restatement.  Loss to 1e-4 relative; discriminator gradients to
    rel 3e-4 / abs 1e-6 (they pass the two-piece gradient GEMMs); every other trained tensor at most five times as far from float64 as
    the float32 restatement on the CPU is (same inputs, same formula, per tensor; both printed).
    Measured on one MI355X (error against float64: device / stock, their ratio): loss 6.6366699e+01 on the device and in float64,
    6.6366692e+01 in float32 on the CPU; critic_mlp.* and value.* 1.2 .. 1.8 times stock (critic_mlp.0.weight 2.6e-7 / 2.1e-7);
    actor_mlp.* and mu.* 1.8 .. 3.3 (actor_mlp.0.weight 4.3e-4 / 1.3e-4); _task_mlp.* 2.5 .. 4.6 (_task_mlp.2.weight 1.9e-4 /
    4.2e-5); _point_net.* 2.2 .. 4.9 (_point_net.0.weight 9.5e-5 / 2.0e-5, the closest to the bar: ratio 4.86).  Two runs give the same
    bits (the next test), so the ratios do not move from run to run; nor does a form of the step move them (_point_net.0.weight 4.87
    with EMLOCO_PPO_HEADS=0, 4.86 with EMLOCO_PPO_STACK_ACTOR=0 and EMLOCO_PPO_DIRECT_GRAD=0).  The GEMMs' arithmetic does: with
    ops.set_matmul_precision("fp32") the same tensor is 2.16 times stock (HISTORY.md)."""
    s = eval_step
    agent, ref, grads64 = s["agent"], s["ref"], s["grads64"]
    net = agent.a2c_network
    assert net.has_people and net.running_var.data_ptr() == agent.running_mean_std.running_var.data_ptr()
    assert any(getattr(p, "_emloco_direct_grad", False) for p in net.parameters()) and agent._stack_actor and agent._fused_heads
    P32 = C.parameters(net, torch.float32)
    r32 = C.restated_loss(P32, s["d"], s["masks"], s["stats"], torch.float32)
    g32 = C.gradients(P32, r32["loss"])
    want = float(ref["loss"].detach())
    print(f"loss: device {s['loss']:.7e}, float64 {want:.7e}, float32 on the CPU {float(r32['loss'].detach()):.7e}")
    assert abs(s["loss"] - want) <= 1e-4 * abs(want)
    for k in ("actor_loss", "critic_loss", "b_loss", "disc_loss", "disc_grad_penalty", "sym_loss"):
        assert abs(s["info"][k] - float(ref[k].detach())) <= 1e-4 * abs(float(ref[k].detach())), (k, s["info"][k], float(ref[k].detach()))
    assert sorted(s["got"]) == sorted(grads64) and all(g is not None for g in grads64.values())
    missed = []
    for k, g in s["got"].items():
        assert float(grads64[k].abs().max()) > 0, k
        if C.is_disc(k):
            _close(g, grads64[k], 3e-4, 1e-6, f"grad {k}")
            continue
        assert k.startswith(NON_DISC), k
        stock, err = C.max_err(g32[k], grads64[k]), C.max_err(g, grads64[k])
        print(f"grad {k}: stock torch fp32 against float64 {stock:.3e}, device {err:.3e}, bar {5 * stock:.3e}"
              + (f", ratio {err / stock:.2f}" if stock else ""))
        if not err <= 5 * stock:                       # (a tensor that stock torch gets exactly must be exact on the device)
            missed.append((k, stock, err))
    assert not missed, missed


def test_three_pieces_govern_every_gradient_on_the_way_to_the_point_net(eval_step, monkeypatch):
    """The step's gradients once more with the process default of ops._BWD_PIECES and once with the OTHER setting (2 for 3 and 3 for 2, for the input and the weight gradients each): two runs of the
    default give identical bits; with the setting changed every non-discriminator gradient keeps its bits -- the people network's
    backward_pieces_for(3) decides there, in the stacked actor, the direct-gradient accumulation and the task MLP alike -- and the
    discriminator's gradients change: the knob did something."""
    from emloco_amd.predictor import ops
    s = eval_step
    _, _, again = _device_gradients(s["agent"], s["dd"], s["dm"])
    for k in again:
        assert torch.equal(again[k], s["got"][k]), f"two identical runs differ in {k}"
    monkeypatch.setattr(ops, "_BWD_PIECES", {kind: 5 - pieces for kind, pieces in ops.backward_pieces().items()})      # 2 <-> 3, per kind
    _, _, moved = _device_gradients(s["agent"], s["dd"], s["dm"])
    for k in moved:
        if not C.is_disc(k):
            assert torch.equal(moved[k], s["got"][k]), f"{k} follows the process-wide setting"
    assert any(not torch.equal(moved[k], s["got"][k]) for k in moved if C.is_disc(k))


def test_reference_shaped_step_agrees_with_the_default_form(eval_step, monkeypatch):
    """tests/test_gpu_policy.py::test_round6_step_variants_agree on the people task: three actor evaluations and autograd's
    accumulation (EMLOCO_PPO_STACK_ACTOR=0, EMLOCO_PPO_DIRECT_GRAD=0) against the default form, same weights, minibatch and
    statistics, eval mode, at that test's bars."""
    s = eval_step
    monkeypatch.setenv("EMLOCO_PPO_GRAPH", "0"); monkeypatch.setenv("EMLOCO_PPO_STACK_ACTOR", "0"); monkeypatch.setenv("EMLOCO_PPO_DIRECT_GRAD", "0")
    ref_agent = C.make_agent(DEV)
    ref_agent.a2c_network.load_state_dict(s["agent"].a2c_network.state_dict())
    assert not ref_agent._stack_actor and not any(getattr(p, "_emloco_direct_grad", False) for p in ref_agent.a2c_network.parameters())
    C.set_agent_statistics(ref_agent, s["stats"])
    ref_agent.set_eval()
    l0, i0, g0 = _device_gradients(ref_agent, s["dd"], s["dm"])
    l1, i1, g1 = s["loss"], s["info"], s["got"]
    assert abs(l0 - l1) <= 2e-5 * abs(l0), (l0, l1)
    assert sorted(i0) == sorted(i1)
    for k in i0:
        assert abs(i0[k] - i1[k]) <= 1e-4 * max(abs(i0[k]), 1e-3), (k, i0[k], i1[k])
    for k in g0:
        _close(g1[k], g0[k], 2e-4, 1e-6, f"grad {k}")


# ------------------------------------------------------------------ training mode
def _train_step(streams):
    """a fresh agent in training mode with count 32, one compute_loss: its info and the three normalisers' moments afterwards"""
    agent = C.make_agent(DEV)
    d, masks, stats, ref, _ = C.case(agent.a2c_network, training=True)
    C.set_agent_statistics(agent, stats)
    agent.set_train()
    torch.cuda.synchronize()
    branch = tuple(torch.cuda.Stream(device=DEV) for _ in range(3)) if streams else None
    loss, info, _, _ = agent.compute_loss(_to_dev(d), dropout_masks=masks.to(DEV), branch_streams=branch)
    torch.cuda.synchronize()
    moments = {name: tuple(t.detach().clone() for t in (r.running_mean, r.running_var, r.count))
               for name, r in (("obs", agent.running_mean_std), ("value", agent.value_mean_std), ("amp", agent._amp_input_mean_std))}
    return dict(agent=agent, d=d, masks=masks, stats=stats, ref=ref, loss=loss.detach().clone(), info={k: v.detach().clone() for k, v in info.items()},
                moments=moments)


@pytest.fixture(scope="module")
def one_chain():
    return _train_step(streams=False)


def test_training_mode_network_reads_the_statistics_after_the_third_update(one_chain):
    """set_train(), count 32, one chain: critic loss, actor loss and the three normalisers' moments against the training-mode
    restatement, in which obs / flipped / next are normalised with S0 / S1 / S2 and EVERY evaluation un-normalises the people columns
    with S3 (the reference's order, amp_continuous.py:345-377).  Losses to 1e-4 relative, moments to 2e-6, counts exact.  The case tells
    S3 from S1: restated critic loss 1.1005639 with S3, 1.0386153 with S1, 5.6e-2 apart (560 times the bar).  Measured on one MI355X:
    critic loss 1.1005639 (before the three updates were issued ahead of the critic's fork: 1.0386152, the S1 value, and this test
    failed on it), actor loss 1.0930419e-01 against 1.0929710e-01 restated (6.5e-5 of it: the float32 log-probabilities are near
    -100, where one ulp is 7.6e-6)."""
    s = one_chain
    ref, d, masks, stats = s["ref"], s["d"], s["masks"], s["stats"]
    P = C.parameters(s["agent"].a2c_network, torch.float64)
    c3 = float(ref["critic_loss"].detach())
    c1 = float(C.restated_loss(P, d, masks, stats, torch.float64, training=True, critic_reads=1)["critic_loss"].detach())
    got_c, got_a, want_a = float(s["info"]["critic_loss"]), float(s["info"]["actor_loss"]), float(ref["actor_loss"].detach())
    print(f"critic loss: device {got_c:.7e}, restated with S3 {c3:.7e}, with S1 {c1:.7e}; actor loss: device {got_a:.7e}, restated {want_a:.7e}")
    assert abs(c3 - c1) > 100 * 1e-4 * abs(c3), "the case cannot tell S1 from S3"
    for name, after in (("obs", ref["obs_stats"][3]), ("amp", ref["amp_stats"]), ("value", stats["value"])):
        mean, var, count = s["moments"][name]
        np.testing.assert_allclose(mean.cpu().numpy(), after[0].numpy(), rtol=2e-6, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(var.cpu().numpy(), after[1].numpy(), rtol=2e-6, atol=2e-6, err_msg=name)
        assert float(count) == float(after[2]), name
    assert float(s["moments"]["obs"][2]) == 80.0 and float(s["moments"]["amp"][2]) == 80.0 and float(s["moments"]["value"][2]) == 32.0
    assert abs(got_a - want_a) <= 1e-4 * abs(want_a), (got_a, want_a)
    assert abs(got_c - c3) <= 1e-4 * abs(c3), (got_c, c3, c1)


def test_arms_do_not_change_the_numbers(one_chain):
    """The same step with the critic, the discriminator and the symmetry loss on three streams of their own, on a fresh identical
    agent: critic loss, actor loss and the normalisers' moments have the bits of the one-chain call -- every read of the statistics is
    ordered behind the third update, on every stream -- and the loss and every other entry of info (the discriminator's, which are
    computed on its arm, the bound and symmetry losses) agree with it at the bars of
    tests/test_gpu_policy.py::test_round6_step_variants_agree: a join that came too early would show there.  Each form runs once: this
    checks the order of issue, it does not hunt a race (with the critic forked behind the first update the single run on one MI355X
    also gave equal bits: both forms read S1)."""
    arms = _train_step(streams=True)
    for k in ("critic_loss", "actor_loss"):
        assert torch.equal(arms["info"][k], one_chain["info"][k]), (k, float(arms["info"][k]), float(one_chain["info"][k]))
    for name in ("obs", "value", "amp"):
        for a, b in zip(arms["moments"][name], one_chain["moments"][name]):
            assert torch.equal(a, b), name
    l0, l1 = float(one_chain["loss"]), float(arms["loss"])
    assert abs(l0 - l1) <= 2e-5 * abs(l0), (l0, l1)
    assert sorted(arms["info"]) == sorted(one_chain["info"]) and {"disc_loss", "disc_grad_penalty", "b_loss", "sym_loss"} <= set(arms["info"])
    for k in one_chain["info"]:
        i0, i1 = float(one_chain["info"][k]), float(arms["info"][k])
        print(f"{k}: one chain {i0:.7e}, arms {i1:.7e}")
        assert abs(i0 - i1) <= 1e-4 * max(abs(i0), 1e-3), (k, i0, i1)


# ------------------------------------------------------------------ the captured step, its checkpoint, the frozen runner
def _seed(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


def _make_env(num_envs):
    import emloco_amd
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group_obs.yaml")
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", "--small_terrain", "--cfg_env", cfg_env])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(dict(num_env_group=8))
    return create_rlgpu_env(args, cfg, cfg_train)


def test_captured_step_equals_the_eager_step_and_its_checkpoint_plays(monkeypatch, tmp_path):
    """tests/test_gpu_env.py::test_amp_agent_optimiser_step_as_a_hip_graph_equals_the_eager_step on pacer_group_obs.yaml (groups of 8, 16
    envs, horizon 8, minibatches of 64, two mini-epochs, two epochs): weights and statistics of the captured and the eager agent at
    that test's bars.  The step is captured with its arms (EMLOCO_PPO_BRANCHES=1: the eight steps of this run are fewer than the timing
    trial between the candidates takes).  Then the people columns' variance has left 1, the network's aliases of the normaliser's buffers
    survive save / restore into a second agent, and AMPPolicyBundle -- PeopleFrozenPolicy on trained, uneven statistics -- gives the
    agent's eval_actor(running_mean_std(obs)) clamped to +-1 within 1e-5 + 1e-4 of the largest value."""
    import yaml
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.amp_policy import DEFAULT_CFG, AMPPolicyBundle, PeopleFrozenPolicy
    from emloco_amd.run import RLGPUEnv
    monkeypatch.setenv("EMLOCO_PPO_GRAPH", "1")
    monkeypatch.setenv("EMLOCO_PPO_BRANCHES", "1")
    outs = []
    for mode in ("0", "1"):
        _seed(21)
        raw = _make_env(16)
        cfg = yaml.safe_load(open(DEFAULT_CFG))
        cfg["params"]["network"]["mlp"]["units"] = [256, 128]
        cfg["params"]["network"]["disc"]["units"] = [128, 64]
        cfg["params"]["config"].update(horizon_length=8, minibatch_size=64, amp_minibatch_size=64, amp_batch_size=64,
                                       amp_obs_demo_buffer_size=512, amp_replay_buffer_size=512, mini_epochs=2)
        agent = AMPAgent(RLGPUEnv(raw), cfg, seed=4)
        assert agent.a2c_network.has_people
        agent.use_graph = mode == "1"
        torch.manual_seed(33)
        infos = [agent.train_epoch() for _ in range(2)]
        assert (agent._graph is not None) == (mode == "1") and (mode == "0" or agent._g_arms)
        outs.append((torch.cat([p.detach().reshape(-1) for p in agent.a2c_network.parameters()]).clone(), agent.running_mean_std.running_mean.clone(),
                     agent.running_mean_std.running_var.clone(), agent._amp_input_mean_std.running_var.clone(), infos[-1]))
    (w0, m0, o0, v0, i0), (w1, m1, o1, v1, i1) = outs
    assert torch.isfinite(w1).all() and (w0 - w1).abs().max().item() <= 2e-5 * w0.abs().max().item() + 1e-6
    assert torch.allclose(m0, m1, rtol=1e-9, atol=1e-9) and torch.allclose(o0, o1, rtol=1e-9, atol=1e-9) and torch.allclose(v0, v1, rtol=1e-9, atol=1e-9)
    for k in ("actor_loss", "critic_loss", "disc_loss", "kl", "b_loss"):
        assert abs(i0[k] - i1[k]) <= 5e-3 * abs(i0[k]) + 1e-5, (k, i0[k], i1[k])
    # the statistics the point-net reads, and the alias it reads them through
    net, rms = agent.a2c_network, agent.running_mean_std
    assert (rms.running_var[-C.PEOPLE:] != 1).all() and float(rms.count) == 1 + 2 * 4 * (3 if agent.motion_sym_loss else 1) * 64

    def aliased(a):
        return (a.a2c_network.running_mean.data_ptr() == a.running_mean_std.running_mean.data_ptr()
                and a.a2c_network.running_var.data_ptr() == a.running_mean_std.running_var.data_ptr())

    assert aliased(agent)
    path = str(tmp_path / "people_policy")
    agent.save(path)
    _seed(22)                                                      # another initialisation: the checkpoint decides
    second = AMPAgent(RLGPUEnv(raw), cfg, seed=9)
    assert aliased(second) and not torch.equal(second.running_mean_std.running_var, rms.running_var)
    second.restore(path + ".pth")
    assert aliased(agent) and aliased(second)
    assert torch.equal(second.a2c_network.running_var, rms.running_var) and torch.equal(second.a2c_network.running_mean, rms.running_mean)
    bundle = AMPPolicyBundle(raw.task, cfg_train=cfg, checkpoint=path + ".pth", deterministic=True)
    assert isinstance(bundle.frozen, PeopleFrozenPolicy) and list(bundle.a2c_network.state_dict()) == list(net.state_dict())
    obs = raw.task.obs_buf.detach().clone()
    assert torch.isfinite(obs).all()
    agent.set_eval(); second.set_eval()
    with torch.no_grad():
        mu = net.eval_actor(rms(obs))[0]
        mu2 = second.a2c_network.eval_actor(second.running_mean_std(obs))[0]
    assert torch.equal(mu, mu2)
    ref = mu.clamp(-1.0, 1.0)
    tol = 1e-5 + 1e-4 * float(ref.abs().max())
    err = C.max_err(bundle.policy(obs), ref)
    print(f"the bundle's policy against the agent's own network: {err:.3e}, bar {tol:.3e}")
    assert err <= tol

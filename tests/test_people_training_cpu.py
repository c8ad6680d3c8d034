"""CPU-only: what tests/test_gpu_people_training.py compares the device with.  The plain-torch restatement of the people network's
training step (tests/people_training_cases.py) against the module on the CPU with non-trivial statistics; its float64 statistics
rule against the reference class's recorded output; and the conditions the device test relies on, for the seed it uses."""
import numpy as np
import pytest
import torch

import people_training_cases as C


@pytest.fixture(scope="module")
def eval_case():
    net, rms = C.build_network()
    d, masks, stats, ref, grads = C.case(net, training=False)
    C.write_statistics(rms, stats["obs"])
    return net, rms, d, masks, stats, ref, grads


def test_restated_actor_and_critic_equal_the_module_with_uneven_statistics(eval_case):
    """eval mode, the moments of `draw_statistics`: mu, value and the gradients of every parameter on the path at the tolerances of
    tests/test_crowd_people_cpu.py::test_network_forward_and_gradients_against_plain_torch (the module runs torch layers here)."""
    net, rms, d, masks, stats, _, _ = eval_case
    assert net.has_people and net.running_var.data_ptr() == rms.running_var.data_ptr()
    assert float((rms.running_var[C.LO:] - 1).abs().min()) > 1e-3 and float(rms.running_mean[C.LO:].abs().min()) > 1e-4
    obs = rms(d["obs"])
    assert torch.equal(obs, C.rms_normalise(stats["obs"], d["obs"], torch.float32))
    mu, _ = net.eval_actor(obs)
    value = net.eval_critic(obs)
    P = dict(net.named_parameters())
    r = C.Restated(P, stats["obs"], torch.float32)
    mu_r, value_r = r.actor(obs), r.critic(obs)
    assert torch.allclose(mu, mu_r, rtol=1e-5, atol=1e-6) and torch.allclose(value, value_r, rtol=1e-5, atol=1e-6)
    names = [n for n, q in P.items() if q.requires_grad and not C.is_disc(n)]
    w = torch.randn(C.B, C.ACTIONS, generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad((mu * w).sum() + value.sum(), [P[n] for n in names])
    want = torch.autograd.grad((mu_r * w).sum() + value_r.sum(), [P[n] for n in names])
    for n, g, t in zip(names, got, want):
        assert g.abs().max() > 0 and torch.allclose(g, t, rtol=1e-4, atol=1e-6 * float(t.abs().max())), n
    # what the statistics are there to catch: the identity un-normalisation, a variance without its root, an epsilon, a shifted range
    wrong = [(torch.zeros(C.OBS, dtype=torch.float64), torch.ones(C.OBS, dtype=torch.float64)),
             (stats["obs"][0], stats["obs"][1] ** 2), (stats["obs"][0], stats["obs"][1] + 0.01),
             (torch.roll(stats["obs"][0], 1), torch.roll(stats["obs"][1], 1)), (torch.roll(stats["obs"][0], C.POINT), torch.roll(stats["obs"][1], C.POINT))]
    for bad in wrong:
        assert not torch.allclose(C.Restated(P, bad, torch.float32).actor(obs), mu, rtol=1e-3, atol=1e-4)


def test_statistics_rule_reproduces_the_reference_fixture():
    """The float64 rule against what the reference's own class recorded (tests/golden/running_mean_std.npz, the fixture of
    test_running_mean_std_training_update_matches_the_reference_class), at that test's 2e-6: four batches, the last two under
    freeze_partial(3)."""
    g = C.rms_fixture()
    cols = g["x0"].shape[1]
    stats = (torch.zeros(cols, dtype=torch.float64), torch.ones(cols, dtype=torch.float64), torch.ones((), dtype=torch.float64))
    for i in range(int(g["n_batches"])):
        x = torch.from_numpy(g[f"x{i}"])
        y = C.rms_normalise(stats, x, torch.float64)
        stats = C.rms_merge(stats, x, diff=3 if i >= 2 else None)
        np.testing.assert_allclose(y.numpy(), g[f"y{i}"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(stats[0].numpy(), g[f"mean{i}"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(stats[1].numpy(), g[f"var{i}"], rtol=2e-6, atol=2e-6)
        assert float(stats[2]) == float(g[f"count{i}"])


def _tied(out):
    """rows of the (B, 5, 64) point-net output whose five neighbours are bit-equal"""
    return (out == out[:, :1]).all(dim=2).all(dim=1)


def _margin(out):
    top = out.sort(dim=1, descending=True)[0]
    return top[:, 0] - top[:, 1]


def test_conditions_of_the_chosen_seed(eval_case):
    net, rms, d, masks, stats, ref64, _ = eval_case
    ref32 = C.restated_loss(C.parameters(net, torch.float32), d, masks, stats, torch.float32)
    lo = C.LO
    for r in (ref64, ref32):
        for tag, key in (("actor", 0), ("critic", 0), ("flip", 1), ("next", 2)):
            idx, out = r["argmax"][tag]
            tied = _tied(out)
            # the all-zero-neighbour rows: five identical point rows, exactly tied maxima -- and no other row is tied
            assert tied.nonzero().flatten().tolist() == list(C.ROWS_ALL_ZERO), tag
            x = r["normalised"][key]
            assert (x[C.ROW_CLAMPED, lo:lo + 2 * C.POINT] == 5.0).all() and (x[C.ROW_CLAMPED, lo + 2 * C.POINT:lo + 3 * C.POINT] == -5.0).all()
            assert (x[C.ROW_CLAMPED, lo + 3 * C.POINT:].abs() < 5.0).any()
            one = x[C.ROW_ONE_NEIGHBOUR, lo:].view(C.TOPK, C.POINT)
            assert torch.equal(one[1], one[2]) and torch.equal(one[1], one[4]) and not torch.equal(one[0], one[1])
    # float32 and float64 agree on the surrogate's branch and on the winning neighbour of every untied row and feature
    assert torch.equal(ref64["clip_branch"], ref32["clip_branch"])
    assert 2 <= int(ref64["clip_branch"].sum()) <= C.B - 2                       # both branches are taken
    assert 0.25 < float(ref64["ratio"].min()) and float(ref64["ratio"].max()) < 4.0
    for tag in ("actor", "critic", "flip", "next"):
        (i64, o64), (i32, _) = ref64["argmax"][tag], ref32["argmax"][tag]
        untied = ~_tied(o64)
        # (where the one-neighbour row's four empty neighbours win, they tie among themselves: compare the winning VALUES' rows there)
        same = (i64 == i32) | (torch.gather(o64, 1, i64[:, None]) == torch.gather(o64, 1, i32[:, None]))[:, 0]
        assert same[untied].all(), tag
        # and no untied maximum is decided by rounding: every margin is a hundred times float32's resolution of these outputs (order one)
        real = _margin(o64)[untied]
        assert float(real[real > 0].min()) > 1e-5, (tag, float(real[real > 0].min()))


def test_training_mode_case_tells_the_first_update_from_the_third():
    """The case of the device test (d): with count 32 the moments after one update and after three differ by a large fraction of the
    batch's, and the critic loss with them: on this file's network 1.4198647 with S3 and 1.3085292 with S1, 7.8e-2 apart, against the
    hundred times the 1e-4 bar the device test asks of its own network."""
    net, _ = C.build_network()
    d, masks, stats, ref, _ = C.case(net, training=True)
    P = C.parameters(net, torch.float64)
    s1 = C.restated_loss(P, d, masks, stats, torch.float64, training=True, critic_reads=1)
    c3, c1 = float(ref["critic_loss"].detach()), float(s1["critic_loss"].detach())
    print(f"critic loss un-normalised with S3 {c3:.7e}, with S1 {c1:.7e}: apart by {abs(c3 - c1) / abs(c3):.3e} of it")
    assert abs(c3 - c1) > 100 * 1e-4 * abs(c3)
    assert float(s1["actor_loss"].detach()) == float(ref["actor_loss"].detach())                   # (the actor reads S3 either way)
    S = ref["obs_stats"]
    assert [float(s[2]) for s in S] == [32.0, 48.0, 64.0, 80.0]
    moved = (S[1][0] - S[0][0]).abs().max() / torch.sqrt(S[0][1]).max()
    assert float(moved) > 0.1

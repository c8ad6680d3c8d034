"""GPU: the LocoVal evaluation (`run.py --test`, emloco_amd/learning/locoval_eval.py, csrc/eval_kernels.hip) on the MI355X.

  * the three kernels against the reference's player (fixture tests/golden/locoval_player.npz): 257 envs replay the fixture's games
    with shifted game boundaries; records bit for bit, the reduction's moments to 1e-12;
  * the evaluator on the real env against the plain-torch restatement (tests/test_locoval_eval_cpu.py) driving an identically seeded
    second env with the same deterministic actions;
  * `python -m emloco_amd.run --test ...` end to end;
  * two ranks sharing the GPU: the all-reduced report is the report of the union of both ranks' records.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]
REPORT_KEYS = ("games", "av_reward", "av_steps", "av_value_loss", "av_loc", "av_pow", "av_disc", "av_total", "std_loc", "std_pow",
               "std_disc", "std_total", "corr_total", "corr_loc", "corr_pow", "corr_disc", "terminated", "inverted", "lines",
               "games_requested", "envs", "games_per_env", "shortfall", "steps")


def _make_env(num_envs, seed=3, rank=0):
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(num_envs), "--seed", str(seed), *ENV_ARGS])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    return RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train, rank=rank))


def _vnet(dev, seed=11):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    torch.manual_seed(seed)
    return ValuePoseNet(True, True).to(dev)


# ------------------------------------------------------------------------------------------------ kernels vs the reference's player
def test_eval_kernels_match_the_reference_player_for_257_shifted_envs():
    import ctypes as C
    from emloco_amd.learning.locoval_eval import RECORD_DTYPE, RECORD_WORDS, moments_from_records
    from emloco_amd.predictor import ops
    from locoval_harness import _ptr as P, eval_state
    from test_locoval_eval_cpu import assert_records_equal_fixture, fixture, run_restatement, shifted_script
    fx = fixture()
    E, K = 257, len(fx["lengths"])
    dev = torch.device("cuda:0")
    s, order = shifted_script(fx, E)
    R, _, _ = run_restatement(fx, E)
    want = R.record_array()
    assert_records_equal_fixture(want, fx, order)
    g = torch.Generator().manual_seed(5)
    wp, ip, iv = (torch.randn(*sh, generator=g).to(dev) for sh in ((E, 15, 3), (E, 24, 3), (E, 2)))
    st, b = eval_state(E, K, int(fx["step_to_pred"]), float(fx["gamma"]), device=dev, waypoint_traj=wp, init_pose=ip, init_vel=iv)
    lib = ops._lib()
    value = torch.zeros(E, device=dev)
    records = torch.zeros(E * K * RECORD_WORDS, dtype=torch.int32, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rr_all = up(np.stack([s["r_loc"], s["r_pow"]], axis=2))
    disc_all, dones_all, term_all, inv_all = up(s["disc"]), up(s["dones"]), up(s["terminate"]), up(s["inverted"].astype(np.uint8))
    vals = up(fx["values"])[up(s["gid"])]
    traj_rel, pose_rel = wp[:, :13] - wp[:, :1], ip - ip[:, :1]
    for t in range(s["r_loc"].shape[0]):
        assert lib.emloco_locoval_eval_step(C.byref(st), P(rr_all[t]), P(disc_all[t]), P(dones_all[t]), P(term_all[t]), P(inv_all[t]), None) == 0
        first = b["row_mask"] != 0
        if t in (0, 30, 173):                                      # the LocoVal inputs of the first steps, origin-relative
            assert torch.equal(b["traj13"][first], traj_rel[first]) and torch.equal(b["pose"][first], pose_rel[first])
            assert torch.equal(b["vel"][first], iv[first]) and bool(first.any())
        value = torch.where(first, vals[t], value)                # stands where emloco_locoval_fwd_rows writes the masked rows
        assert lib.emloco_locoval_eval_finish(C.byref(st), P(value), P(records), None) == 0
    moments = torch.zeros(20, dtype=torch.float64, device=dev)
    assert lib.emloco_locoval_eval_reduce(E, K, P(records), P(b["games"]), P(moments), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(b["games"].cpu(), torch.full((E,), K, dtype=torch.int32)) and int(b["n_full"].item()) == E
    raw = records.cpu().numpy().view(RECORD_DTYPE).reshape(E, K)
    got = raw[want["env"], want["game"]]
    for k in RECORD_DTYPE.names:
        assert got[k].tobytes() == want[k].tobytes(), k
    np.testing.assert_allclose(moments.cpu().numpy(), moments_from_records(want), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ the evaluator on the real env
def test_evaluator_on_the_real_env_equals_the_restatement(tmp_path):
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from test_locoval_eval_cpu import Restatement
    E = 64
    env = _make_env(E)
    task = env.env.task
    dev = torch.device(task.device)
    torch.manual_seed(21)
    bundle = AMPPolicyBundle(task, deterministic=True)
    path = str(tmp_path / "locoval.pth")
    torch.save({k: v.cpu() for k, v in _vnet(dev).state_dict().items()}, path)
    vnet = ValuePoseNet(True, True).to(dev)
    vnet.load_state_dict(torch.load(path, map_location=dev))
    ev = LocoValEvaluator(env, bundle, vnet, games_num=2 * E)
    assert ev.games_per_env == 2
    torch.manual_seed(1234)                                        # the resets' random draws (and the seed of the device generator
    rep = ev.run(say=None)                                         # of reset_done) as for the second env below
    got = ev.records()
    assert rep["games"] == 2 * E == len(got) and rep["shortfall"] == 0
    n_steps = ev.steps_run

    env2 = _make_env(E)                                            # identically seeded second env, the same deterministic actions
    t2 = env2.env.task
    R = Restatement(E, int(t2.step_to_pred), 0.99, 2, device=dev)
    torch.manual_seed(1234)
    with torch.no_grad():
        for k in range(n_steps):
            if k == 0:
                env2.env.reset(torch.arange(E, device=dev))
            else:
                env2.env.reset_done()
            act = bundle.frozen.act(t2.obs_buf, deterministic=True).clone()
            _o, _r, dones, infos = env2.step(act)
            disc = bundle.disc_reward(infos["amp_obs"]).clone()
            rr = t2.reward_raw.clone()
            value_fn = lambda first: vnet(env2.env.get_waypoint_traj()[:, :13], env2.env.get_init_pose(), env2.env.get_init_vel()).reshape(E)
            R.step(rr[:, 0], rr[:, 1], disc, dones.clone(), infos["terminate"].clone(), t2.inverted.clone(), value_fn)
    want = R.record_array()
    assert len(want) == len(got)
    for k in want.dtype.names:
        if want[k].dtype.kind == "f":
            assert want[k].tobytes() == got[k].tobytes(), k
        else:
            assert np.array_equal(want[k], got[k]), k
    assert (got["steps"] >= 1).all() and np.isfinite(got["value"]).all()


# ------------------------------------------------------------------------------------------------ the command line
def test_run_test_cli_prints_the_reference_summary(tmp_path):
    path = str(tmp_path / "locoval.pth")
    torch.save({k: v.cpu() for k, v in _vnet("cpu").state_dict().items()}, path)
    out, recs = str(tmp_path / "eval.json"), str(tmp_path / "games.npz")
    p = subprocess.run([sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "64", "--seed", "1", *ENV_ARGS,
                        "--policy_random_init", "--valuenet_path", path, "--games_num", "128", "--eval_out", out, "--eval_records", recs],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    for head in ("av reward: ", "av_loc: ", "std_loc: ", "Correlation: ", " Total reward: ", "Loc reward: ", "Pow reward: ", "Disc reward: "):
        assert any(ln.startswith(head) for ln in lines), head
    rep = json.load(open(out))
    assert rep["games"] == 128 and rep["games_per_env"] == 2 and rep["envs"] == 64
    for k in REPORT_KEYS:
        assert k in rep, k
    g = np.load(recs)
    assert len(g["value"]) == 128 and set(np.unique(g["game"])) == {0, 1}


# ------------------------------------------------------------------------------------------------ two ranks sharing the GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_worker(rank, world, port, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        from emloco_amd.dist import init_from_env
        init_from_env("gloo")
        torch.cuda.set_device(0)
        from emloco_amd.learning.amp_policy import AMPPolicyBundle
        from emloco_amd.learning.locoval_eval import LocoValEvaluator
        env = _make_env(32, rank=rank)
        torch.manual_seed(21)
        bundle = AMPPolicyBundle(env.env.task, deterministic=True)
        ev = LocoValEvaluator(env, bundle, _vnet(env.env.task.device), games_num=128)
        rep = ev.run(say=None)
        rec = ev.records()
        torch.distributed.destroy_process_group()
        q.put((rank, rep, rec))
    except Exception as e:                                        # the parent reads the failure instead of waiting for the timeout
        import traceback
        q.put((rank, {"error": traceback.format_exc()}, None))
        raise e


def test_two_ranks_all_reduce_the_report_of_the_union_of_their_records():
    import torch.multiprocessing as mp
    from emloco_amd.learning.locoval_eval import moments_from_records, report_from_moments
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
    for r, rep, _ in res:
        assert "error" not in rep, rep["error"]
    for p in procs:
        assert p.exitcode == 0
    (_, r0, rec0), (_, r1, rec1) = res
    assert r0["games"] == r1["games"] == 128 and r0["envs"] == 64 and r0["games_per_env"] == 2
    assert r0["moments"] == r1["moments"] and r0["lines"] == r1["lines"]
    union = np.concatenate([rec0, rec1])
    ref = report_from_moments(moments_from_records(union))
    np.testing.assert_allclose(np.array(r0["moments"]), moments_from_records(union), rtol=1e-12, atol=0)
    for k in ("av_reward", "av_steps", "av_value_loss", "av_total", "std_total", "corr_total", "corr_loc", "corr_pow", "corr_disc"):
        assert abs(r0[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    assert r0["terminated"] == ref["terminated"] and r0["inverted"] == ref["inverted"]

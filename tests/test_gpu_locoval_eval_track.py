"""GPU: the path tracking of the LocoVal evaluation (`run.py --test --eval_tracks`; emloco_locoval_eval_track / _track_reduce) on the MI355X.

  * the scripted cases of tests/track_cases.py through the library, in the product's order (step -> track -> finish), against the float64
    restatement with the bound derived there; two runs give the same bytes; the reduction against `track_moments_from_records`;
  * one small real rollout (8 envs, random-init policy and LocoVal, 16 games): at every step exp(-2 dev_now^2) is the step's
    reward_raw[:, 0]; the LocoVal records and report are byte-identical with and without `track`; with two networks the track records
    are the single-network run's;
  * `python -m emloco_amd.run --test --pred_path ... --eval_tracks --eval_records`: the `track` / `walked` / `target` columns line up with
    `pred_row` (the stored targets are points of the table row the game walked) and the tracking block is printed.

Measured on the device, as printed by `track_cases.check` (fractions of the bound 8 * 2^-24 * C + 8 * 2^-24 * |want|): main case ade 0.003,
fde 0.022, mean_dev / max_dev / final_dev 0.118, path_len 0.005, per-step deviation 0.149, samples 0.156 ulp(C); cap case at most 0.047
for the records, 0.099 per step, samples 0.907 ulp(C); max |exp(-2 dev_now^2) - reward_raw[:, 0]| over the 71 steps of the rollout
5.5e-8 = 0.93 x 2^-24.
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

import track_cases as TC  # noqa: E402
from locoval_harness import _ptr as P, eval_state, track_state  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]


# ------------------------------------------------------------------------------------------------ the scripted cases on the device
def run_device(case):
    from emloco_amd.learning.locoval_eval import RECORD_WORDS, TRACK_DTYPE, TRACK_WORDS
    from emloco_amd.predictor import ops
    E, G, T = case["E"], case["G"], case["T"]
    dev = torch.device("cuda:0")
    lib = ops._lib()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    st, b = eval_state(E, G, device=dev)
    t, _tb = track_state(case, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, root, prog, dones = up(case["verts"][:T]), up(case["root"][:T]), up(case["progress"][:T]), up(case["dones"][:T])
    records, track = z(E * G * RECORD_WORDS, dt=torch.int32), z(E * G * TRACK_WORDS, dt=torch.int32)
    samples, value, rr, dev_now = z(E, G, TC.TRACK_SAMPLES, 4), z(E), torch.ones(E, 2, device=dev), z(T, E)
    for k in range(T):
        t.root_pos, t.traj_verts, t.progress_buf, t.dev_now = root[k].data_ptr(), verts[k].data_ptr(), prog[k].data_ptr(), dev_now[k].data_ptr()
        assert lib.emloco_locoval_eval_step(C.byref(st), P(rr), None, P(dones[k]), None, None, None) == 0
        assert lib.emloco_locoval_eval_track(C.byref(st), C.byref(t), P(track), P(samples), None) == 0
        assert lib.emloco_locoval_eval_finish(C.byref(st), P(value), P(records), None) == 0
    moments = z(ops.TRACK_MOMENTS, dt=torch.float64)
    assert lib.emloco_locoval_track_reduce(E, G, P(track), P(b["games"]), 4.0, P(moments), None) == 0
    torch.cuda.synchronize()
    return dict(track=track.cpu().numpy().view(TRACK_DTYPE).reshape(E, G), samples=samples.cpu().numpy(), games=b["games"].cpu().numpy(),
                dev_now=dev_now.cpu().numpy(), moments=moments.cpu().numpy())


@pytest.mark.parametrize("name", ["main", "cap"])
def test_scripted_cases_on_the_device_equal_the_float64_restatement(name):
    from emloco_amd.learning.locoval_eval import track_moments_from_records
    case = TC.main_case() if name == "main" else TC.cap_case()
    want = TC.restate(case)
    got, again = run_device(case), run_device(case)
    worst = TC.check(case, want, got["track"], got["samples"], got["games"], got["dev_now"])
    assert max(worst.values()) <= 1.0
    for k in ("track", "samples", "games", "dev_now", "moments"):               # no atomics, a fixed order: the same bytes
        assert np.ascontiguousarray(got[k]).view(np.uint8).tobytes() == np.ascontiguousarray(again[k]).view(np.uint8).tobytes(), k
    env, game = np.nonzero(np.arange(case["G"])[None, :] < got["games"][:, None])
    np.testing.assert_allclose(got["moments"], track_moments_from_records(got["track"][env, game]), rtol=1e-12, atol=0)
    if name == "cap":
        assert list(got["track"]["n_samples"][:, 0]) == [16, 16, 16]


# ------------------------------------------------------------------------------------------------ one small real rollout
def _make_env(num_envs, seed=3):
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(num_envs), "--seed", str(seed), *ENV_ARGS])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    return RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))


def _rollout(nets, track, each_step=None):
    """An identically seeded env, policy and LocoVal network(s) every time: the same games (tests/test_gpu_locoval_eval.py)."""
    from emloco_amd.learning.amp_policy import AMPPolicyBundle
    from emloco_amd.learning.locoval_eval import LocoValEvaluator
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    E = 8
    env = _make_env(E)
    task = env.env.task
    torch.manual_seed(21)
    bundle = AMPPolicyBundle(task, deterministic=True)
    made = []
    for seed, (pose, vel) in nets:
        torch.manual_seed(seed)
        made.append(ValuePoseNet(pose, vel).to(task.device))
    ev = LocoValEvaluator(env, bundle, made if len(made) > 1 else made[0], games_num=16, **({"track": True} if track else {}))
    assert ev.games_per_env == 2
    torch.manual_seed(1234)
    while ev.steps_run < 2000:
        ev.step_once()
        if each_step is not None:
            each_step(ev, task)
        if ev.envs_full() == E:
            break
    rep = ev.report(say=None)
    return ev, rep


def test_real_rollout_tracks_the_reward_and_leaves_the_evaluation_as_it_was():
    one = [(11, (True, True))]
    worst = [0.0]

    def each_step(ev, task):
        dev_now = ev._tb["dev_now"].cpu().numpy().astype(np.float64)
        loc = task.reward_raw[:, 0].cpu().numpy().astype(np.float64)
        worst[0] = max(worst[0], float(np.abs(np.exp(-2.0 * dev_now * dev_now) - loc).max()))

    ev_t, rep_t = _rollout(one, True, each_step)
    print(f"max |exp(-2 dev_now^2) - reward_raw[:, 0]| over {ev_t.steps_run} steps: {worst[0]:.3e} ({worst[0] / 2.0 ** -24:.2f} x 2^-24)")
    assert worst[0] <= 4 * 2.0 ** -24                           # one fp32 exp of a value <= 1
    ev_p, rep_p = _rollout(one, False)
    assert "tracking" in rep_t and "tracking" not in rep_p and not hasattr(ev_p, "_tb")
    trk = rep_t.pop("tracking")
    assert json.dumps(rep_t, sort_keys=True, default=float) == json.dumps(rep_p, sort_keys=True, default=float)
    assert ev_t.records().tobytes() == ev_p.records().tobytes() and ev_t.steps_run == ev_p.steps_run
    # the block against the records, and the records against the games
    rec, lv = ev_t.track_records(), ev_t.records()
    walked, target = ev_t.track_samples()
    assert len(rec) == 16 == trk["games"] and np.array_equal(rec["env"], lv["env"]) and np.array_equal(rec["game"], lv["game"])
    assert np.array_equal(rec["n_samples"], lv["steps"] // 12) and walked.shape == target.shape == (16, 16, 2)
    assert (rec["max_dev"] >= rec["final_dev"]).all() and (rec["max_dev"] >= rec["mean_dev"]).all() and (rec["mean_dev"] > 0).all()
    for i in range(16):
        n = int(rec["n_samples"][i])
        assert not walked[i, n:].any() and not target[i, n:].any()
        if n:
            d = np.sqrt(((walked[i, :n].astype(np.float64) - target[i, :n]) ** 2).sum(axis=1))
            # (a sanity check of the layout, not a precision bound: the stored samples are fp32 differences of world coordinates of up to
            # hundreds of metres, 3e-5 m an ulp)
            assert abs(d.mean() - rec["ade"][i]) <= 1e-3 and abs(d[-1] - rec["fde"][i]) <= 1e-3
    s = rec["n_samples"] > 0
    assert trk["games_sampled"] == int(s.sum()) and abs(trk["av_mean_dev"] - rec["mean_dev"].astype(np.float64).mean()) < 1e-9
    assert len(trk["lines"]) == 4 and isinstance(trk["corr_value_ade"], float)
    # two networks on the same games: one tracking launch per step, the same track records
    ev_m, rep_m = _rollout(one + [(12, (False, True))], True)
    assert ev_m.track_records().tobytes() == rec.tobytes()
    assert ev_m.track_samples()[0].tobytes() == walked.tobytes() and ev_m.track_samples()[1].tobytes() == target.tobytes()
    assert ev_m.records(0).tobytes() == lv.tobytes() and len(rep_m["tracking"]["corr_value_ade"]) == 2
    assert rep_m["tracking"]["moments"] == trk["moments"]


# ------------------------------------------------------------------------------------------------ the command line
def test_run_test_pred_path_eval_tracks_end_to_end(tmp_path):
    """16 envs on a 96-row predicted-path table, one game each: every game's stored targets are points of the table row it walked.
    (Without --init_heading, which turns a placed path about its first vertex to the humanoid's heading: the reset then only translates
    the row, tests/test_gpu_traj_densify.py.)"""
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    from test_gpu_traj_densify import _write_pred_table
    table_path = str(tmp_path / "preds.pkl")
    table = _write_pred_table(table_path)
    torch.manual_seed(11)
    net = str(tmp_path / "locoval.pth")
    torch.save({k: v.cpu() for k, v in ValuePoseNet(True, True).state_dict().items()}, net)
    out, recs = str(tmp_path / "eval.json"), str(tmp_path / "games.npz")
    p = subprocess.run([sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "16", "--seed", "1", "--random_heading", "--policy_random_init",
                        "--valuenet_path", net, "--games_num", "16", "--pred_path", "--pred_traj_file", table_path, "--eval_tracks",
                        "--eval_out", out, "--eval_records", recs], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    for head in ("tracking: 16 games", "av_ade: ", "av_mean_dev: ", "Correlation of value with ade: "):
        assert any(ln.startswith(head) for ln in lines), head
    rep = json.load(open(out))
    assert rep["games"] == 16 and rep["tracking"]["games"] == 16 and rep["tracking"]["stride"] == 12
    g = np.load(recs)
    assert len(g["pred_row"]) == len(g["track"]) == len(g["walked"]) == len(g["target"]) == 16
    assert g["track"].dtype.names == ("ade", "fde", "mean_dev", "max_dev", "final_dev", "path_len", "n_samples")
    assert np.array_equal(g["track"]["n_samples"], g["steps"] // 12)
    dense = np.stack([v["coord_dense"] for v in table.values()])
    dt, dur = np.float32(rep["tracking"]["dt"]), np.float32(rep["tracking"]["traj_dur"])
    checked = 0
    for i in range(16):
        row = (dense[g["pred_row"][i]] - dense[g["pred_row"][i]][:1]).astype(np.float32)
        for k in range(int(g["track"]["n_samples"][i])):
            want = TC.target64(row, 12 * (k + 1), dt, dur)[:2]
            np.testing.assert_allclose(g["target"][i, k], want, atol=5e-4)            # the table row placed at the root, in fp32 (rows differ by metres)
            checked += 1
    assert checked > 0

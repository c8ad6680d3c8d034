"""CPU-only: the bookkeeping of the game statistics (the numpy restatement of tests/episode_stats_ref.py against numbers worked out by
hand), `report_from_moments`, the merge of moment vectors, and the training driver of `emloco_amd.run` on stub agents without a device:
checkpoint names and cadence, the per-epoch log, --resume, the refusal of --steps with --max_iterations, and the entry point's output
without the driver's flags."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_ref as ER                                                   # noqa: E402
from emloco_amd import run                                                       # noqa: E402
from emloco_amd.learning.episode_stats import MOMENT_NAMES, MOMENT_OPS, merge_moments, report_from_moments      # noqa: E402


def test_moment_names_follow_the_header():
    from emloco_amd import _abi, _lib as L
    import re
    txt = open(os.path.join(_abi.INCLUDE, "emloco_task.h")).read()
    enum = {k.lower(): int(v) for k, v in re.findall(r"EMLOCO_EPM_(\w+)\s*=\s*(\d+)", txt)}
    assert enum == {n: i for i, n in enumerate(MOMENT_NAMES)}
    assert len(MOMENT_NAMES) == L.EPISODE_MOMENTS == int(re.search(r"#define EMLOCO_EPISODE_MOMENTS (\d+)", txt).group(1))
    assert [n for n, op in zip(MOMENT_NAMES, MOMENT_OPS) if op != "sum"] == ["min_len", "max_len", "max_speed2", "max_ang_speed2"]
    assert {k: int(v) for k, v in re.findall(r"EMLOCO_EPISODE_(RUNS|TIMEOUT|FAR|FALLEN)\s*=\s*(\d+)", txt)} == \
        dict(RUNS=ER.RUNS, TIMEOUT=ER.TIMEOUT, FAR=ER.FAR, FALLEN=ER.FALLEN)


def test_hand_written_script():
    """3 envs, 6 steps, fail_dist 4 (threshold 16), every number a short binary fraction.
    env 0: reward 0.5 per step; ends at step 2 (flag only, d2 = 1: timeout) and at step 6 (d2 = 25: far): games of 2 and 4 steps,
           returns 1.0 and 2.0
    env 1: reward 0.25, inverted, penalty 0.5 -> -0.125 per step; ends at step 3 with terminate set, d2 = 4: fallen, 3 steps, -0.375;
           three more steps of a game in progress
    env 2: reward 1.0, never ends
    reward_raw is (0.75, -0.25) everywhere."""
    ref = ER.EpisodeStatsRef(3, 4.0, inverted_penalty=0.5)
    rew = np.array([0.5, 0.25, 1.0], np.float32)
    raw = np.tile(np.array([0.75, -0.25], np.float32), (3, 1))
    inverted = np.array([False, True, False])
    script = {2: ([1, 0, 0], [0, 0, 0], [1.0, 0.0, 0.0]), 3: ([0, 1, 0], [0, 1, 0], [0.0, 4.0, 0.0]), 6: ([1, 0, 0], [1, 0, 0], [25.0, 0.0, 0.0])}
    finished = []
    for step in range(1, 7):
        reset, term, d2 = script.get(step, ([0, 0, 0], [0, 0, 0], [0.0, 0.0, 0.0]))
        out = ref.step(rew, raw, np.array(reset), np.array(term), np.array(d2, np.float32), inverted=inverted)
        finished += [(step, e, *out[e].tolist()) for e in range(3) if reset[e]]
    assert finished == [(2, 0, 1.0, 1.5, -0.5, 2.0, ER.TIMEOUT), (3, 1, -0.375, 2.25, -0.75, 3.0, ER.FALLEN), (6, 0, 2.0, 3.0, -1.0, 4.0, ER.FAR)]
    assert ref.running.tolist() == [[0.0, 0.0, 0.0, 0.0], [-0.375, 2.25, -0.75, 3.0], [6.0, 4.5, -1.5, 6.0]]
    rep = ref.report()
    assert rep["games"] == 3 and (rep["timeout"], rep["far"], rep["fallen"]) == (1 / 3, 1 / 3, 1 / 3)
    assert (rep["len_mean"], rep["len_min"], rep["len_max"]) == (3.0, 2.0, 4.0)
    assert rep["len_std"] == pytest.approx(math.sqrt(2.0 / 3.0), rel=1e-14)
    assert rep["ret_mean"] == pytest.approx(2.625 / 3.0, rel=1e-15)
    assert rep["ret_std"] == pytest.approx(math.sqrt((1.0 + 4.0 + 0.140625) / 3.0 - (2.625 / 3.0) ** 2), rel=1e-13)
    assert rep["ret_loc_mean"] == 2.25 and rep["ret_pow_mean"] == -0.75
    assert rep["nonfinite_steps"] == 0 and rep["max_speed"] == 0.0
    # the totals were cleared, the games in progress go on: a second epoch reports only its own games
    out = ref.step(rew, raw, np.array([0, 1, 0]), np.array([0, 0, 0]), np.zeros(3, np.float32), inverted=inverted)
    assert out[1].tolist() == [-0.5, 3.0, -1.0, 4.0, ER.TIMEOUT]
    rep = ref.report()
    assert rep["games"] == 1 and rep["timeout"] == 1.0 and rep["len_mean"] == 4.0 and rep["len_std"] == 0.0 and rep["ret_mean"] == -0.5


def test_running_sums_are_float32_in_step_order():
    """0.1 added ten times in float32 is not 1.0: the restatement adds one step after the other in float32, not in float64"""
    ref = ER.EpisodeStatsRef(1, 4.0)
    z, one = np.zeros(1, np.int64), np.ones(1, np.int64)
    for step in range(10):
        out = ref.step([0.1], [[0.1, 0.0]], one if step == 9 else z, z, [0.0])
    s = np.float32(0.0)
    for _ in range(10):
        s = np.float32(s + np.float32(0.1))
    assert out[0, 0] == s and float(s) != float(np.float32(1.0)) and out[0, 3] == 10.0


def test_health_values():
    ref = ER.EpisodeStatsRef(2, 4.0)
    st = np.zeros((2, 24, 13), np.float32)
    st[0, 5, 7:10] = (3.0, 4.0, 12.0)
    st[1, 7, 10:13] = (1.0, 2.0, 2.0)
    z = np.zeros(2, np.int64)
    ref.step([0, 0], np.zeros((2, 2)), z, z, [0, 0], rb_state=st)
    st2 = st.copy()
    st2[1, 3, 0] = np.nan
    st2[1, 4, 8] = np.inf
    ref.step([0, 0], np.zeros((2, 2)), z, z, [0, 0], rb_state=st2)
    assert ref.totals[0, ER.K["max_speed2"]] == 169.0 and ref.totals[1, ER.K["max_ang_speed2"]] == 9.0
    assert ref.totals[:, ER.K["nonfinite_steps"]].tolist() == [0.0, 1.0] and ref.totals[1, ER.K["max_speed2"]] == np.inf
    rep = ref.report()
    assert rep["games"] == 0 and rep["nonfinite_steps"] == 1 and rep["max_ang_speed"] == 3.0 and rep["max_speed"] == math.inf


def test_report_from_moments_edge_cases():
    zero = report_from_moments(np.zeros(len(MOMENT_NAMES)))
    assert zero == dict(games=0, max_speed=0.0, max_ang_speed=0.0, nonfinite_steps=0)          # no mean, no share: nothing was divided
    m = dict.fromkeys(MOMENT_NAMES, 0.0)
    m.update(games=1, fallen=1, sum_len=7, sum_len2=49, min_len=7, max_len=7, sum_ret=2.5, sum_ret2=6.25, sum_loc=3.0, sum_pow=-0.5, max_speed2=4.0)
    one = report_from_moments([m[n] for n in MOMENT_NAMES])
    assert one["games"] == 1 and one["len_std"] == 0.0 and one["ret_std"] == 0.0 and one["len_mean"] == 7.0 and one["ret_mean"] == 2.5
    assert (one["timeout"], one["far"], one["fallen"]) == (0.0, 0.0, 1.0) and one["max_speed"] == 2.0
    m.update(games=7, timeout=2, far=4, fallen=1, sum_len=70, sum_len2=800)
    rep = report_from_moments([m[n] for n in MOMENT_NAMES])
    assert rep["timeout"] + rep["far"] + rep["fallen"] == pytest.approx(1.0, abs=1e-15)


def _random_script(E, T, seed):
    g = np.random.default_rng(seed)
    return [dict(rew=g.random(E, dtype=np.float32), raw=g.normal(size=(E, 2)).astype(np.float32), reset=(g.random(E) < 0.3).astype(np.int64),
                 term=(g.random(E) < 0.5).astype(np.int64), d2=(g.random(E) * 32).astype(np.float32),
                 rb=g.normal(size=(E, 24, 13)).astype(np.float32), inv=g.random(E) < 0.4) for _ in range(T)]


def test_merging_shards_equals_the_concatenation():
    E, cut = 10, 4
    whole, a, b = ER.EpisodeStatsRef(E, 4.0, 0.3), ER.EpisodeStatsRef(cut, 4.0, 0.3), ER.EpisodeStatsRef(E - cut, 4.0, 0.3)
    for s in _random_script(E, 9, 5):
        whole.step(s["rew"], s["raw"], s["reset"], s["term"], s["d2"], s["rb"], s["inv"])
        a.step(*[s[k][:cut] for k in ("rew", "raw", "reset", "term", "d2", "rb", "inv")])
        b.step(*[s[k][cut:] for k in ("rew", "raw", "reset", "term", "d2", "rb", "inv")])
    (mw, scale), (ma, _), (mb, _) = whole.moments(), a.moments(), b.moments()
    assert mw[0] >= 5
    merged = merge_moments(ma, mb)
    for k, op in enumerate(MOMENT_OPS):
        if op == "sum":
            assert abs(merged[k] - mw[k]) <= 1e-12 * scale[k], MOMENT_NAMES[k]
        else:
            assert merged[k] == mw[k], MOMENT_NAMES[k]
    # a shard without games does not lend its 0 to the minimum length
    none = np.zeros(len(MOMENT_NAMES))
    none[ER.K["max_speed2"]] = 1e6
    m = merge_moments(none, mw)
    assert m[ER.K["min_len"]] == mw[ER.K["min_len"]] > 0 and m[ER.K["max_speed2"]] == 1e6 and merge_moments(none, none)[ER.K["min_len"]] == 0.0


# ---------------------------------------------------------------------------------------------------------------- the driver
class StubTrainee:
    """What run_training asks of a trainee, on the host: an epoch is `horizon_length` steps of 8 envs."""
    kind = "locoval"
    horizon_length = 4

    def __init__(self):
        self.epoch_num, self.frame, self.saved = 0, 0, []

    def run_epoch(self):
        self.epoch_num += 1
        self.frame += 8 * self.horizon_length
        m = dict.fromkeys(MOMENT_NAMES, 0.0)
        m.update(games=2, timeout=2, sum_len=20, sum_len2=208, min_len=8, max_len=12, sum_ret=3.0, sum_ret2=5.0)
        return dict(games=report_from_moments([m[n] for n in MOMENT_NAMES]), vnet_pred=0.25, combine_rwd=0.5, vnet_loss=0.125 * self.epoch_num,
                    fps_step=1000.0, fps_total=900.0, ep_time=0.5)

    def save(self, mof, epoch=None):
        path = mof + ("_valuenet.pth" if epoch is None else "_valuenet_" + str(epoch).zfill(8) + ".pth")
        torch.save(dict(epoch=self.epoch_num, frame=self.frame), path)
        self.saved.append((self.epoch_num, os.path.basename(path)))

    def resume(self, mof):
        ck = torch.load(mof + "_valuenet.pth")
        self.epoch_num, self.frame = ck["epoch"], ck["frame"]

    def final_line(self, n, dt):
        return f"final: {n} steps"


def _opt(tmp_path, *extra):
    return run.train_options(["--num_envs", "8", "--network_path", str(tmp_path), *extra])


def test_driver_cadence_log_and_resume(tmp_path):
    said = []
    t = StubTrainee()
    assert run.run_training(t, _opt(tmp_path, "--experiment", "exp", "--max_iterations", "11", "--save_freq", "2"), said.append) == 11
    # latest every 2 epochs, an intermediate every 10, the latest again at the end
    assert t.saved == [(2, "exp_valuenet.pth"), (4, "exp_valuenet.pth"), (6, "exp_valuenet.pth"), (8, "exp_valuenet.pth"), (10, "exp_valuenet.pth"),
                       (10, "exp_valuenet_00000010.pth"), (11, "exp_valuenet.pth")]
    assert sorted(os.listdir(tmp_path)) == ["exp_log.jsonl", "exp_valuenet.pth", "exp_valuenet_00000010.pth"]
    lines = [json.loads(ln) for ln in open(tmp_path / "exp_log.jsonl")]
    assert [r["epoch"] for r in lines] == list(range(1, 12)) and [r["frame"] for r in lines] == [32 * k for k in range(1, 12)]
    assert lines[2]["games"]["len_mean"] == 10.0 and lines[2]["vnet_loss"] == 0.375 and lines[2]["wall_time"] > 0 and lines[2]["ep_time"] == 0.5
    # the reference's line (common_agent.py:236), one per epoch, then the end-of-run line
    assert said[0] == "Ep: 1\trwd: 1.50\tvnet_pred: 0.25\tcombine_rwd: 0.50\tvnet_loss: 0.125\tfps_step: 1000.0\tfps_total: 900.0\tep_time:0.5\tframe: 32\teps_len: 10.0"
    assert sum(s.startswith("Ep: ") for s in said) == 11 and said[-1] == "final: 44 steps"
    assert said.count("latest model saved") == 5 and said.count("intermediate model saved") == 1
    # --resume: numbering and frames carry on, the log is appended; --max_iterations counts the experiment's epochs in total
    said, t2 = [], StubTrainee()
    assert run.run_training(t2, _opt(tmp_path, "--experiment", "exp", "--max_iterations", "14", "--save_freq", "2", "--resume"), said.append) == 3
    assert said[0].startswith("resumed ") and "epoch 11" in said[0] and said[1].startswith("Ep: 12\t")
    assert t2.saved == [(12, "exp_valuenet.pth"), (14, "exp_valuenet.pth"), (14, "exp_valuenet.pth")]
    lines = [json.loads(ln) for ln in open(tmp_path / "exp_log.jsonl")]
    assert [r["epoch"] for r in lines] == list(range(1, 15)) and lines[-1]["frame"] == 32 * 14
    # without --resume the experiment starts over: a fresh log
    t3 = StubTrainee()
    run.run_training(t3, _opt(tmp_path, "--experiment", "exp", "--steps", "6", "--save_freq", "0"), lambda s: None)
    assert t3.epoch_num == 2 and t3.saved == [(2, "exp_valuenet.pth")] and len(open(tmp_path / "exp_log.jsonl").readlines()) == 2


def test_stats_alone_prints_and_writes_nothing(tmp_path, monkeypatch):
    said, t = [], StubTrainee()
    monkeypatch.chdir(tmp_path)
    run.run_training(t, run.train_options(["--stats", "--steps", "8"]), said.append)
    assert [s[:5] for s in said] == ["Ep: 1", "Ep: 2", "final"] and t.saved == [] and os.listdir(tmp_path) == []
    said, t = [], StubTrainee()
    run.run_training(t, run.train_options(["--max_iterations", "3"]), said.append)          # neither statistics nor files: the end-of-run line
    assert said == ["final: 12 steps"] and t.saved == []


def test_policy_line_is_the_short_variant():
    info = dict(games=dict(games=3, ret_mean=12.345, len_mean=80.0), fps_step=5e5, fps_total=2e5, ep_time=1.25)
    assert run.epoch_line("policy", 7, 4096, info) == "Ep: 7\trwd: 12.3\tfps_step: 500000.0\tfps_total: 200000.0\tep_time:1.2\tframe: 4096\teps_len: 80.0"
    assert run.epoch_line("policy", 7, 4096, dict(info, games=dict(games=0))).startswith("Ep: 7\trwd: 0.0\t")


def test_options_are_checked_before_a_device_is_touched():
    with pytest.raises(SystemExit, match="--steps and --max_iterations"):
        run.train_options(["--steps", "64", "--max_iterations", "2"])
    with pytest.raises(SystemExit, match="--steps and --max_iterations"):
        run.main(["--num_envs", "8", "--steps", "64", "--max_iterations", "2"])                # (main stops there: nothing was built)
    with pytest.raises(SystemExit, match="--resume continues an experiment"):
        run.train_options(["--resume"])
    with pytest.raises(SystemExit, match="belong to training"):
        run.train_options(["--test", "--experiment", "x"])
    argv = ["--num_envs", "8", "--steps", "64", "--random_heading"]
    opt = run.train_options(argv)
    assert argv == ["--num_envs", "8", "--random_heading"] and opt["steps"] == 64
    assert not opt["driver"] and not opt["stats"] and opt["model_output_file"] is None          # today's command line: today's loop
    opt = run.train_options(["--experiment", "walk", "--network_path", "out/dir"])
    assert opt["driver"] and opt["stats"] and opt["model_output_file"] == os.path.join("out/dir", "walk") and opt["save_freq"] == 200


def test_checkpoint_names_of_both_trainers(tmp_path):
    """LocoValRollout.save / AMPAgent.save under the trainees: the reference's file names (common_agent.py:248-265), rank 0 only"""
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    net = torch.nn.Linear(3, 1)
    states = []
    lv = types.SimpleNamespace(_sync_fit=lambda: None, valuenet=net, horizon_length=32, epoch_num=0, frames=0, num_actors=8)
    lv.save = lambda mof, epoch=None: LocoValRollout.save(lv, mof, epoch)
    lv.save_state = lambda mof: states.append(mof)
    mof = str(tmp_path / "exp")
    t = run.LocoValTrainee(lv)
    t.save(mof)
    t.save(mof, 1000)
    assert sorted(os.listdir(tmp_path)) == ["exp_valuenet.pth", "exp_valuenet_00001000.pth"] and states == [mof]
    sd = torch.load(tmp_path / "exp_valuenet_00001000.pth")
    assert set(sd) == {"weight", "bias"} and torch.equal(sd["weight"], net.weight.detach())            # a plain state_dict
    run.LocoValTrainee(lv, world=2, rank=1).save(str(tmp_path / "other"))
    assert len(os.listdir(tmp_path)) == 2
    pa = types.SimpleNamespace(horizon_length=32, epoch_num=3, frame=96, get_full_state_weights=lambda: dict(epoch=3, frame=96))
    pa.save = lambda fn: AMPAgent.save(pa, fn)
    p = run.PolicyTrainee(pa)
    assert pa.episode_stats is None
    p.save(mof)
    p.save(mof, 1000)
    assert sorted(f for f in os.listdir(tmp_path) if "valuenet" not in f) == ["exp.pth", "exp_00001000.pth"]
    assert torch.load(tmp_path / "exp.pth") == dict(epoch=3, frame=96)


def test_entry_point_without_the_new_flags_prints_what_it_printed(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(run, "time", types.SimpleNamespace(time=iter([10.0, 12.0]).__next__))
    agent = types.SimpleNamespace(horizon_length=32, vnet_loss=0.03125, fitted_episodes=17, calls=0)
    agent.play_steps = lambda: setattr(agent, "calls", agent.calls + 1)
    said = []
    run.locoval_loop(agent, 8, 2, 40, said.append)
    n, dt, num_envs, world = 64, 2.0, 8, 2
    assert agent.calls == 2 and said == [f"fps_step: {num_envs * world * n / dt:,.0f} env-steps/s ({n} steps of {num_envs} envs x {world} ranks), "
                                         f"LocoVal loss {agent.vnet_loss:.4f}, {agent.fitted_episodes} episodes fitted"]
    info = dict(fps_step=123456.7, fps_total=65432.1, actor_loss=0.5, critic_loss=0.25, disc_loss=0.125, kl=0.001)
    pol = types.SimpleNamespace(horizon_length=32, epoch_num=0)

    def train_epoch():
        pol.epoch_num += 1
        return info
    pol.train_epoch = train_epoch
    said = []
    run.policy_loop(pol, 33, said.append)
    assert said == [f"epoch {k}: fps_step {info['fps_step']:,.0f} fps_total {info['fps_total']:,.0f} "
                    f"a_loss {info['actor_loss']:.4f} c_loss {info['critic_loss']:.4f} disc_loss {info['disc_loss']:.4f} kl {info['kl']:.5f}" for k in (1, 2)]

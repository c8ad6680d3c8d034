"""GPU: the game statistics kernels (emloco_episode_stats_step / emloco_episode_stats_reduce, include/emloco_task.h) against the numpy
restatement of tests/episode_stats_ref.py, on scripted buffers without a simulator; their agreement with the flags kernel on the states of
tests/task_cases.py; and `EpisodeStats` / the LocoVal checkpoints inside the rollout loop at 64 envs.

Bars.  Running values, finished games, targets, squared distances, speed maxima, counts, minima and maxima: bit for bit (the kernel's
translation unit is built without contraction and adds in step order, as the restatement does; the target is the host
TrajGenerator.calc_pos in float32).  The reduced sums: 1e-12 of the sum of |terms| of the entry (a double tree sum over at most
70 x 12 terms against numpy's order).  Every finished game of a script sits at least 1 % of fail_dist^2 off the threshold, so no cause
hangs on a rounding.

The scripted cases: 70 envs (neither a multiple of the 64-lane wave nor of the 4 envs of a workgroup) over 12 steps -- "mixed": env 0
ends at its first step, env 1 never ends, env 2 ends twice, the other envs end at random steps; "all_end": the same with a step at which
every env ends (a script cannot hold both that step and an env that never ends) -- and 1 env.  A third of the envs is inverted, the penalty
scale is 0.3, all three causes occur."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_stats_ref as ER                                                   # noqa: E402

DEV = "cuda"
DT, EPISODE_DUR, FAIL_DIST, PENALTY = 1.0 / 30.0, 168.0 / 30.0, 4.0, 0.3
SENT = 12345.0
BAND = 64


def _lib():
    from emloco_amd import _lib as L
    return L.require_device()


def _host_traj(verts):
    from emloco_amd.env.util.traj_generator import TrajGenerator
    tg = TrajGenerator(verts.shape[0], EPISODE_DUR, 101, "cpu", 2.0, 0.5, 1.5, 2.0, 0.15)
    tg._verts_flat.copy_(torch.from_numpy(verts).reshape(-1, 3))
    return tg


def make_script(E, T, variant, seed):
    """The inputs of T steps as numpy arrays, with the host's targets; see the module docstring."""
    g = np.random.default_rng(seed)
    reset = (g.random((T, E)) < 0.12).astype(np.int64)
    for e, steps in ((0, [0]), (1, []), (2, [3, 8])):
        if e < E:
            reset[:, e] = 0
            reset[steps, e] = 1
    if E == 1:
        reset[:, 0] = 0
        reset[[0, 4, 8], 0] = 1
    if variant == "all_end":
        reset[6, :] = 1
    cause = g.integers(1, 4, size=(T, E))                         # of the steps at which a game ends
    for e in range(min(E, 3)):                                    # the first finished games cover the three causes whatever the draw
        cause[:, e] = 1 + (np.arange(T) + e) % 3
    term = ((cause != ER.TIMEOUT) & (reset != 0)).astype(np.int64)
    term |= ((g.random((T, E)) < 0.1) & (reset == 0)).astype(np.int64)          # a terminate flag without a reset flag ends nothing
    progress = np.zeros((T, E), np.int64)
    run = np.zeros(E, np.int64)
    for t in range(T):
        run += 1
        progress[t] = run + (17 if t % 2 else 0) * (np.arange(E) % 3 == 1)       # (some targets further along the path)
        run[reset[t] != 0] = 0
    heading = g.random(E) * 2 * np.pi
    speed = 0.03 + 0.05 * g.random(E)
    i = np.arange(101)[None, :, None]
    verts = (np.stack([np.cos(heading), np.sin(heading), np.zeros(E)], -1)[:, None, :] * speed[:, None, None] * i
             + 0.01 * g.normal(size=(E, 101, 3)) + np.array([30.0, -20.0, 0.0]) * g.random((E, 1, 1))).astype(np.float32)
    tg = _host_traj(verts)
    times = torch.from_numpy(progress).float() * DT
    tar = np.stack([tg.calc_pos(torch.arange(E), times[t]).numpy() for t in range(T)])         # [T][E][3] float32
    # roots: beyond the fail distance where the script says "far", well inside everywhere else
    far = (cause == ER.FAR) & (reset != 0)
    radius = np.where(far, 4.1 + 1.9 * g.random((T, E)), 3.9 * g.random((T, E)))
    phi = g.random((T, E)) * 2 * np.pi
    rb = g.normal(size=(T, E, 24, 13)).astype(np.float32)
    rb[..., 7:13] *= 3.0
    rb[:, :, 0, 0] = (tar[..., 0] + radius * np.cos(phi)).astype(np.float32)
    rb[:, :, 0, 1] = (tar[..., 1] + radius * np.sin(phi)).astype(np.float32)
    return dict(E=E, T=T, reset=reset, term=term, progress=progress, verts=verts, tar=tar, rb=rb, traj_dur=float(tg.get_traj_duration()),
                rew=(g.random((T, E)) * 1.1).astype(np.float32), raw=g.normal(size=(T, E, 2)).astype(np.float32),
                inverted=(np.arange(E) % 3 == 0) if E > 1 else np.array([True]))


class _Out:
    """an output buffer with a sentinel band before and behind it"""

    def __init__(self, shape, dtype, fill=0.0):
        n = int(np.prod(shape))
        self.buf = torch.full((BAND + n + BAND,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[BAND:BAND + n].view(shape)
        self.t.fill_(fill)

    def bands_intact(self):
        return bool((self.buf[:BAND] == SENT).all() and (self.buf[-BAND:] == SENT).all())


class Device:
    """the buffers of one run of the kernels, driven by a script"""

    def __init__(self, sc, penalty=PENALTY, fill=0.0):
        from emloco_amd import _lib as L
        E = self.E = sc["E"]
        self.sc, self.penalty = sc, penalty
        self.verts = torch.from_numpy(sc["verts"]).to(DEV)
        self.inverted = torch.from_numpy(sc["inverted"].astype(np.uint8)).to(DEV)
        self.running = _Out((E, L.EPISODE_RUNNING), torch.float32, fill)
        self.totals = _Out((E, L.EPISODE_MOMENTS), torch.float64, fill)
        self.game_out = _Out((E, L.EPISODE_GAME_OUT), torch.float32, fill)
        self.moments = _Out((L.EPISODE_MOMENTS,), torch.float64, SENT)
        self.keep = []

    def step(self, t, rb=None, n_envs=None, null=None, fail_dist=FAIL_DIST):
        sc = self.sc
        ins = dict(rew=torch.from_numpy(sc["rew"][t]), raw=torch.from_numpy(sc["raw"][t]), reset=torch.from_numpy(sc["reset"][t]),
                   term=torch.from_numpy(sc["term"][t]), progress=torch.from_numpy(sc["progress"][t]),
                   rb=torch.from_numpy(sc["rb"][t] if rb is None else rb))
        ins = {k: v.to(DEV).contiguous() for k, v in ins.items()}
        ins.update(verts=self.verts, running=self.running.t, totals=self.totals.t)
        self.keep.append(ins)
        p = lambda k: None if k == null else C.c_void_p(ins[k].data_ptr())
        rc = _lib().emloco_episode_stats_step(
            self.E if n_envs is None else n_envs, p("rew"), p("raw"), p("reset"), p("term"), p("progress"), p("rb"), p("verts"),
            None if self.penalty is None else C.c_void_p(self.inverted.data_ptr()), float(self.penalty or 0.0), DT, sc["traj_dur"], fail_dist,
            p("running"), p("totals"), C.c_void_p(self.game_out.t.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def reduce(self, n_envs=None, null=None):
        p = lambda k, o: None if k == null else C.c_void_p(o.t.data_ptr())
        rc = _lib().emloco_episode_stats_reduce(self.E if n_envs is None else n_envs, p("totals", self.totals), p("moments", self.moments),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def intact(self):
        return all(o.bands_intact() for o in (self.running, self.totals, self.game_out, self.moments))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _ref_step(ref, sc, t, rb=None):
    d2 = ER.d2_f32(sc["tar"][t], (sc["rb"][t] if rb is None else rb)[:, 0, :2])
    return d2, ref.step(sc["rew"][t], sc["raw"][t], sc["reset"][t], sc["term"][t], d2, sc["rb"][t] if rb is None else rb, sc["inverted"])


def _check_moments(got, ref_m, scale):
    from emloco_amd.learning.episode_stats import MOMENT_NAMES, MOMENT_OPS
    exact = {"games", "timeout", "far", "fallen", "nonfinite_steps"}
    for k, (name, op) in enumerate(zip(MOMENT_NAMES, MOMENT_OPS)):
        err = abs(got[k] - ref_m[k])
        print(f"    {name:16s} device {got[k]!r:24} reference {ref_m[k]!r:24} |diff| {err:.3e} bar {0.0 if op != 'sum' or name in exact else 1e-12 * scale[k]:.3e}")
        if op != "sum" or name in exact:
            assert got[k] == ref_m[k], name
        else:
            assert err <= 1e-12 * scale[k], name


@pytest.mark.parametrize("E,variant", [(70, "mixed"), (70, "all_end"), (1, "mixed")])
def test_scripted_steps_against_the_numpy_reference(E, variant):
    sc = make_script(E, 12, variant, seed=11 + E)
    dev, ref = Device(sc), ER.EpisodeStatsRef(E, FAIL_DIST, PENALTY)
    seen = set()
    for t in range(sc["T"]):
        d2, want = _ref_step(ref, sc, t)
        done = sc["reset"][t] != 0
        assert (np.abs(d2[done].astype(np.float64) - FAIL_DIST ** 2) >= 0.01 * FAIL_DIST ** 2).all(), "the script puts no game near the threshold"
        assert dev.step(t) == 0
        out = dev.game_out.t.cpu().numpy()
        assert np.array_equal(_bits(dev.running.t.cpu().numpy()), _bits(ref.running)), f"running values after step {t + 1}"
        assert np.array_equal(_bits(out[:, :4]), _bits(want[:, :4])), f"finished games of step {t + 1}"
        assert np.array_equal(out[:, 4], want[:, 4]), f"causes of step {t + 1}"
        assert np.array_equal(_bits(out[:, 5:7]), _bits(sc["tar"][t][:, :2])), "the target is TrajGenerator.calc_pos in float32"
        assert np.array_equal(_bits(out[:, 7]), _bits(d2))
        seen |= set(want[done, 4].astype(int).tolist())
    if variant == "all_end":
        assert (sc["reset"][6] != 0).all()
    elif E > 1:
        assert sc["reset"][0, 0] == 1 and sc["reset"][:, 1].sum() == 0 and sc["reset"][:, 2].sum() == 2
    assert seen == {ER.TIMEOUT, ER.FAR, ER.FALLEN}
    per_env = dev.totals.t.cpu().numpy()
    for name in ("games", "timeout", "far", "fallen", "min_len", "max_len", "nonfinite_steps", "max_speed2", "max_ang_speed2"):
        assert np.array_equal(per_env[:, ER.K[name]], ref.totals[:, ER.K[name]]), name
    ref_m, scale = ref.moments()
    assert dev.reduce() == 0
    print(f"\n  E = {E} ({variant}): {int(ref_m[0])} games")
    _check_moments(dev.moments.t.cpu().numpy(), ref_m, scale)
    assert dev.intact()


def test_nonfinite_states_are_counted_and_stay_in_their_env():
    E, bad = 70, 37
    sc = make_script(E, 12, "mixed", seed=5)
    planted = {4: (9, 2, np.nan), 9: (20, 8, np.inf)}                 # step -> (body, component, value)
    plain, dev = Device(sc), Device(sc)
    for t in range(sc["T"]):
        rb = None
        if t in planted:
            body, comp, val = planted[t]
            rb = sc["rb"][t].copy()
            rb[bad, body, comp] = val
        assert plain.step(t) == 0 and dev.step(t, rb=rb) == 0
    a, b = plain.totals.t.cpu().numpy(), dev.totals.t.cpu().numpy()
    others = np.arange(E) != bad
    assert np.array_equal(_bits(a[others]), _bits(b[others])) and np.array_equal(_bits(plain.running.t.cpu().numpy()), _bits(dev.running.t.cpu().numpy()))
    assert a[:, ER.K["nonfinite_steps"]].sum() == 0 and b[bad, ER.K["nonfinite_steps"]] == 2 and b[others, ER.K["nonfinite_steps"]].sum() == 0
    assert b[bad, ER.K["max_speed2"]] == np.inf                       # the Inf sat in a linear velocity; the NaN (a position) is no maximum
    assert dev.reduce() == 0
    from emloco_amd.learning.episode_stats import report_from_moments
    assert report_from_moments(dev.moments.t.cpu().numpy())["nonfinite_steps"] == 2


def test_reduce_clears_the_totals_and_keeps_the_games_in_progress():
    E = 70
    sc = make_script(E, 12, "mixed", seed=23)
    dev, ref = Device(sc), ER.EpisodeStatsRef(E, FAIL_DIST, PENALTY)
    for epoch in range(2):
        for t in range(6 * epoch, 6 * epoch + 6):
            _ref_step(ref, sc, t)
            assert dev.step(t) == 0
        running = dev.running.t.clone()
        ref_m, scale = ref.moments()
        assert dev.reduce() == 0
        assert int(ref_m[0]) > 0 and (running[:, 3] > 0).any()
        assert not dev.totals.t.any(), "the epoch totals are zero after the reduce"
        assert torch.equal(running, dev.running.t) and np.array_equal(_bits(running.cpu().numpy()), _bits(ref.running))
        print(f"\n  epoch {epoch + 1}: {int(ref_m[0])} games")
        _check_moments(dev.moments.t.cpu().numpy(), ref_m, scale)     # the second epoch's vector covers its own games only
    assert dev.intact()


def test_causes_agree_with_the_flags_kernel():
    import kernel_refs as R
    import task_cases as TC
    from emloco_amd import _lib as L
    from test_gpu_task_matrix import Scene, _amp0
    hf = R.task_map()
    n_far = n_near = n_done = 0
    for E, seed in TC.POST_CASES:
        s = Scene(R.case_task(E, seed), hf, _amp0(E, seed))
        assert s.launch(TC.POST_STEP) == 0
        b = s.bufs
        running = torch.zeros(E, L.EPISODE_RUNNING, device=DEV)
        totals = torch.zeros(E, L.EPISODE_MOMENTS, dtype=torch.float64, device=DEV)
        out = torch.zeros(E, L.EPISODE_GAME_OUT, device=DEV)
        v = C.c_void_p
        assert _lib().emloco_episode_stats_step(E, v(b.rew_buf), v(b.reward_raw), v(b.reset_buf), v(b.terminate_buf), v(b.progress_buf), v(b.rb_state),
                                                v(b.traj_verts), None, 0.0, b.dt, b.traj_dur, b.fail_dist, v(running.data_ptr()), v(totals.data_ptr()),
                                                v(out.data_ptr()), v(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        got = s.numpy()
        out = out.cpu().numpy()
        done, term = got["reset"] != 0, got["terminate"] != 0
        far = out[:, 7] > np.float32(b.fail_dist) * np.float32(b.fail_dist)
        cause = out[:, 4].astype(int)
        assert (term[far]).all(), "far implies terminate"
        assert np.array_equal(cause != ER.RUNS, done)
        assert np.array_equal(np.isin(cause, (ER.FAR, ER.FALLEN))[done], term[done]) and np.array_equal(cause[done] == ER.FAR, far[done])
        n_far, n_near, n_done = n_far + int(far.sum()), n_near + int((~far).sum()), n_done + int(done.sum())
    assert n_far > 0 and n_near > 0 and n_done > 0


def test_refused_arguments_write_nothing():
    sc = make_script(5, 12, "mixed", seed=3)
    dev = Device(sc, fill=SENT)
    before = [o.buf.clone() for o in (dev.running, dev.totals, dev.game_out, dev.moments)]
    for null in ("rew", "raw", "reset", "term", "progress", "rb", "verts", "running", "totals"):
        assert dev.step(0, null=null) == -1, null
    assert dev.step(0, n_envs=0) == -1 and dev.step(0, n_envs=-3) == -1
    for fd in (0.0, -4.0, float("nan"), float("inf")):
        assert dev.step(0, fail_dist=fd) == -1, fd
    assert dev.reduce(n_envs=0) == -1 and dev.reduce(null="totals") == -1 and dev.reduce(null="moments") == -1
    for o, b in zip((dev.running, dev.totals, dev.game_out, dev.moments), before):
        assert torch.equal(o.buf.view(torch.int32 if o.buf.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


# ---------------------------------------------------------------------------------------------------------------- inside the rollout loop
ENV_FLAGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel", "--input_init_pose", "--input_init_vel"]


def _locoval_run(with_stats, tmp, overlap_reset=False):
    from emloco_amd.learning.episode_stats import EpisodeStats
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    from emloco_amd.run import RLGPUEnv
    from test_gpu_env import _make_env
    E = 64
    env = RLGPUEnv(_make_env(E, ENV_FLAGS))
    task = env.env.task
    g = torch.Generator(device=task.device)
    g.manual_seed(77)
    pool = torch.randn(8, E, 69, device=task.device, generator=g) * 0.3
    k = [0]

    def pol(obs):
        k[0] += 1
        return pool[k[0] % 8]
    pol.reads_obs = not overlap_reset                            # (a policy that leaves the reset chain beside the step, as bench.py's)
    torch.manual_seed(5)
    agent = LocoValRollout(env, horizon_length=16, policy=pol, overlap_reset=overlap_reset, warmup_epochs=5, max_epochs=40)
    assert bool(task.overlap_reset) == overlap_reset
    out = dict(agent=agent, env=env, reports=[], flags=torch.zeros((), dtype=torch.int64, device=task.device))
    if with_stats:
        stats = EpisodeStats(task, inverted_penalty=agent.inversion_penalty_scale)
        step = stats.step

        def hooked():                                            # the test's hook: this step's reset flags, counted on the device
            out["flags"] += (task.reset_buf != 0).sum()
            step()
        stats.step = hooked
        agent.attach_episode_stats(stats)
        fit, sums = agent._fit_launches, torch.zeros(4, dtype=torch.float64, device=task.device)

        def fit_hooked(st, stage=None):                          # the test's second hook: the fitted episodes' outputs and targets, in float64
            fit(st, stage)
            z = dict(agent._fz, **(stage or {}))
            on = z["weight"] > 0
            for i, x in enumerate((z["value"], z["target"])):
                x = torch.where(on, x, torch.zeros_like(x)).double()
                sums[i] += x.sum()
                sums[2 + i] += x.abs().sum()
        agent._fit_launches = fit_hooked
        out["fit_sums"] = []
    for _ in range(2):
        for _ in range(agent.horizon_length):
            agent.step_once()
        agent.end_epoch()
        if with_stats:
            out["reports"].append(agent.epoch_report())
            out["fit_sums"].append(sums.cpu().numpy().copy())
            sums.zero_()
    agent._sync_fit()
    torch.cuda.synchronize()
    out["params"] = torch.cat([p.detach().reshape(-1) for p in agent.valuenet.parameters()]).clone()
    if with_stats:
        agent.attach_episode_stats(None)
        mof = os.path.join(tmp, "exp")
        out.update(mof=mof, net_path=agent.save(mof), state_path=agent.save_state(mof))
    agent.detach()
    return out


@pytest.fixture(scope="module")
def locoval_runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("episode_stats"))
    return _locoval_run(True, tmp), _locoval_run(False, tmp)


def test_locoval_loop_is_unchanged_by_the_statistics(locoval_runs):
    on, off = locoval_runs
    assert torch.equal(on["params"], off["params"]), "the LocoVal parameters with and without the statistics"
    assert on["agent"].fitted_episodes == off["agent"].fitted_episodes and on["agent"].epoch_num == off["agent"].epoch_num == 2
    games = sum(rep["games"] for rep, own in on["reports"])
    print("\n  reports:", on["reports"])
    assert games == int(on["flags"].item()) and games > 0
    for rep, own in on["reports"]:
        assert rep["nonfinite_steps"] == 0 and np.isfinite(rep["max_speed"]) and rep["max_speed"] > 0
        if rep["games"]:
            assert abs(rep["timeout"] + rep["far"] + rep["fallen"] - 1.0) < 1e-12 and 1 <= rep["len_min"] <= rep["len_mean"] <= rep["len_max"]
    assert sum(own["fitted_episodes"] for rep, own in on["reports"]) == on["agent"].fitted_episodes
    # vnet_pred / combine_rwd are the means over the epoch's fitted episodes: float32 dot products of at most 64 terms per fit against
    # the hook's float64 sums, 64 x 2^-24 of the sum of |terms|
    for (rep, own), sums in zip(on["reports"], on["fit_sums"]):
        n = own["fitted_episodes"]
        assert n > 0 and np.isfinite(own["vnet_loss"]) and own["vnet_loss"] > 0
        assert abs(own["vnet_pred"] * n - sums[0]) <= 64 * 2.0 ** -24 * sums[2] and abs(own["combine_rwd"] * n - sums[1]) <= 64 * 2.0 ** -24 * sums[3]


def test_statistics_with_the_reset_chain_on_a_second_stream(locoval_runs, tmp_path):
    """overlap_reset: reset_done() forks the reset chain from the caller's stream by an event recorded behind the statistics launch, so
    the launch sees every finished env before it is reset -- the reports are those of the one-stream schedule, same seeds, and the
    network is the one the schedule fits without the statistics"""
    seq, _ = locoval_runs
    on, off = _locoval_run(True, str(tmp_path), overlap_reset=True), _locoval_run(False, str(tmp_path), overlap_reset=True)
    assert torch.equal(on["params"], off["params"])
    games = sum(rep["games"] for rep, own in on["reports"])
    assert games == int(on["flags"].item()) > 0
    assert [rep for rep, own in on["reports"]] == [rep for rep, own in seq["reports"]]


def test_locoval_checkpoint_restores_the_training_state(locoval_runs):
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    on, _ = locoval_runs
    a = on["agent"]
    assert os.path.basename(on["net_path"]) == "exp_valuenet.pth" and os.path.basename(on["state_path"]) == "exp_valuenet_state.pth"
    net = ValuePoseNet(use_pose=True, use_vel=True)
    net.load_state_dict(torch.load(on["net_path"]))                      # a plain state_dict, loaded unaided
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in net.parameters()]), on["params"].cpu())
    b = LocoValRollout(on["env"], horizon_length=16, overlap_reset=False, warmup_epochs=5, max_epochs=40)
    assert not torch.equal(torch.cat([p.detach().reshape(-1) for p in b.valuenet.parameters()]), on["params"])
    b.restore_state(on["mof"])
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in b.valuenet.parameters()]), on["params"])
    assert a.fitted_episodes > 0 and a._fz["m"].abs().sum() > 0
    assert torch.equal(a._fz["m"], b._fz["m"]) and torch.equal(a._fz["v"], b._fz["v"])
    assert torch.equal(a._fz["steps"][a._flip], b._fz["steps"][b._flip]) and float(b._fz["steps"][b._flip]) == a.vnet_fits
    lr = 1e-5 + 2 * (1e-3 - 1e-5) / 4                                     # two epochs into a warm-up of five (scheduler.py)
    assert a.vnet_optimizer.param_groups[0]["lr"] == b.vnet_optimizer.param_groups[0]["lr"] and abs(a.vnet_optimizer.param_groups[0]["lr"] - lr) < 1e-12
    assert a.vnet_scheduler.last_epoch == b.vnet_scheduler.last_epoch and (a.epoch_num, a.frames) == (b.epoch_num, b.frames) == (2, 2 * 16 * 64)
    assert torch.equal(a._stats, b._stats)
    b.detach()


# ---------------------------------------------------------------------------------------------------------------- through the entry point
def test_entry_point_trains_checkpoints_and_resumes(tmp_path, capsys):
    """`python -m emloco_amd.run --experiment ...` in process: two epochs of the LocoVal fit at 64 envs, then --resume for a third"""
    from emloco_amd import run
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    import json
    argv = ["--num_envs", "64", "--seed", "3", *ENV_FLAGS, "--experiment", "e2e", "--network_path", str(tmp_path), "--save_freq", "1"]
    run.main(argv + ["--max_iterations", "2"])
    said = capsys.readouterr().out.splitlines()
    eps = [ln for ln in said if ln.startswith("Ep: ")]
    assert len(eps) == 2 and eps[1].startswith("Ep: 2\trwd: ") and eps[1].endswith(tuple("0123456789"))
    assert [f.split(":")[0].strip() for f in eps[0].split("\t")] == ["Ep", "rwd", "vnet_pred", "combine_rwd", "vnet_loss", "fps_step", "fps_total",
                                                                      "ep_time", "frame", "eps_len"]
    assert "\tframe: 4096\t" in eps[1] and said.count("latest model saved") == 2 and any(ln.startswith("fps_step: ") for ln in said)
    assert sorted(os.listdir(tmp_path)) == ["e2e_log.jsonl", "e2e_valuenet.pth", "e2e_valuenet_state.pth"]
    log = [json.loads(ln) for ln in open(tmp_path / "e2e_log.jsonl")]
    assert [(r["epoch"], r["frame"]) for r in log] == [(1, 2048), (2, 4096)]
    assert all({"games", "vnet_pred", "combine_rwd", "vnet_loss", "fps_step", "ep_time", "wall_time", "fitted_episodes"} <= set(r) for r in log)
    assert sum(r["games"]["games"] for r in log) > 0 and all(r["games"]["nonfinite_steps"] == 0 for r in log)
    ValuePoseNet(use_pose=True, use_vel=True).load_state_dict(torch.load(tmp_path / "e2e_valuenet.pth"))
    state = torch.load(tmp_path / "e2e_valuenet_state.pth")
    assert (state["epoch"], state["frame"]) == (2, 4096) and float(state["adamw_step"]) == float(state["stats"][4]) > 0
    run.main(argv + ["--max_iterations", "3", "--resume"])
    said = capsys.readouterr().out.splitlines()
    assert any(ln.startswith("resumed ") and "epoch 2" in ln for ln in said)
    assert [ln.split("\t")[0] for ln in said if ln.startswith("Ep: ")] == ["Ep: 3"]
    log = [json.loads(ln) for ln in open(tmp_path / "e2e_log.jsonl")]
    assert [(r["epoch"], r["frame"]) for r in log] == [(1, 2048), (2, 4096), (3, 6144)]
    state3 = torch.load(tmp_path / "e2e_valuenet_state.pth")
    assert state3["epoch"] == 3 and float(state3["adamw_step"]) > float(state["adamw_step"])       # the optimiser's count carried on
    assert state3["scheduler"]["last_epoch"] == state["scheduler"]["last_epoch"] + 1


def test_policy_trainer_under_the_driver(tmp_path):
    """PPO + AMP at toy size under run_training with the statistics on: the games it reports are the reset flags of its rollout"""
    import json
    import yaml
    from emloco_amd import run
    from emloco_amd.learning.amp_agent import AMPAgent
    from emloco_amd.learning.amp_policy import DEFAULT_CFG
    from emloco_amd.learning.episode_stats import EpisodeStats
    from test_gpu_env import _make_env
    env = run.RLGPUEnv(_make_env(64, ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]))
    task = env.env.task
    cfg = yaml.safe_load(open(DEFAULT_CFG))
    cfg["params"]["network"]["mlp"]["units"] = [256, 128]
    cfg["params"]["network"]["disc"]["units"] = [128, 64]
    cfg["params"]["config"].update(horizon_length=16, minibatch_size=128, amp_minibatch_size=128, amp_batch_size=64,
                                   amp_obs_demo_buffer_size=512, amp_replay_buffer_size=512, mini_epochs=1)
    agent = AMPAgent(env, cfg)
    stats = EpisodeStats(task)
    flags = torch.zeros((), dtype=torch.int64, device=task.device)
    step = stats.step

    def hooked():
        nonlocal flags
        flags += (task.reset_buf != 0).sum()
        step()
    stats.step = hooked
    said = []
    opt = run.train_options(["--experiment", "pol", "--network_path", str(tmp_path), "--max_iterations", "3", "--save_freq", "2"])
    assert run.run_training(run.PolicyTrainee(agent, stats=stats), opt, said.append) == 3
    eps = [ln for ln in said if ln.startswith("Ep: ")]
    assert len(eps) == 3 and [f.split(":")[0].split(" ")[0] for f in eps[2].split("\t")] == ["Ep", "rwd", "fps_step", "fps_total", "ep_time", "frame",
                                                                                             "eps_len", "a_loss"]
    assert "\tframe: 3072\t" in eps[2]
    assert sorted(os.listdir(tmp_path)) == ["pol.pth", "pol_log.jsonl"]
    log = [json.loads(ln) for ln in open(tmp_path / "pol_log.jsonl")]
    assert [r["epoch"] for r in log] == [1, 2, 3] and sum(r["games"]["games"] for r in log) == int(flags.item()) > 0
    ck = torch.load(tmp_path / "pol.pth")
    assert (ck["epoch"], ck["frame"]) == (3, 3072) and "optimizer" in ck
    fresh = AMPAgent(env, cfg)
    run.PolicyTrainee(fresh).resume(str(tmp_path / "pol"))
    assert (fresh.epoch_num, fresh.frame) == (3, 3072) and fresh.episode_stats is None

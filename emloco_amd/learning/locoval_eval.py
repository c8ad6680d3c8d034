"""LocoVal evaluation: the `--test` player of the reference, batched on the device.

Mirror of pacer/pacer/learning/amp_value_players.py:35-272 (AMPPlayerContinuousValue.run, the `plot_val_reward: True` branch of
the shipped player config): the frozen policy plays deterministically; for every game the loop records the discounted return up
to `step_to_pred` and its locomotion / power / style parts, what LocoVal predicted for the game's start, the squared error of
that prediction against the normalised return, the return at the end and the game's length; at the end it prints the averages,
the (population) standard deviations and the Pearson correlations of prediction against return.

The reference plays one env at a time and reads the device every step.  Here every env of the batch plays its own games one after
another with the semantics of the reference's single-env game, and the bookkeeping is three HIP launches per step
(include/emloco_predictor.h: emloco_locoval_eval_step -> emloco_locoval_fwd_rows -> emloco_locoval_eval_finish).  Each env records
exactly its first G = ceil(games_num / E_total) games -- stopping at the first `games_num` finished games would over-sample short
games -- into a slot of its own (records[env][game]: fixed order, deterministic), keeps stepping once its quota is met, and records
nothing more.  The host reads one device counter (envs whose quota is met) every `poll_every` steps and nothing else until the end,
when one launch reduces the records to a moment vector (in double, fixed order); ranks all-reduce that vector once, and
`report_from_moments` turns it into the reference's numbers and printed lines.

Several networks (a list for `valuenet`; `run.py --compare_valuenet`): the games are played once and every network is scored on exactly
those games.  What the bookkeeping keeps per game does not depend on the network, so the step is still three launches
(emloco_locoval_eval_step -> emloco_locoval_eval_fwd_multi -> emloco_locoval_eval_finish_multi: the staged inputs are normalised once
per row and every network of the table evaluated on them, each game recorded once per network), the records are N planes that differ
in `value` and `sq_err` alone and equal bit for bit what N single-network runs on the same games record, and `paired_from_records`
compares the networks game by game.

Path tracking (`track=True`; `run.py --eval_tracks`): one more launch per step between the first and the last of the three
(emloco_locoval_eval_track, once per step however many networks) records per game how far the root was from the path's target -- at
every step and at the predictor's frames, every `round(sample_dt / dt)` steps: an ADE / FDE of the walk against the path -- how far it
walked, and the walked and target xy at those frames in the origin-relative frame of the LocoVal inputs.  The reference's player keeps
`real_traj` / `ideal_traj` for its video (amp_value_players.py:105,126,239) and computes no number from them: these metrics are this
project's.  Their moments are reduced and all-reduced on their own (`track_moments_from_records` / `tracking_from_moments`); the report
gains a `tracking` block, nothing else in it changes, and without `track` there is no launch, no buffer and no block.

Crowd contacts (`crowd=True`; `run.py --eval_crowd`): on a configuration with groups the crowd contact audit (emloco_amd/crowd_contacts.py)
rides in the same place -- its geometry and bookkeeping launches once per step between the first and the last of the three, whatever
the number of networks, on this step's `done` flags and the games' slots.  Members whose quota is met keep walking and keep counting
as neighbours; they write no record.  The report gains a `crowd` block; without `crowd` there is no launch, no buffer and no block.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import dist as D

# EmlocoLocoValRecord (include/emloco_predictor.h), 48 bytes
RECORD_DTYPE = np.dtype({"names": ["disc_to_pred", "value", "cr_to_pred", "loc_to_pred", "pow_to_pred", "norm", "sq_err", "cr_end",
                                   "steps", "terminated", "inverted"],
                         "formats": ["<f8"] + ["<f4"] * 7 + ["<i4"] * 3,
                         "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44], "itemsize": 48})
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
# the moment vector of emloco_locoval_eval_reduce (EMLOCO_EVAL_MOMENTS doubles)
MOMENT_NAMES = ("games", "sum_v", "sum_v2",
                "sum_total", "sum_total2", "sum_v_total", "sum_loc", "sum_loc2", "sum_v_loc",
                "sum_pow", "sum_pow2", "sum_v_pow", "sum_disc", "sum_disc2", "sum_v_disc",
                "sum_sq_err", "sum_cr_end", "sum_steps", "terminated", "inverted")
PARTS = ("total", "loc", "pow", "disc")
_Y_FIELD = {"total": "cr_to_pred", "loc": "loc_to_pred", "pow": "pow_to_pred", "disc": "disc_to_pred"}


def moments_from_records(rec):
    """The moment vector of a structured array of records (RECORD_DTYPE), in float64, summed in record order -- what
    emloco_locoval_eval_reduce computes on the device (there in a fixed tree order)."""
    m = np.zeros(len(MOMENT_NAMES), np.float64)
    v = rec["value"].astype(np.float64)
    m[0] = len(rec)
    m[1], m[2] = float(np.add.reduce(v)), float(np.add.reduce(v * v))
    for k, part in enumerate(PARTS):
        y = rec[_Y_FIELD[part]].astype(np.float64)
        m[3 + 3 * k], m[4 + 3 * k], m[5 + 3 * k] = float(np.add.reduce(y)), float(np.add.reduce(y * y)), float(np.add.reduce(v * y))
    m[15] = float(np.add.reduce(rec["sq_err"].astype(np.float64)))
    m[16] = float(np.add.reduce(rec["cr_end"].astype(np.float64)))
    m[17] = float(np.add.reduce(rec["steps"].astype(np.float64)))
    m[18] = float(np.count_nonzero(rec["terminated"]))
    m[19] = float(np.count_nonzero(rec["inverted"]))
    return m


def _std(n, s, s2):
    """numpy's population std from the sums (amp_value_players.py:260: np.std, ddof 0)."""
    var = (s2 - s * s / n) / n
    return math.sqrt(max(var, 0.0))


def _corr(n, sv, sv2, sy, sy2, svy):
    """np.corrcoef(v, y)[0, 1] from the sums (NaN where a variance is zero, as numpy returns it)."""
    cov = n * svy - sv * sy
    den = (n * sv2 - sv * sv) * (n * sy2 - sy * sy)
    if not den > 0.0:
        return float("nan")
    return max(-1.0, min(1.0, cov / math.sqrt(den)))


def report_from_moments(m):
    """The reference's summary (amp_value_players.py:256,258,260,268-271, same formats) from a moment vector: a dict of the numbers
    and `lines`, the lines the reference prints (the Correlation line carries the reference's embedded newline)."""
    m = [float(x) for x in m]
    n = m[0]
    if n < 1:
        return {"games": 0, "lines": ["no game finished"]}
    r = {"games": int(round(n))}
    r["av_reward"], r["av_steps"], r["av_value_loss"] = m[16] / n, m[17] / n, m[15] / n
    r["av_value"] = m[1] / n
    r["std_value"] = _std(n, m[1], m[2])
    for k, part in enumerate(PARTS):
        s, s2, svy = m[3 + 3 * k], m[4 + 3 * k], m[5 + 3 * k]
        r["av_" + part] = s / n
        r["std_" + part] = _std(n, s, s2)
        r["corr_" + part] = _corr(n, m[1], m[2], s, s2, svy)
    r["terminated"], r["inverted"] = int(round(m[18])), int(round(m[19]))
    r["lines"] = [
        f"av reward: {r['av_reward']:.3f}, av steps: {r['av_steps']:.3f}, av value loss: {r['av_value_loss']:.3f}",
        f"av_loc: {r['av_loc']:.2f}, av_pow: {r['av_pow']:.2f}, av_disc: {r['av_disc']:.2f}, av_total: {r['av_total']:.2f}",
        f"std_loc: {r['std_loc']:.2f}, std_pow: {r['std_pow']:.2f}, std_disc: {r['std_disc']:.2f}, std_total: {r['std_total']:.2f}",
        f"Correlation: \n Total reward: {r['corr_total']:.3f}",
        f"Loc reward: {r['corr_loc']:.3f}",
        f"Pow reward: {r['corr_pow']:.3f}",
        f"Disc reward: {r['corr_disc']:.3f}",
    ]
    return r


SHARED_FIELDS = tuple(k for k in RECORD_DTYPE.names if k not in ("value", "sq_err"))      # the same in every network's plane


def paired_from_records(recs):
    """The comparison of N networks scored on the same games, in float64 from their record arrays (one per network, the same games
    in the same order): per network the MSE (mean of `sq_err`) and Pearson r of `value` against the return up to step_to_pred, and
    for each pair a < b the differences b - a.  The games count is the same for every network by construction; a difference in it
    or in any shared column is an error."""
    n = len(recs[0])
    for r in recs[1:]:
        assert len(r) == n, "the networks of one evaluation record the same games"
        for k in SHARED_FIELDS:
            assert np.array_equal(r[k], recs[0][k]), f"record column {k} differs between networks scored on the same games"
    mse, corr = [], []
    for r in recs:
        v, y = r["value"].astype(np.float64), r["cr_to_pred"].astype(np.float64)
        mse.append(float(np.mean(r["sq_err"].astype(np.float64))) if n else float("nan"))
        ok = n > 1 and v.std() > 0 and y.std() > 0
        corr.append(float(np.corrcoef(v, y)[0, 1]) if ok else float("nan"))
    pairs = [dict(a=a, b=b, d_mse=mse[b] - mse[a], d_corr_total=corr[b] - corr[a]) for a in range(len(recs)) for b in range(a + 1, len(recs))]
    return dict(games=int(n), mse=mse, corr_total=corr, pairs=pairs)


# EmlocoLocoValTrackRecord (include/emloco_predictor.h), 32 bytes
TRACK_DTYPE = np.dtype({"names": ["ade", "fde", "mean_dev", "max_dev", "final_dev", "path_len", "n_samples"],
                        "formats": ["<f4"] * 6 + ["<i4"], "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 32})
TRACK_WORDS = TRACK_DTYPE.itemsize // 4
TRACK_SAMPLES = 16          # EMLOCO_TRACK_SAMPLES
FAIL_DIST = 4.0             # humanoid_traj.py: the distance from the target at which the task ends a game
# the moment vector of emloco_locoval_track_reduce (EMLOCO_TRACK_MOMENTS doubles)
TRACK_MOMENT_NAMES = ("games", "games_sampled", "sum_ade", "sum_ade2", "sum_fde", "sum_fde2", "sum_mean_dev", "sum_mean_dev2",
                      "sum_final_dev", "sum_path_len", "sum_samples", "failed")


class TrackRefusal(ValueError):
    """The path tracking cannot sample this task at the path's own frames (`track_stride`)."""


def track_stride(sample_dt, dt, episode_length):
    """Control steps between two sample instants, round(sample_dt / dt); a TrackRefusal (a ValueError) where the frames of the predictor do
    not fall on control steps or a full game has more of them than a game's EMLOCO_TRACK_SAMPLES slots."""
    sample_dt, dt = float(sample_dt), float(dt)
    if not (dt > 0.0 and sample_dt > 0.0):
        raise TrackRefusal(f"path tracking: sample_dt {sample_dt} and dt {dt} must be positive")
    stride = int(round(sample_dt / dt))
    if stride < 1 or abs(stride * dt - sample_dt) > 1e-6:
        raise TrackRefusal(f"path tracking: the sample interval {sample_dt} s is no whole number of control steps of {dt} s "
                         f"({stride} steps are {stride * dt} s): the walk cannot be sampled at the path's own frames")
    if -(-int(episode_length) // stride) > TRACK_SAMPLES:
        raise TrackRefusal(f"path tracking: a game of {int(episode_length)} steps has {-(-int(episode_length) // stride)} sample instants "
                         f"{stride} steps apart, a game's record holds {TRACK_SAMPLES}")
    return stride


def track_moments_from_records(rec, fail_dist=FAIL_DIST):
    """The moment vector of a structured array of track records (the TRACK_DTYPE columns), in float64, summed in record order -- what
    emloco_locoval_track_reduce computes on the device (there in a fixed tree order).  Sums only: the moments of two shards add up to
    the moments of their union."""
    m = np.zeros(len(TRACK_MOMENT_NAMES), np.float64)
    col = lambda k, sel=slice(None): rec[k][sel].astype(np.float64)
    sampled = rec["n_samples"] > 0
    m[0], m[1] = len(rec), int(np.count_nonzero(sampled))
    for i, k in ((2, "ade"), (4, "fde")):
        y = col(k, sampled)
        m[i], m[i + 1] = float(np.add.reduce(y)), float(np.add.reduce(y * y))
    y = col("mean_dev")
    m[6], m[7] = float(np.add.reduce(y)), float(np.add.reduce(y * y))
    m[8], m[9], m[10] = float(np.add.reduce(col("final_dev"))), float(np.add.reduce(col("path_len"))), float(np.add.reduce(col("n_samples")))
    m[11] = float(np.count_nonzero(rec["max_dev"] > np.float32(fail_dist)))
    return m


def tracking_from_moments(m):
    """The `tracking` block of the report from a track moment vector: a dict of the numbers and `lines`.  ade / fde are averaged over the
    games that reached a sample instant (`games_sampled`), everything else over all games.  The moments hold no sum of final_dev^2:
    `std_final_dev` is not in this block; the evaluator's report takes it, like the correlations, from `tracking_from_records`."""
    m = [float(x) for x in m]
    n, ns = m[0], m[1]
    if n < 1:
        return {"games": 0, "lines": ["tracking: no game finished"]}
    nan = float("nan")
    r = {"games": int(round(n)), "games_sampled": int(round(ns))}
    r["av_ade"], r["std_ade"] = (m[2] / ns, _std(ns, m[2], m[3])) if ns >= 1 else (nan, nan)
    r["av_fde"], r["std_fde"] = (m[4] / ns, _std(ns, m[4], m[5])) if ns >= 1 else (nan, nan)
    r["av_mean_dev"], r["std_mean_dev"] = m[6] / n, _std(n, m[6], m[7])
    r["av_final_dev"], r["av_path_len"], r["av_samples"] = m[8] / n, m[9] / n, m[10] / n
    r["failed"], r["fail_share"] = int(round(m[11])), m[11] / n
    r["lines"] = [
        f"tracking: {r['games']} games, {r['games_sampled']} with a sample instant, av samples: {r['av_samples']:.2f}",
        f"av_ade: {r['av_ade']:.3f}, std_ade: {r['std_ade']:.3f}, av_fde: {r['av_fde']:.3f}, std_fde: {r['std_fde']:.3f}",
        f"av_mean_dev: {r['av_mean_dev']:.3f}, std_mean_dev: {r['std_mean_dev']:.3f}, av_final_dev: {r['av_final_dev']:.3f}, "
        f"av_path_len: {r['av_path_len']:.3f}, beyond fail_dist: {100.0 * r['fail_share']:.1f} %",
    ]
    return r


def tracking_from_records(values, track):
    """What the moments do not carry, in float64 from the gathered records (as `paired_from_records`): the std of final_dev, and per
    network (`values`: one array per network, the games of `track` in its order) Pearson r of `value` against ade and fde over the games
    that reached a sample instant -- whether LocoVal predicts how well the path is tracked.  NaN where a variance is zero."""
    sel = track["n_samples"] > 0
    out = {"std_final_dev": float(np.std(track["final_dev"].astype(np.float64))) if len(track) else float("nan"),
           "corr_value_ade": [], "corr_value_fde": []}
    for v in values:
        v = np.asarray(v)[sel].astype(np.float64)
        for k in ("ade", "fde"):
            y = track[k][sel].astype(np.float64)
            ok = len(v) > 1 and v.std() > 0 and y.std() > 0
            out["corr_value_" + k].append(float(np.corrcoef(v, y)[0, 1]) if ok else float("nan"))
    return out


# The per-env buffers of EmlocoLocoValEval and EmlocoLocoValTrack (include/emloco_predictor.h) under the structs' own field names:
# (name, dtype, shape after the env axis).  All start at zero but `coef`, a game's discount, which starts at one; EmlocoLocoValEval also
# holds `n_full`, the one int32 counter the host polls.
EVAL_BUFFERS = (("coef", "float64", ()), ("c_disc", "float64", ()), ("tp_disc", "float64", ()), ("cr", "float32", ()),
                ("c_loc", "float32", ()), ("c_pow", "float32", ()), ("tp_cr", "float32", ()), ("tp_loc", "float32", ()),
                ("tp_pow", "float32", ()), ("steps", "int32", ()), ("games", "int32", ()), ("done", "uint8", ()),
                ("terminated", "uint8", ()), ("inverted", "uint8", ()), ("traj13", "float32", (13, 3)), ("pose", "float32", (24, 3)),
                ("vel", "float32", (2,)), ("row_mask", "float32", ()))
EVAL_INPUTS = (("waypoint_traj", (15, 3)), ("init_pose", (24, 3)), ("init_vel", (2,)))      # the task's float32 tensors the step reads by address
TRACK_BUFFERS = (("sum_dev", "float64", ()), ("sum_sample_dev", "float64", ()), ("path_len", "float64", ()), ("max_dev", "float32", ()),
                 ("prev_xy", "float32", (2,)), ("last_sample_dev", "float32", ()), ("n_samples", "int32", ()), ("dev_now", "float32", ()))


def eval_state(n_env, step_to_pred, games_per_env, gamma, inputs, zeros, ptr):
    """(EmlocoLocoValEval, {field: buffer}): the game state of `n_env` envs at the start of an evaluation.  inputs: {name: array} for
    EVAL_INPUTS; zeros(shape, dtype name) allocates a zeroed array and ptr(array) gives its address (torch on the device here; the
    tests run the same state on host arrays)."""
    from .._lib import LocoValEval
    b = {k: zeros((n_env, *shape), dt) for k, dt, shape in EVAL_BUFFERS}
    b["coef"] += 1
    b["n_full"] = zeros((1,), "int32")
    s = LocoValEval(n_env=n_env, step_to_pred=step_to_pred, games_per_env=games_per_env, gamma=gamma,
                    **{k: ptr(v) for k, v in b.items()}, **{k: ptr(inputs[k]) for k, _ in EVAL_INPUTS})
    return s, b


def track_state(n_env, zeros, ptr, **scalars):
    """(EmlocoLocoValTrack, {field: buffer}) beside `eval_state`; scalars: the struct's own (stride, root_stride, dt, traj_dur)."""
    from .._lib import LocoValTrack
    tb = {k: zeros((n_env, *shape), dt) for k, dt, shape in TRACK_BUFFERS}
    return LocoValTrack(**scalars, **{k: ptr(v) for k, v in tb.items()}), tb


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class LocoValEvaluator:
    """Plays `games_num` games (all ranks together) of a frozen policy and scores a LocoVal network on them.

    vec_env: the RLGPUEnv / VecTaskPythonWrapper of the task (this rank's shard of the envs).
    policy_bundle: an AMPPolicyBundle (the deterministic action of its FrozenPolicy, the style reward of its FrozenDisc), or a
      callable obs -> actions (then `disc_reward`, a callable amp_obs -> (E,), or None for a style reward of 0).
    valuenet: a ValuePoseNet on the task's device (the fused HIP forward evaluates it), or a list of 1 .. EVAL_MAX_NETS of them (any
      variants): all are scored on the same games, and `report` / `records` answer per network.
    max_steps: the step cap of the reference's player (rl_games BasePlayer: 27 000); a run whose games never finish stops there and
      the report states the shortfall.
    track: also record per game how closely the root followed its path (module docstring): `report` gains a `tracking` block,
      `track_records` / `track_samples` answer per game.
    crowd: also audit per game how close the env came to the other members of its group (crowd_contacts.CrowdContactAudit, `near_dist`
      = crowd_near_dist): `report` gains a `crowd` block, `crowd_records` answers per game.  A task without groups or without a
      capsule table is a CrowdContactRefusal (a ValueError) before anything is allocated."""

    def __init__(self, vec_env, policy_bundle, valuenet, games_num, max_steps=27000, poll_every=16, gamma=0.99, disc_reward=None,
                 track=False, crowd=False, crowd_near_dist=1.0):
        from ..predictor import ops
        from .value_pose_net import ValuePoseNet
        self.vec_env = vec_env
        env = vec_env.env if hasattr(vec_env, "env") else vec_env
        self.env, self.task = env, env.task
        task = self.task
        self.flight_recorder = None               # learning/flight_recorder.py: a bound FlightRecorder, set by the driver (--capture)
        self.track = bool(track)
        if self.track:                            # refused by name before anything is allocated
            self.track_stride = track_stride(task._traj_sample_timestep, task.dt, task.max_episode_length)
            self.fail_dist = float(getattr(task, "_fail_dist", FAIL_DIST))
        self.crowd = None
        if crowd:                                 # refused by name before anything is allocated
            from ..crowd_contacts import CrowdContactRefusal
            if not getattr(task, "_divide_group", False):
                raise CrowdContactRefusal("LocoValEvaluator(crowd=True): the task has divide_group: False -- without groups there is "
                                          "nobody to measure against")
        self.device = torch.device(task.device)
        self.multi = isinstance(valuenet, (list, tuple))
        nets = list(valuenet) if self.multi else [valuenet]
        if self.multi and not 1 <= len(nets) <= ops.EVAL_MAX_NETS:
            raise ValueError(f"LocoValEvaluator: {len(nets)} networks; one evaluation scores 1 to {ops.EVAL_MAX_NETS}")
        if self.device.type != "cuda" or not all(isinstance(n, ValuePoseNet) for n in nets):
            raise RuntimeError("LocoValEvaluator runs its bookkeeping and the LocoVal forward as HIP kernels: it needs a gfx950 device, "
                               "libemloco_hip.so and the HIP ValuePoseNet (there is no CPU path in the product)")
        for flag in ("fused_chain", "overlap_obs", "overlap_reset"):
            if getattr(task, flag, False):        # the loop reads the inputs the task captured at reset right after env.step
                raise RuntimeError(f"LocoValEvaluator: task.{flag} is set (a loop that left it on must detach() first)")
        if hasattr(task, "attach_returns"):
            task.attach_returns(None)             # no training bookkeeping rides in the task's flags launch here
        if getattr(task, "amp_ring", False):
            task.enable_amp_ring(False)
        if int(games_num) < 1:
            raise ValueError("games_num must be at least 1")
        self.valuenets, self.valuenet = nets, nets[0]
        if hasattr(policy_bundle, "frozen"):
            bundle = policy_bundle
            self.policy = lambda obs: bundle.frozen.act(obs, deterministic=True, generator=bundle.generator)
            self.disc_reward = disc_reward or bundle.disc_reward
        else:
            self.policy, self.disc_reward = policy_bundle, disc_reward
        E = task.num_envs
        self.num_envs = E
        self.games_num = int(games_num)
        e_total = torch.tensor([E], dtype=torch.float64, device=self.device)
        D.all_reduce_(e_total)
        self.envs_total = int(e_total.item())
        self.games_per_env = G = -(-self.games_num // self.envs_total)
        self.max_steps, self.poll_every, self.gamma = int(max_steps), max(1, int(poll_every)), float(gamma)
        self.step_to_pred = int(task.step_to_pred)
        dev = self.device
        f = lambda *s: torch.zeros(*s, device=dev)
        zeros = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device=dev)
        self._inputs = tuple(k for k, _ in EVAL_INPUTS)
        self._s, self._b = eval_state(E, self.step_to_pred, G, self.gamma, {k: self._input(k) for k in self._inputs}, zeros,
                                      torch.Tensor.data_ptr)
        # the forward's persistent output (a game's prediction stays in its row until the game is recorded) and its scratch rows
        N = len(nets)
        if self.multi:          # a value plane and a record plane per network: the table of emloco_locoval_eval_fwd_multi / _finish_multi
            self._values = f(N, E)
            self._records = torch.zeros(N * E * G * RECORD_WORDS, dtype=torch.int32, device=dev)
            self._moments = torch.zeros(N, ops.EVAL_MOMENTS, dtype=torch.float64, device=dev)
            self._nets = ops.LocoValNets(n_nets=N)
            self._net_weights = []
            for k, net in enumerate(nets):
                w = self._weights(net)
                self._net_weights.append(w)
                self._nets.net[k] = ops.LocoValNet(net.variant, 0, *[t.data_ptr() for t in w], self._values[k].data_ptr())
        else:
            n_in, n_h1, n_h2, _ = ops.locoval_dims(valuenet.variant)          # the network's input configuration (value_pose_net.py:43-52)
            self._value, self._x100, self._h1, self._h2, self._ang = f(E), f(E, n_in), f(E, n_h1), f(E, n_h2), f(E)
            self._records = torch.zeros(E * G * RECORD_WORDS, dtype=torch.int32, device=dev)
            self._moments = torch.zeros(ops.EVAL_MOMENTS, dtype=torch.float64, device=dev)
        if self.track:
            self._t, self._tb = track_state(E, zeros, torch.Tensor.data_ptr, stride=self.track_stride)
            self._track_records = torch.zeros(E * G * TRACK_WORDS, dtype=torch.int32, device=dev)
            self._track_samples = f(E, G, ops.TRACK_SAMPLES, 4)
            self._track_moments = torch.zeros(ops.TRACK_MOMENTS, dtype=torch.float64, device=dev)
        if crowd:
            from ..crowd_contacts import CrowdContactAudit
            self.crowd = CrowdContactAudit(task, near_dist=crowd_near_dist, games_per_env=G)
        self.steps_run = 0
        self.started = False
        # --pred_path: the host reset knows which row of the predicted-path table every game walks; logged from the first reset on
        tg = getattr(task, "_traj_gen", None)
        self._pred_log = None
        if tg is not None and getattr(tg, "traj_pred_data", None) is not None:
            self._pred_log = tg.pred_row_log = []

    def _input(self, name):
        """The task's LocoVal inputs the kernel reads by address (15 x 3 waypoints, 24 x 3 joints, 2 velocity components per env)."""
        t = getattr(self.task, name)
        want = (self.num_envs, *dict(EVAL_INPUTS)[name])
        if tuple(t.shape) != want or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
            raise RuntimeError(f"LocoValEvaluator: task.{name} must be a contiguous float32 {want} tensor on {self.device}")
        return t

    def _weights(self, net):
        n = net._network
        w = [n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias]
        for t in w:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device
        return w

    def _check_nets(self):
        """The table holds the parameters' addresses: a network whose parameters moved since the evaluator was built is an error."""
        for k, (net, w) in enumerate(zip(self.valuenets, self._net_weights)):
            if any(a is not b for a, b in zip(self._weights(net), w)) or self._nets.net[k].w1 != w[0].data_ptr():
                raise RuntimeError(f"LocoValEvaluator: the parameters of network {k} were replaced after the evaluator took their addresses")

    def _check_inputs(self):
        for k, ptr in zip(self._inputs, (self._s.waypoint_traj, self._s.init_pose, self._s.init_vel)):
            if self._input(k).data_ptr() != ptr:
                raise RuntimeError(f"LocoValEvaluator: the task re-allocated {k} after the evaluator took its address")

    # ------------------------------------------------------------------ one step
    def step_once(self):
        """env_reset(done_indices) -> deterministic action -> env.step -> style reward -> the three launches (:116-204)."""
        task = self.task
        with torch.no_grad():
            if not self.started:
                self.env.reset(torch.arange(self.num_envs, device=self.device))
                self.started = True
            elif hasattr(self.env, "reset_done"):
                self.env.reset_done()
            else:
                self.env.reset(task.reset_buf.nonzero(as_tuple=False).flatten())
            actions = self.policy(task.obs_buf)
            _obs, _rew, dones, infos = self.vec_env.step(actions)
            if self.flight_recorder is not None:
                self.flight_recorder.check()                      # (a bound FlightRecorder, set by the driver: run.py --test --capture)
            disc = None if self.disc_reward is None else self.disc_reward(infos["amp_obs"]).contiguous().float()
            self._launch(task.reward_raw, disc, dones, infos.get("terminate", getattr(task, "_terminate_buf", None)), task.inverted)
        self.steps_run += 1

    def _launch(self, reward_raw, disc, dones, terminate, inverted):
        """The bookkeeping of one step on the current stream (also the entry point of the tests that script the streams)."""
        from ..predictor import ops
        from ..sim import current_stream_handle
        lib = ops._lib()
        st = current_stream_handle(self.device)
        assert reward_raw.dtype == torch.float32 and reward_raw.shape == (self.num_envs, 2) and dones.dtype == torch.int64
        assert terminate is None or terminate.dtype == torch.int64
        if inverted is not None and inverted.dtype == torch.bool:
            inverted = inverted.view(torch.uint8)
        self._check_inputs()
        ops._chk(lib.emloco_locoval_eval_step(C.byref(self._s), _p(reward_raw.contiguous()), _p(disc), _p(dones.contiguous()),
                                              _p(None if terminate is None else terminate.contiguous()),
                                              _p(None if inverted is None else inverted.contiguous()), st), "emloco_locoval_eval_step")
        if self.track:                              # once per step, whatever the number of networks: nothing tracked depends on them
            ops._chk(lib.emloco_locoval_eval_track(C.byref(self._s), C.byref(self._track_inputs()), _p(self._track_records),
                                                   _p(self._track_samples), st), "emloco_locoval_eval_track")
        if self.crowd is not None:                  # likewise: this step's done flags, the slots of the games in progress
            self.crowd.step(done=self._b["done"], slot=self._b["games"])
        if self.multi:
            self._check_nets()
            ops._chk(lib.emloco_locoval_eval_fwd_multi(C.byref(self._s), C.byref(self._nets), st), "emloco_locoval_eval_fwd_multi")
            ops._chk(lib.emloco_locoval_eval_finish_multi(C.byref(self._s), C.byref(self._nets), _p(self._records), st),
                     "emloco_locoval_eval_finish_multi")
            return
        self._forward(st)
        ops._chk(lib.emloco_locoval_eval_finish(C.byref(self._s), _p(self._value), _p(self._records), st), "emloco_locoval_eval_finish")

    def _track_inputs(self):
        """The tracker reads what the task's reward kernel read this step: the addresses and constants of the task's own EmlocoTaskBufs."""
        from .. import _lib as L
        pb = getattr(self.task, "_post_bufs", None)
        if pb is None:
            raise RuntimeError("LocoValEvaluator(track=True): the task has not launched its post-physics kernel yet (no EmlocoTaskBufs)")
        t = self._t
        t.root_pos, t.root_stride, t.traj_verts, t.progress_buf = pb.rb_state, L.NB * 13, pb.traj_verts, pb.progress_buf
        t.dt, t.traj_dur = pb.dt, pb.traj_dur
        return t

    def _forward(self, st):
        """LocoVal on the rows whose game took its first step (:128-134), into the persistent `value` rows."""
        from ..predictor import ops
        b, w = self._b, self._weights(self.valuenet)
        if self.valuenet.variant == ops.LOCOVAL_FULL:
            ops._chk(ops._lib().emloco_locoval_fwd_rows(self.num_envs, _p(b["traj13"]), 3, _p(b["pose"]), _p(b["vel"]), *[_p(t) for t in w],
                                                        _p(self._value), _p(self._x100), _p(self._h1), _p(self._h2), _p(self._ang), _p(b["row_mask"]),
                                                        st), "emloco_locoval_fwd_rows")
        else:
            ops._chk(ops._lib().emloco_locoval_variant_fwd_rows(self.valuenet.variant, self.num_envs, _p(b["traj13"]), 3, _p(b["pose"]), _p(b["vel"]),
                                                                *[_p(t) for t in w], _p(self._value), _p(self._x100), _p(self._h1), _p(self._h2),
                                                                _p(self._ang), None, _p(b["row_mask"]), st), "emloco_locoval_variant_fwd_rows")

    # ------------------------------------------------------------------ the run
    def envs_full(self):
        """Envs of this rank whose quota is met (a host read)."""
        return int(self._b["n_full"].item())

    def run(self, say=print):
        """Step until every env of this rank has recorded its quota (polled every `poll_every` steps) or `max_steps` is reached; then one
        reduction, one all-reduce of the moment vector (all ranks), the report.  Returns the report dict."""
        while self.steps_run < self.max_steps:
            self.step_once()
            if self.steps_run % self.poll_every == 0 and self.envs_full() == self.num_envs:
                break
        return self.report(say=say)

    def moments(self):
        from ..predictor import ops
        from ..sim import current_stream_handle
        # one reduction per record plane -> [N][EVAL_MOMENTS] (a list of networks) or [EVAL_MOMENTS], and the one collective of the evaluation
        N = len(self.valuenets)
        for rec, mom in zip(self._records.view(N, -1), self._moments.view(N, -1)):
            ops._chk(ops._lib().emloco_locoval_eval_reduce(self.num_envs, self.games_per_env, _p(rec), _p(self._b["games"]), _p(mom),
                                                           current_stream_handle(self.device)), "emloco_locoval_eval_reduce")
        m = self._moments.clone()
        D.all_reduce_(m)
        return m.cpu().numpy()

    def track_moments(self):
        """The track moment vector of all ranks: one reduction, one all-reduce of its own (the moment vector of `moments` is untouched)."""
        from ..predictor import ops
        from ..sim import current_stream_handle
        ops._chk(ops._lib().emloco_locoval_track_reduce(self.num_envs, self.games_per_env, _p(self._track_records), _p(self._b["games"]),
                                                        self.fail_dist, _p(self._track_moments), current_stream_handle(self.device)),
                 "emloco_locoval_track_reduce")
        m = self._track_moments.clone()
        D.all_reduce_(m)
        return m.cpu().numpy()

    def track_records(self):
        """This rank's track records (TRACK_DTYPE columns plus `env` and `game`), in the order of `records`."""
        E, G = self.num_envs, self.games_per_env
        raw = self._track_records.cpu().numpy().view(TRACK_DTYPE).reshape(E, G)
        env, game = self._slots(self._b["games"].cpu().numpy(), G)
        out = np.zeros(len(env), dtype=[(k, TRACK_DTYPE.fields[k][0]) for k in TRACK_DTYPE.names] + [("env", "<i4"), ("game", "<i4")])
        for k in TRACK_DTYPE.names:
            out[k] = raw[k][env, game]
        out["env"], out["game"] = env, game
        return out

    def track_samples(self):
        """(walked, target): [games][TRACK_SAMPLES][2] each, the root's and the target's xy at the sample instants of every recorded game
        (order of `records`) relative to the path's first vertex; rows past the game's n_samples are zero."""
        env, game = self._slots(self._b["games"].cpu().numpy(), self.games_per_env)
        smp = self._track_samples.cpu().numpy()[env, game]
        return np.ascontiguousarray(smp[:, :, 0:2]), np.ascontiguousarray(smp[:, :, 2:4])

    def _tracking(self, values, say):
        """The `tracking` block: the all-reduced moments, and from all ranks' records the Pearson r of every network's value."""
        m = self.track_moments()
        trk = tracking_from_moments(m)
        rec = self.track_records()
        if D.is_distributed():
            parts = [None] * D.world_size()
            torch.distributed.all_gather_object(parts, (values, rec))
            values = [np.concatenate([p[0][k] for p in parts]) for k in range(len(values))]
            rec = np.concatenate([p[1] for p in parts])
        assert trk["games"] == len(rec), "the track records and their moments cover the same games"
        extra = tracking_from_records(values, rec)
        if not self.multi:
            extra["corr_value_ade"], extra["corr_value_fde"] = extra["corr_value_ade"][0], extra["corr_value_fde"][0]
        trk.update(extra, fail_dist=self.fail_dist, stride=self.track_stride, dt=float(self._t.dt), traj_dur=float(self._t.traj_dur),
                   moments=[float(x) for x in m])
        if trk["games"] > 0:
            fmt = lambda c: ", ".join(f"{x:.3f}" for x in (c if self.multi else [c]))
            trk["lines"] = trk["lines"] + [f"Correlation of value with ade: {fmt(trk['corr_value_ade'])}, with fde: {fmt(trk['corr_value_fde'])}"]
        if say is not None:
            for ln in trk["lines"]:
                say(ln)
        return trk

    def crowd_records(self):
        """This rank's crowd contact records (crowd_contacts.RECORD_DTYPE columns plus `env` and `game`), in the order of `records`."""
        return self.crowd.records()

    def _crowd(self, values, say):
        """The `crowd` block: the all-reduced moments, and from all ranks' records the deepest penetration and the Pearson r of every
        network's value against it."""
        from ..crowd_contacts import crowd_from_moments, crowd_from_records
        m = self.crowd.moments()
        blk = crowd_from_moments(m, self.crowd.near_dist, self.crowd.group_size)
        rec = self.crowd_records()
        if D.is_distributed():
            parts = [None] * D.world_size()
            torch.distributed.all_gather_object(parts, (values, rec))
            values = [np.concatenate([p[0][k] for p in parts]) for k in range(len(values))]
            rec = np.concatenate([p[1] for p in parts])
        assert blk["games"] == len(rec), "the crowd records and their moments cover the same games"
        extra = crowd_from_records(values, rec)
        if not self.multi:
            extra["corr_value_max_pen"], extra["corr_value_contact"] = extra["corr_value_max_pen"][0], extra["corr_value_contact"][0]
        blk.update(extra, moments=[float(x) for x in m])
        if blk["games"] > 0:
            fmt = lambda c: ", ".join(f"{x:.3f}" for x in (c if self.multi else [c]))
            blk["lines"] = blk["lines"] + [f"deepest penetration of all games: {blk['max_pen']:.4f}; correlation of value with max_pen: "
                                           f"{fmt(blk['corr_value_max_pen'])}, with a contact: {fmt(blk['corr_value_contact'])}"]
        if say is not None:
            for ln in blk["lines"]:
                say(ln)
        return blk

    def report(self, say=print):
        """One network: the report dict.  A list of networks: {"networks": [the report of each, as a single run of it gives],
        "paired": paired_from_records of all ranks' records}; the lines of every network are said under a `network k` heading.
        With `track` the dict also holds `tracking` (its lines are said last and kept in the block, not in the report's `lines`)."""
        if not self.multi:
            rep = self._report(self.moments(), say)
            if self.track:
                rep["tracking"] = self._tracking([self.records()["value"]], say)
            if self.crowd is not None:
                rep["crowd"] = self._crowd([self.records()["value"]], say)
            return rep
        reps = []
        for k, m in enumerate(self.moments()):
            if say is not None:
                say(f"network {k} (variant {self.valuenets[k].variant}: {self.valuenets[k].layer_sizes[0]} inputs)")
            reps.append(self._report(m, say))
        recs = self.records()
        if D.is_distributed():                      # the paired block covers the games of every rank, as the moments do
            parts = [None] * D.world_size()
            torch.distributed.all_gather_object(parts, recs)
            recs = [np.concatenate([p[k] for p in parts]) for k in range(len(recs))]
        paired = paired_from_records(recs)
        assert all(r["games"] == paired["games"] for r in reps), "every network is scored on the same games"
        if say is not None:
            for pr in paired["pairs"]:
                say(f"network {pr['b']} - network {pr['a']}: MSE {pr['d_mse']:+.6f}, Pearson r (total) {pr['d_corr_total']:+.4f}")
        out = {"networks": reps, "paired": paired}
        if self.track:
            out["tracking"] = self._tracking([r["value"] for r in self.records()], say)
        if self.crowd is not None:
            out["crowd"] = self._crowd([r["value"] for r in self.records()], say)
        return out

    def _report(self, m, say):
        rep = report_from_moments(m)
        full = torch.tensor([float(self.envs_full()), float(self.steps_run)], dtype=torch.float64, device=self.device)
        D.all_reduce_(full)
        expected = self.envs_total * self.games_per_env
        rep.update(games_requested=self.games_num, envs=self.envs_total, games_per_env=self.games_per_env, games_expected=expected,
                   shortfall=expected - rep["games"], steps=self.steps_run, max_steps=self.max_steps, ranks=D.world_size(),
                   moments=[float(x) for x in m])
        head = [f"LocoVal evaluation: {rep['games']} games = {self.envs_total} envs x {self.games_per_env} (the first "
                f"{self.games_per_env} games of every env), {self.steps_run} steps"]
        if expected != self.games_num:
            head.append(f"  games_num {self.games_num} is not a multiple of the {self.envs_total} envs: {expected} games are recorded")
        if rep["shortfall"] > 0:
            head.append(f"  step cap {self.max_steps} reached: {rep['shortfall']} of {expected} games did not finish")
        if rep["games"] > 0:
            head.append(f"  early terminations {rep['terminated']}, inverted paths {rep['inverted']}")
        rep["lines"] = head + rep["lines"]
        if say is not None:
            for ln in rep["lines"]:
                say(ln)
        return rep

    def records(self, net=None):
        """This rank's recorded games as a numpy structured array (RECORD_DTYPE) with `env` and `game` columns, env-major.  With a list
        of networks: the list of their N arrays (the same games in the same order; `value` and `sq_err` are the network's), or the
        array of network `net`."""
        E, G = self.num_envs, self.games_per_env
        if self.multi:
            planes = self._records.cpu().numpy().view(RECORD_DTYPE).reshape(len(self.valuenets), E, G)
            games = self._b["games"].cpu().numpy()
            out = [self._records_of(planes[k], games) for k in (range(len(planes)) if net is None else [net])]
            return out if net is None else out[0]
        assert net in (None, 0)
        return self._records_of(self._records.cpu().numpy().view(RECORD_DTYPE).reshape(E, G), self._b["games"].cpu().numpy())

    def pred_rows(self, records):
        """Under --pred_path: per record the row of the predicted-path table (position in its key order) the game walked -- game g of
        an env follows that env's g-th reset since the evaluation began -- or None when the run walks no predicted paths."""
        if self._pred_log is None:
            return None
        G = self.games_per_env
        table = np.full((self.num_envs, G), -1, np.int64)
        seen = np.zeros(self.num_envs, np.int64)
        for ids, rows in self._pred_log:
            keep = seen[ids] < G
            table[ids[keep], seen[ids[keep]]] = rows[keep]
            seen[ids] += 1
        return table[records["env"], records["game"]]

    @staticmethod
    def _slots(games, G):
        """(env, game) of the recorded slots, env-major."""
        return np.nonzero(np.arange(G)[None, :] < games[:, None])

    @staticmethod
    def _records_of(raw, games):
        G = raw.shape[1]
        env, game = LocoValEvaluator._slots(games, G)
        rec = raw[env, game]
        out = np.zeros(len(rec), dtype=[(k, RECORD_DTYPE.fields[k][0]) for k in RECORD_DTYPE.names] + [("env", "<i4"), ("game", "<i4")])
        for k in RECORD_DTYPE.names:
            out[k] = rec[k]
        out["env"], out["game"] = env, game
        return out

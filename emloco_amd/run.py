"""run.py: entry point with the reference's surface (pacer/pacer/run.py): flags, create_rlgpu_env, RLGPUEnv.

    python -m emloco_amd.run --num_envs 4096 --random_heading --init_heading --heading_inversion \
        --adjust_root_vel --input_init_pose --input_init_vel --steps 200

rl_games (the PPO runner the reference plugs into, pacer/requirements.txt:26) is not vendored; this entry
runs the LocoVal rollout loop of `learning/locoval_rollout.py` (AMPValueAgent.play_steps bookkeeping) with a
frozen random-init policy, and prints the reference's `fps_step` counter (common_agent.py:187).

    python -m emloco_amd.run --test --num_envs 4096 --policy_checkpoint policy.pth --valuenet_path LocoVal.pth \
        [--games_num N] [--eval_out report.json] [--eval_records games.npz] [--compare_valuenet Other.pth ...]
        [--pred_path [--pred_traj_file preds.pkl]] [--eval_tracks] [--eval_crowd [--crowd_near_dist M]]

is the reference's `pacer/run.py --test --valuenet_path ...` (AMPPlayerContinuousValue.run): the frozen policy plays
deterministically and LocoVal is scored against the discounted returns of the games (`learning/locoval_eval.py`).  Every `--compare_valuenet` adds a network (its input configuration read off its fc1 width) that is
scored on the very same games, played once: the input ablation on one set of trajectories.  `--pred_path` makes the humanoid walk the
predictor's output (traj_generator.py:53-54,163-175): the table `evaluate_jta --save_pred_trajs` writes, named by `--pred_traj_file`
(default data/traj/traj_pred_data.pkl); `--eval_records` then carries the table row of every game as `pred_row`.  `--real_path JTA`
takes its tables (`python -m emloco_amd.predictor.export_trajs`) from `--real_traj_file a.pkl[,b.pkl]`.  `--eval_tracks` also records how
closely every game followed its path (learning/locoval_eval.py): a `tracking` block in the report, and in `--eval_records` the per-game
`track` table and the `walked` / `target` xy at the path's own frames, origin-relative as the rows of the predicted-path table.

    python -m emloco_amd.run ... --experiment NAME [--network_path DIR] [--max_iterations N | --steps N] [--save_freq K] [--resume] [--stats]

is what CommonAgent.train does around train_epoch (common_agent.py:151-273), for the LocoVal fit and for `--train_policy` alike: per epoch
the reference's line (`Ep: .. rwd: .. fps_step: .. eps_len: ..`, :236-238) from game statistics kept on the device
(learning/episode_stats.py), one JSON object in DIR/NAME_log.jsonl, and checkpoints under the reference's names (:248-265) --
`NAME_valuenet.pth` (+ `NAME_valuenet_state.pth`, the optimiser / schedule / epoch sidecar) and `NAME_valuenet_<epoch:08d>.pth` for the
LocoVal fit, `NAME.pth` and `NAME_<epoch:08d>.pth` for the policy -- every --save_freq epochs, every fifth of those also as an
intermediate, and at the end.  `--resume` carries an experiment on from them (not the simulator's state nor the random streams: a
valid continuation, not a bit-identical one).  `--stats` alone: the statistics and the line, nothing on disk.

    python -m emloco_amd.run --task HumanoidPedestrianTerrainGetup --cfg_env emloco_amd/data/cfg/pacer_getup.yaml --train_policy ...

trains the policy on the get-up curriculum (env/tasks/humanoid_pedestrain_terrain_getup.py; learning/pre_epoch.py holds its schedule); the
epoch's line and log record gain the share of recovery / fall / normal resets and the mean recovery counter (`getup`).
"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

from .utils.config import get_args, load_cfg, parse_sim_params
from .utils.flags import flags
from .utils.parse_task import parse_task


def fill_flags(args):
    """run.py:263-331."""
    flags.debug, flags.follow, flags.fixed = args.debug, args.follow, True
    flags.divide_group = flags.no_collision_check = flags.fixed_path = False
    flags.real_path = flags.jta_path = flags.jrdb_path = False
    flags.pred_path, flags.small_terrain = args.pred_path, args.small_terrain
    flags.show_traj = flags.render = False
    flags.server_mode, flags.slow, flags.height_debug = args.server_mode, False, False
    flags.random_heading, flags.no_virtual_display = args.random_heading, args.no_virtual_display
    flags.init_heading, flags.heading_inversion = args.init_heading, args.heading_inversion
    flags.adjust_root_vel, flags.input_init_pose = args.adjust_root_vel, args.input_init_pose
    flags.add_noise, flags.vru, flags.add_proj = args.add_noise, args.vru, args.add_proj
    if args.real_path != "":
        flags.real_path = True
        flags.jta_path = "JTA" in args.real_path
        flags.jrdb_path = "JRDB" in args.real_path


def create_rlgpu_env(args, cfg, cfg_train, rank=0):
    """run.py:57-86; per-rank seed offset as run.py:65."""
    seed = cfg_train.get("seed", -1)
    if seed is not None and seed >= 0:
        seed = seed + rank
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
    sim_params = parse_sim_params(args, cfg, cfg_train)
    task, env = parse_task(args, cfg, cfg_train, sim_params)
    return env


class RLGPUEnv:
    """run.py:135-182 without the rl_games base class."""

    def __init__(self, env):
        self.env = env
        self.use_global_obs = self.env.num_states > 0
        self.full_state = {}
        self.full_state["obs"] = self.reset()

    def step(self, action):
        next_obs, reward, is_done, info = self.env.step(action)
        self.full_state["obs"] = next_obs
        return self.full_state["obs"], reward, is_done, info

    def reset(self, env_ids=None):
        self.full_state["obs"] = self.env.reset(env_ids)
        return self.full_state["obs"]

    def get_number_of_agents(self):
        return self.env.get_number_of_agents()


def _pop_opt(argv, name, default=None):
    """Remove `name VALUE` from argv (an option get_args does not know) and return VALUE."""
    if name in argv:
        i = argv.index(name)
        if i + 1 >= len(argv):
            raise SystemExit(f"run.py: {name} needs a value")
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


LOCOVAL_WIDTHS = {100: 3, 98: 2, 28: 1, 26: 0}          # fc1 width -> variant (use_pose << 1) | use_vel (value_pose_net.py:43-50)
MAX_NETS = 8                                             # EMLOCO_EVAL_MAX_NETS


def _pop_all(argv, name):
    """Remove every `name VALUE` from argv and return the VALUEs in order."""
    out = []
    while name in argv:
        out.append(_pop_opt(argv, name))
    return out


def load_compare_valuenets(paths):
    """The checkpoints of --compare_valuenet on the host: [(path, variant, state dict)], the variant inferred from the fc1 width.  A file
    whose width is no LocoVal network's, or a network beyond the eighth of the run (--valuenet_path counts), stops the run."""
    out = []
    for i, path in enumerate(paths):
        if 1 + i >= MAX_NETS:
            raise SystemExit(f"run.py --test: --compare_valuenet {path} is network {2 + i} of the run; one run scores at most {MAX_NETS} "
                             "(--valuenet_path and seven --compare_valuenet)")
        state = torch.load(path, map_location="cpu")
        fc1 = state.get("_network.fc1.weight") if hasattr(state, "get") else None
        width = int(fc1.shape[1]) if fc1 is not None and fc1.dim() == 2 else None
        if width not in LOCOVAL_WIDTHS:
            raise SystemExit(f"run.py --test: --compare_valuenet {path}: fc1 has {width} inputs, no LocoVal network's "
                             f"({' / '.join(str(w) for w in LOCOVAL_WIDTHS)})")
        out.append((path, LOCOVAL_WIDTHS[width], state))
    return out


def pop_test_options(argv):
    """Remove the options of --test from argv (get_args does not know them) and return them; one that is given without --test but means
    nothing there stops the run."""
    opt = dict(games_num=_pop_opt(argv, "--games_num"), eval_out=_pop_opt(argv, "--eval_out"), eval_records=_pop_opt(argv, "--eval_records"),
               max_steps=_pop_opt(argv, "--max_steps"), compare=_pop_all(argv, "--compare_valuenet"), eval_tracks="--eval_tracks" in argv)
    if opt["eval_tracks"]:
        argv.remove("--eval_tracks")
        if "--test" not in argv:
            raise SystemExit("run.py: --eval_tracks records the path tracking of the games of --test")
    opt["eval_crowd"] = "--eval_crowd" in argv
    near = _pop_opt(argv, "--crowd_near_dist")
    if opt["eval_crowd"]:
        argv.remove("--eval_crowd")
        if "--test" not in argv:
            raise SystemExit("run.py: --eval_crowd audits the crowd contacts of the games of --test (training runs take --crowd_audit)")
    opt["crowd_near_dist_given"] = near is not None      # (main checks it against --crowd_audit, which train_options took out of argv)
    try:
        opt["crowd_near_dist"] = 1.0 if near is None else float(near)
    except ValueError as e:
        raise SystemExit(f"run.py: --crowd_near_dist: {e}")
    if not (0.0 < opt["crowd_near_dist"] < float("inf")):
        raise SystemExit("run.py: --crowd_near_dist must be a finite positive length [m]")
    if opt["compare"] and "--test" not in argv:
        raise SystemExit("run.py: --compare_valuenet adds networks to the evaluation of --test")
    return opt


# ---------------------------------------------------------------------------------------------------------------- the crowd spawn
def pop_spawn_options(argv):
    """Remove --group_spawn and its sub-flags from argv (get_args does not know them): None without --group_spawn, else the keys they
    set in cfg["env"] (emloco_amd/crowd_spawn.py).  A sub-flag without --group_spawn, a value that does not parse and
    EMLOCO_OVERLAP_RESET=1 stop the run by name."""
    on = "--group_spawn" in argv
    if on:
        argv.remove("--group_spawn")
    raw = {k: _pop_opt(argv, "--group_spawn_" + k) for k in ("min_dist", "extent", "tries")}
    if not on:
        given = [k for k, v in raw.items() if v is not None]
        if given:
            raise SystemExit(f"run.py: --group_spawn_{given[0]} sets up the crowd spawn: turn it on with --group_spawn")
        return None
    if os.environ.get("EMLOCO_OVERLAP_RESET", "0") == "1":
        raise SystemExit("run.py: --group_spawn places members in the host reset path of the sequential launch arrangement; "
                         "EMLOCO_OVERLAP_RESET=1 switches on a reset chain that never asks it")
    keys = dict(group_spawn=True)
    try:
        if raw["min_dist"] is not None:
            keys["group_spawn_min_dist"] = float(raw["min_dist"])
        if raw["extent"] is not None:
            keys["group_spawn_extent"] = "auto" if raw["extent"] == "auto" else float(raw["extent"])
        if raw["tries"] is not None:
            keys["group_spawn_tries"] = int(raw["tries"])
    except ValueError as e:
        bad = [k for k in ("min_dist", "extent", "tries") if raw[k] is not None and "group_spawn_" + k not in keys][0]
        raise SystemExit(f"run.py: --group_spawn_{bad}: {e}")
    return keys


def apply_spawn_options(keys, env_cfg):
    """Set the keys of --group_spawn on cfg["env"]; a configuration the crowd spawn cannot run on stops here, before the simulator is built"""
    if keys is None:
        return
    from .crowd_spawn import spawn_refusal
    if not env_cfg.get("divide_group", False):
        raise SystemExit("run.py --group_spawn: the configuration has no groups (divide_group); the crowd spawn places the members of a "
                         "group apart (emloco_amd/data/cfg/pacer_group.yaml is one that has them)")
    why = spawn_refusal(dict(env_cfg, **keys))
    if why:
        raise SystemExit(f"run.py --group_spawn: {why}")
    env_cfg.update(keys)


def _spawn_of(task):
    return getattr(task, "_spawn", None)


# ---------------------------------------------------------------------------------------------------------------- the flight recorder
def capture_options(argv):
    """Remove the flight recorder's options from argv (get_args does not know them): None without --capture, else the arguments of
    `make_capture`.  Non-finite states are always a cause; the speed and early-fall causes are off unless their option is given."""
    path = _pop_opt(argv, "--capture")
    raw = {k: _pop_opt(argv, "--capture_" + k) for k in ("depth", "slots", "speed", "ang_speed", "early_fall")}
    if path is None:
        given = [k for k, v in raw.items() if v is not None]
        if given:
            raise SystemExit(f"run.py: --capture_{given[0]} sets up the flight recorder: turn it on with --capture PATH")
        return None
    try:
        opt = dict(path=path, depth=int(raw["depth"] or 8), slots=int(raw["slots"] or 16),
                   speed=None if raw["speed"] is None else float(raw["speed"]),
                   ang_speed=None if raw["ang_speed"] is None else float(raw["ang_speed"]),
                   early_fall=None if raw["early_fall"] is None else int(raw["early_fall"]))
    except ValueError as e:
        raise SystemExit(f"run.py: --capture_*: {e}")
    if opt["depth"] < 1 or opt["slots"] < 1 or any(opt[k] is not None and not opt[k] >= 0 for k in ("speed", "ang_speed", "early_fall")):
        raise SystemExit("run.py: --capture_depth / --capture_slots must be at least 1, the limits not negative")
    return opt


def make_capture(task, opt, rank=0, world=1):
    """The run's flight recorder and its file (learning/flight_recorder.py): rank r of several writes PATH with _rank{r} ahead of the
    extension.  To be called once the loop is built: a task whose launch arrangement the recorder cannot follow (overlap_reset, which
    a loop's constructor switches on) stops the run by name here; switched on later still, it raises where the recorder is bound."""
    from .learning.flight_recorder import CaptureLog, FlightRecorder, rank_path
    try:
        rec = FlightRecorder(task, depth=opt["depth"], slots=opt["slots"], speed=opt["speed"], ang_speed=opt["ang_speed"],
                             early_fall=opt["early_fall"])
    except RuntimeError as e:
        raise SystemExit(f"run.py --capture: {e}")
    path = rank_path(opt["path"], rank, world)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    return CaptureLog(rec, path, per_file=opt.get("per_file", 256))


# ---------------------------------------------------------------------------------------------------------------- the training driver
def train_options(argv, args=None):
    """What the driver needs of the command line, checked before anything touches a device: `--steps N` is taken out of argv (get_args
    does not know it), the driver's own flags are read from `args` (utils/config.py) or, ahead of get_args, straight from argv."""
    steps = None
    if "--steps" in argv:
        i = argv.index("--steps")
        if i + 1 >= len(argv):
            raise SystemExit("run.py: --steps needs a value")
        steps = int(argv[i + 1])
        del argv[i:i + 2]
    flag = lambda name: (name in argv) if args is None else bool(getattr(args, name[2:]))
    val = lambda name, default, conv: (conv(_pop_opt(list(argv), name, default)) if args is None else conv(getattr(args, name[2:])))
    opt = dict(steps=steps, experiment=val("--experiment", "", str), network_path=val("--network_path", "output/", str),
               max_iterations=val("--max_iterations", 0, int), save_freq=val("--save_freq", 200, int), resume=flag("--resume"),
               stats=flag("--stats"), crowd_audit="--crowd_audit" in argv)
    if opt["crowd_audit"]:
        argv.remove("--crowd_audit")                     # (get_args does not know it)
        if "--test" in argv:
            raise SystemExit("run.py: --crowd_audit belongs to training (--stats / --experiment); --test takes --eval_crowd")
        if not (opt["stats"] or opt["experiment"]):
            raise SystemExit("run.py: --crowd_audit adds to the epoch statistics: give it with --stats or --experiment NAME")
        if "--train_policy" in argv:
            raise SystemExit("run.py: --crowd_audit rides in the LocoVal rollout; --train_policy is refused on crowd configurations")
    if steps is not None and opt["max_iterations"] > 0:
        raise SystemExit("run.py: --steps and --max_iterations both say how long to train: give one of them")
    if opt["max_iterations"] < 0 or (steps is not None and steps < 0):
        raise SystemExit("run.py: --steps / --max_iterations must not be negative")
    if opt["resume"] and not opt["experiment"]:
        raise SystemExit("run.py: --resume continues an experiment: name it with --experiment NAME")
    if "--test" in argv and (opt["experiment"] or opt["resume"] or opt["stats"] or opt["max_iterations"]):
        raise SystemExit("run.py: --experiment / --max_iterations / --resume / --stats belong to training, not to --test")
    opt["stats"] = opt["stats"] or bool(opt["experiment"])
    opt["driver"] = bool(opt["experiment"] or opt["stats"] or opt["max_iterations"])
    opt["model_output_file"] = os.path.join(opt["network_path"], opt["experiment"]) if opt["experiment"] else None
    return opt


def epoch_line(kind, epoch, frame, info):
    """The reference's per-epoch line (common_agent.py:236-238): the long variant for the LocoVal fit, the short one for the policy
    trainer.  An epoch without a finished game prints 0 for the means of the games."""
    g = info.get("games") or {}
    rwd, eps_len = g.get("ret_mean", 0.0), g.get("len_mean", 0.0)
    head = f"Ep: {epoch}\trwd: {rwd:.2f}" if kind == "locoval" else f"Ep: {epoch}\trwd: {rwd:.1f}"
    if kind == "locoval":
        head += f"\tvnet_pred: {info['vnet_pred']:.2f}\tcombine_rwd: {info['combine_rwd']:.2f}\tvnet_loss: {info['vnet_loss']:.3f}"
    return head + (f"\tfps_step: {info['fps_step']:.1f}\tfps_total: {info['fps_total']:.1f}\tep_time:{info['ep_time']:.1f}"
                   f"\tframe: {frame}\teps_len: {eps_len:.1f}")


def run_training(trainee, opt, say=print, rank=0):
    """CommonAgent.train around `trainee.run_epoch()` (common_agent.py:151-273).  `trainee` (LocoValTrainee / PolicyTrainee below, a stub
    in the tests) has `kind`, `horizon_length`, `epoch_num`, `frame`, `run_epoch() -> dict`, `save(model_output_file, epoch=None)`,
    `resume(model_output_file)` and `final_line(steps, seconds)`.  Returns the number of epochs it ran."""
    mof, K = opt["model_output_file"], int(opt["save_freq"])
    log = None
    if mof:
        if rank == 0:
            os.makedirs(os.path.dirname(mof) or ".", exist_ok=True)
        if opt["resume"]:
            trainee.resume(mof)
            say(f"resumed {mof} at epoch {trainee.epoch_num}, frame {trainee.frame}")
        if rank == 0:
            log = open(mof + "_log.jsonl", "a" if opt["resume"] else "w")
    # --max_iterations counts the experiment's epochs in total, as the reference's max_epochs does (a resumed run trains the rest);
    # --steps (default 100) asks for that many more env steps, in whole epochs
    if opt["max_iterations"] > 0:
        todo = max(opt["max_iterations"] - trainee.epoch_num, 0)
    else:
        steps = 100 if opt["steps"] is None else opt["steps"]
        todo = -(-steps // trainee.horizon_length)
    t0 = time.time()
    ran = 0
    try:
        for _ in range(todo):
            info = trainee.run_epoch()
            ran += 1
            epoch, frame = trainee.epoch_num, trainee.frame
            if opt["stats"]:
                say(epoch_line(trainee.kind, epoch, frame, info) + info.get("tail", ""))
            if log is not None:
                rec = dict(epoch=epoch, frame=frame, wall_time=time.time(), **{k: v for k, v in info.items() if k != "tail"})
                log.write(json.dumps(rec, default=float) + "\n")
                log.flush()
            if mof and K > 0 and epoch % K == 0:
                trainee.save(mof)
                say("latest model saved")
                if epoch % (5 * K) == 0:
                    trainee.save(mof, epoch)
                    say("intermediate model saved")
        if mof:
            trainee.save(mof)
    finally:
        if log is not None:
            log.close()
    line = trainee.final_line(ran * trainee.horizon_length, time.time() - t0)
    if line:
        say(line)
    return ran


def _locoval_final_line(agent, num_envs, world, n, dt):
    return (f"fps_step: {num_envs * world * n / dt:,.0f} env-steps/s ({n} steps of {num_envs} envs x {world} ranks), "
            f"LocoVal loss {agent.vnet_loss:.4f}, {agent.fitted_episodes} episodes fitted")


def _policy_epoch_tail(info):
    return (f"fps_step {info['fps_step']:,.0f} fps_total {info['fps_total']:,.0f} "
            f"a_loss {info['actor_loss']:.4f} c_loss {info['critic_loss']:.4f} disc_loss {info['disc_loss']:.4f} kl {info['kl']:.5f}")


def locoval_loop(agent, num_envs, world, steps, say=print):
    """The entry point's LocoVal loop without the driver's flags: `steps` env steps in whole horizons, one line at the very end."""
    t0 = time.time()
    n = 0
    while n < steps:
        agent.play_steps()
        n += agent.horizon_length
    torch.cuda.synchronize()
    say(_locoval_final_line(agent, num_envs, world, n, time.time() - t0))


def policy_loop(agent, steps, say=print):
    """The entry point's PPO + AMP loop without the driver's flags: one line per epoch with the losses."""
    n = 0
    while n < steps:
        info = agent.train_epoch()
        n += agent.horizon_length
        say(f"epoch {agent.epoch_num}: " + _policy_epoch_tail(info))


class LocoValTrainee:
    """The LocoVal fit under run_training: an epoch is one horizon of `LocoValRollout.step_once` and `end_epoch`."""
    kind = "locoval"

    def __init__(self, agent, world=1, rank=0, stats=None, capture=None, crowd=None):
        self.agent, self.world, self.rank, self.stats, self.capture, self.crowd = agent, world, rank, stats, capture, crowd
        self.horizon_length = agent.horizon_length
        if crowd is not None:
            agent.attach_crowd_audit(crowd)
        if stats is not None:
            agent.attach_episode_stats(stats)
        if capture is not None:
            agent.attach_flight_recorder(capture.recorder)

    epoch_num = property(lambda self: self.agent.epoch_num)
    frame = property(lambda self: self.agent.frames * self.world)

    def run_epoch(self):
        a = self.agent
        t0 = time.time()
        a.pre_epoch(a.epoch_num + 1)                     # the motion clips are redrawn on the reference's schedule (learning/pre_epoch.py)
        for _ in range(a.horizon_length):
            a.step_once()
        a.end_epoch()
        info = {}
        if self.stats is not None:
            games, own = a.epoch_report()                # (waits for the epoch's launches: the one read of the device)
            info.update(games=games, **own)
        else:
            torch.cuda.synchronize()
        dt = max(time.time() - t0, 1e-9)
        frames = a.num_actors * self.world * a.horizon_length
        info.update(fps_step=frames / dt, fps_total=frames / dt, ep_time=dt)     # the fit runs beside the rollout: one clock for both
        if self.capture is not None:
            info.update(self.capture.end_epoch())        # one read of the counters; the file grows only when captures were taken
        if self.crowd is not None:                       # one reduction and one read per epoch (this rank's envs)
            from .crowd_contacts import epoch_tail
            info["crowd"] = self.crowd.end_epoch()
            info["tail"] = info.get("tail", "") + epoch_tail(info["crowd"])
        spawn = _spawn_of(getattr(a, "task", None))
        if spawn is not None and self.stats is not None:  # the epoch's placements (this rank's envs): one read of four totals
            from .crowd_spawn import epoch_tail as spawn_tail
            info["spawn"] = spawn.totals(clear=True)
            info["tail"] = info.get("tail", "") + spawn_tail(info["spawn"])
        return info

    def save(self, mof, epoch=None):
        if self.rank != 0:
            return
        self.agent.save(mof, epoch)
        if epoch is None:
            self.agent.save_state(mof)

    def resume(self, mof):
        self.agent.restore_state(mof)

    def final_line(self, n, dt):
        return _locoval_final_line(self.agent, self.agent.num_actors, self.world, n, max(dt, 1e-9))


class PolicyTrainee:
    """PPO + AMP under run_training: an epoch is one `AMPAgent.train_epoch`."""
    kind = "policy"

    def __init__(self, agent, world=1, rank=0, stats=None, capture=None):
        self.agent, self.world, self.rank, self.stats, self.capture = agent, world, rank, stats, capture
        self.horizon_length = agent.horizon_length
        agent.episode_stats = stats
        agent.flight_recorder = None if capture is None else capture.recorder.bind()

    epoch_num = property(lambda self: self.agent.epoch_num)
    frame = property(lambda self: self.agent.frame * self.world)

    def run_epoch(self):
        info = self.agent.train_epoch()
        out = {k: info[k] for k in ("actor_loss", "critic_loss", "disc_loss", "kl", "reward_raw") if k in info}
        out.update(fps_step=info["fps_step"] * self.world, fps_total=info["fps_total"] * self.world, ep_time=info["total_time"])
        if self.stats is not None:
            out["games"] = self.stats.end_epoch()
        if self.capture is not None:
            out.update(self.capture.end_epoch())
        out["tail"] = (f"\ta_loss {info['actor_loss']:.4f} c_loss {info['critic_loss']:.4f} disc_loss {info['disc_loss']:.4f} "
                       f"kl {info['kl']:.5f}")
        task = getattr(self.agent, "task", None)
        if self.stats is not None and hasattr(task, "getup_epoch_stats"):
            # the get-up task's reset mix and mean recovery counter of the epoch, from sums its kernels keep on the device (one read)
            g = out["getup"] = task.getup_epoch_stats()
            out["tail"] += (f"\tgetup rec/fall/normal {g['getup_recovery_share']:.2f}/{g['getup_fall_share']:.2f}/{g['getup_normal_share']:.2f}"
                            f" counter {g['getup_mean_recovery_counter']:.1f}")
        return out

    def save(self, mof, epoch=None):
        if self.rank == 0:
            self.agent.save(mof if epoch is None else mof + "_" + str(epoch).zfill(8))

    def resume(self, mof):
        self.agent.restore(mof + ".pth")

    def final_line(self, n, dt):
        return None


def load_policy_cfg(args):
    """The policy's training configuration (network, algorithm settings): the file of --cfg_train, the shipped sept configuration
    without one."""
    import yaml
    from .learning.amp_policy import DEFAULT_CFG
    path = args.cfg_train or DEFAULT_CFG
    try:
        with open(path) as f:
            return yaml.safe_load(f)
    except OSError as e:
        raise SystemExit(f"run.py --cfg_train: cannot read {path}: {e}")


def crowd_policy_refusal(env_cfg, network, use_policy, train_policy, test, cnn_backward=False):
    """Why this combination of environment configuration, policy network (`params.network.name` of the training configuration) and
    flags cannot run, or None.  `cnn_backward`: --cnn_backward was given, which lets --train_policy through for the amp_sept_cnn
    network (the trunk's backward kernel, emloco_cnn_trunk_backward).  No device is touched."""
    from .crowd_sensor import is_crowd_config
    if not (use_policy or train_policy or test):
        return None
    from .learning.amp_policy import NETWORKS
    if network not in NETWORKS:
        return f"run.py --cfg_train: network '{network}' is not built (params.network.name: one of {', '.join(NETWORKS)})"
    crowd = is_crowd_config(env_cfg)
    from .crowd_people import config_block
    if config_block(env_cfg):
        # group_obs: the map carries no stamps and the rows end in the `people` block, which the sept network's point-net branch reads
        # (amp_network_sept_builder.py); frozen, --test and --train_policy alike -- its layers are GEMMs with a backward
        if network == "amp_sept_cnn":
            return ("run.py: the configuration has group_obs: True, and the policy network 'amp_sept_cnn' does not read the 'people' block "
                    "it appends to the observation (its map slice assumes the map ends the row).  The people block is read by the sept "
                    "network's point-net branch: pass --cfg_train emloco_amd/data/cfg/train/rlg/amp_humanoid_smpl_sept_task.yaml, or none")
        if env_cfg.get("velocity_map", False):
            return ("run.py: the configuration has group_obs: True with velocity_map: True, and the sept network's task MLP reads a "
                    "one-channel 'heightmap' block (amp_network_sept_builder.py:113-116): set velocity_map: False, as "
                    "emloco_amd/data/cfg/pacer_group_obs.yaml does")
        return None
    if train_policy and (crowd or network == "amp_sept_cnn") and not (cnn_backward and network == "amp_sept_cnn"):
        return ("run.py --train_policy: the CNN policy of the crowd sensor (amp_network_sept_cnn_builder.py, network amp_sept_cnn) runs as "
                "inference only by default -- the CNN trunk's backward is not built into the default run, so it cannot be trained without "
                "asking: add --cnn_backward (with --cfg_train emloco_amd/data/cfg/train/rlg/amp_humanoid_smpl_cnn_task.yaml) to train it "
                "through emloco_cnn_trunk_backward; an opt-in, the device path is unmeasured and nobody has shown that this network learns "
                "on this physics.  A frozen policy (--policy_checkpoint / --policy_random_init) and --test take --cfg_train "
                "emloco_amd/data/cfg/train/rlg/amp_humanoid_smpl_cnn_task.yaml")
    if crowd and network != "amp_sept_cnn":
        return ("run.py: the configuration asks for the crowd sensor (divide_group / velocity_map / sensor_res / sensor_extent), whose "
                f"observations the policy network '{network}' cannot read: they need the CNN trunk (amp_network_sept_cnn_builder.py).  Pass "
                "--cfg_train emloco_amd/data/cfg/train/rlg/amp_humanoid_smpl_cnn_task.yaml (network amp_sept_cnn) with --policy_checkpoint, "
                "--policy_random_init or --test.  Without a policy flag the run is the LocoVal loop under noise actions")
    return None


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    train_opt = train_options(argv)                      # (--steps leaves argv; a bad combination stops the run before any device call)
    # --test (the reference's player, amp_value_players.py): its own options, checked before anything touches a device
    opt = pop_test_options(argv)
    spawn_opt = pop_spawn_options(argv)
    cap_opt = capture_options(argv)
    if cap_opt is not None and "--test" not in argv:
        train_opt["driver"] = True                       # the recorder is drained once per epoch: the run goes through the driver
    games_num, eval_out, eval_records, max_steps = opt["games_num"], opt["eval_out"], opt["eval_records"], opt["max_steps"]
    compare, eval_tracks = opt["compare"], opt["eval_tracks"]
    eval_crowd = (opt["crowd_near_dist"],) if opt["eval_crowd"] else None
    if opt["crowd_near_dist_given"] and not (opt["eval_crowd"] or train_opt["crowd_audit"]):
        raise SystemExit("run.py: --crowd_near_dist sets up the crowd contact audit: turn it on with --eval_crowd (--test) or --crowd_audit")
    if "--test" in argv:
        vp = _pop_opt(list(argv), "--valuenet_path", "")
        if not vp:
            raise SystemExit("run.py --test: --valuenet_path <LocoVal.pth> is required (the LocoVal network to evaluate; "
                             "pacer/run.py --test takes it the same way)")
        if "--policy_checkpoint" not in argv and "--policy_random_init" not in argv:
            raise SystemExit("run.py --test: give the policy to play, --policy_checkpoint <policy.pth> or --policy_random_init")
        if "--train_policy" in argv:
            raise SystemExit("run.py: --test and --train_policy exclude each other")
        compare = load_compare_valuenets(compare)
    from . import configure_runtime
    configure_runtime()                                  # entry point: 16 hardware queues, ahead of the first GPU call (emloco_amd/__init__.py)
    steps = 100 if train_opt["steps"] is None else train_opt["steps"]
    policy_ckpt, use_policy = None, False
    if "--policy_checkpoint" in argv:            # rl_games-layout checkpoint of the frozen PACER policy (config 3)
        i = argv.index("--policy_checkpoint")
        policy_ckpt, use_policy = argv[i + 1], True
        del argv[i:i + 2]
    if "--policy_random_init" in argv:           # same architecture, random weights (no checkpoint ships)
        use_policy = True
        argv.remove("--policy_random_init")
    train_policy = "--train_policy" in argv        # configs[1]: PPO + AMP pretraining of the policy (pacer/run.py without --test)
    if train_policy:
        argv.remove("--train_policy")
    cnn_backward = "--cnn_backward" in argv        # opt-in: PPO on the amp_sept_cnn network through the trunk's backward kernel
    if cnn_backward:
        argv.remove("--cnn_backward")
        if not train_policy:
            raise SystemExit("run.py --cnn_backward: the flag switches on the CNN trunk's backward for --train_policy and means nothing "
                             "without it (a frozen policy and --test never differentiate the trunk)")
    # one process per GPU (torch.distributed.run): the reference's --horovod launch (run.py:57-66, common_agent.py:165-180).
    # num_envs is the GLOBAL count: rank r simulates the contiguous shard [r * E / W, (r + 1) * E / W) on cuda:LOCAL_RANK with
    # seed + rank; the learners exchange gradients / statistics through emloco_amd.dist
    from .dist import init_from_env, shard_range
    rank, local_rank, world = init_from_env()
    if world > 1:
        for flag in ("--sim_device", "--rl_device"):
            if flag in argv:
                i = argv.index(flag)
                del argv[i:i + 2]
        argv += ["--sim_device", f"cuda:{local_rank}", "--rl_device", f"cuda:{local_rank}"]
        torch.cuda.set_device(local_rank)
    args = get_args(argv)
    if world > 1:
        args.num_envs = shard_range(int(args.num_envs), rank, world)[1]
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    apply_spawn_options(spawn_opt, cfg["env"])
    policy_cfg = load_policy_cfg(args) if (use_policy or train_policy or args.test) else None
    network = policy_cfg["params"]["network"].get("name", "amp_sept") if policy_cfg else None
    refusal = crowd_policy_refusal(cfg["env"], network, use_policy, train_policy, args.test, cnn_backward=cnn_backward)
    if refusal:
        raise SystemExit(refusal)
    if cnn_backward and network != "amp_sept_cnn":
        raise SystemExit(f"run.py --cnn_backward: the policy network '{network}' has no CNN trunk to differentiate; the flag goes with "
                         "--cfg_train emloco_amd/data/cfg/train/rlg/amp_humanoid_smpl_cnn_task.yaml (network amp_sept_cnn)")
    if eval_crowd is not None or train_opt["crowd_audit"]:      # a configuration the audit cannot run on stops here, before the simulator is built
        from .crowd_contacts import config_refusal
        why = config_refusal(cfg["env"])
        if why:
            raise SystemExit(f"run.py {'--eval_crowd' if eval_crowd is not None else '--crowd_audit'}: {why}")
    if flags.pred_path:                                  # a missing table stops the run here, by name, before the simulator is built
        from .env.util.traj_generator import PRED_TRAJ_FILE
        import os
        pred_file = cfg["env"].get("pred_traj_data", None) or PRED_TRAJ_FILE
        if isinstance(pred_file, str) and not os.path.isfile(pred_file):
            raise SystemExit(f"run.py --pred_path: the predicted-path table {pred_file} does not exist (--pred_traj_file PATH names it; "
                             "`python -m emloco_amd.predictor.evaluate_jta --save_pred_trajs PATH` writes one)")
    env = RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train, rank=rank))
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.test:
        capture = None if cap_opt is None else make_capture(env.env.task, cap_opt, rank, world)
        _run_test(args, env, policy_ckpt, games_num, max_steps, eval_out, eval_records, rank, world, say, compare, eval_tracks, capture,
                  policy_cfg, eval_crowd)
        return
    if train_policy:
        from .learning.amp_agent import AMPAgent
        agent = AMPAgent(env, policy_cfg)
        if policy_ckpt:
            agent.restore(policy_ckpt)
        capture = None if cap_opt is None else make_capture(env.env.task, cap_opt, rank, world)
        if train_opt["driver"]:
            from .learning.episode_stats import EpisodeStats
            stats = EpisodeStats(env.env.task) if train_opt["stats"] else None           # the policy trainer's rewards carry no penalty
            run_training(PolicyTrainee(agent, world, rank, stats, capture), train_opt, say, rank)
        else:
            policy_loop(agent, steps, say)
        return
    from .learning.locoval_rollout import LocoValRollout
    kw = {}
    if use_policy:
        from .learning.amp_policy import AMPPolicyBundle
        bundle = AMPPolicyBundle(env.env.task, cfg_train=policy_cfg, checkpoint=policy_ckpt)
        kw = dict(policy=bundle.policy, disc_reward=bundle.disc_reward,
                  inversion_penalty_scale=float(bundle.config.get("inversion_penalty_scale", 0.3)))
    agent = LocoValRollout(env, use_pose=args.input_init_pose, use_vel=args.input_init_vel, **kw)
    # (behind the loop's constructor, which is where a launch arrangement is switched on: EMLOCO_OVERLAP_RESET=1 stops the run here)
    capture = None if cap_opt is None else make_capture(env.env.task, cap_opt, rank, world)
    if train_opt["driver"]:
        stats = None
        if train_opt["stats"]:
            from .learning.episode_stats import EpisodeStats
            stats = EpisodeStats(env.env.task, inverted_penalty=agent.inversion_penalty_scale)
        crowd = None
        if train_opt["crowd_audit"]:
            from .crowd_contacts import CrowdContactAudit, CrowdContactRefusal
            try:
                crowd = CrowdContactAudit(env.env.task, near_dist=opt["crowd_near_dist"], totals=True)
            except CrowdContactRefusal as e:
                raise SystemExit(f"run.py --crowd_audit: {e}")
        try:
            trainee = LocoValTrainee(agent, world, rank, stats, capture, crowd)
        except RuntimeError as e:
            if crowd is None:
                raise
            raise SystemExit(f"run.py --crowd_audit: {e}")
        run_training(trainee, train_opt, say, rank)
    else:
        locoval_loop(agent, env.env.num_envs, world, steps, say)
    if world > 1:
        torch.distributed.destroy_process_group()


def _track_columns(ev):
    """--eval_tracks: the --eval_records columns of this rank's games, in the order of its records."""
    walked, target = ev.track_samples()
    trk = ev.track_records()
    from numpy.lib import recfunctions
    cols = recfunctions.repack_fields(trk[[k for k in trk.dtype.names if k not in ("env", "game")]])      # env / game are columns already
    return dict(track=cols, walked=walked, target=target)


def _gather_track_columns(ev, world):
    """The track columns of every rank, concatenated in rank order as the records are (collective)."""
    parts = [_track_columns(ev)]
    if world > 1:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, parts[0])
        parts = gathered
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _crowd_columns(ev, world):
    """--eval_crowd: the `crowd` column set of --eval_records, the record fields of every rank's games in the order of the records
    (collective)."""
    from numpy.lib import recfunctions
    rec = ev.crowd_records()
    parts = [recfunctions.repack_fields(rec[[k for k in rec.dtype.names if k not in ("env", "game")]])]      # env / game are columns already
    if world > 1:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, parts[0])
        parts = gathered
    return dict(crowd=np.concatenate(parts))


def _crowd_kw(eval_crowd):
    return {} if eval_crowd is None else dict(crowd=True, crowd_near_dist=eval_crowd[0])


def _run_test(args, env, policy_ckpt, games_num, max_steps, eval_out, eval_records, rank, world, say, compare=(), eval_tracks=False,
              capture=None, cfg_train=None, eval_crowd=None):
    """--test: LocoValEvaluator with the frozen policy (deterministic actions) and the LocoVal network of --valuenet_path.
    cfg_train: the policy's training configuration (load_policy_cfg).  eval_crowd: None, or (near_dist,) of --eval_crowd."""
    import json
    from .learning.amp_policy import AMPPolicyBundle
    from .learning.locoval_eval import LocoValEvaluator, TrackRefusal
    from .learning.value_pose_net import ValuePoseNet
    if cfg_train is None:
        cfg_train = load_policy_cfg(args)
    config = cfg_train["params"]["config"]
    player = config.get("player", {})
    task = env.env.task
    bundle = AMPPolicyBundle(task, cfg_train=cfg_train, checkpoint=policy_ckpt, deterministic=bool(player.get("deterministic", True)))
    state = torch.load(args.valuenet_path, map_location=task.device)
    use_pose, use_vel = bool(args.input_init_pose), bool(args.input_init_vel)          # amp_value_players.py:294-301 (player.use_pose / use_vel)
    fc1 = state.get("_network.fc1.weight") if hasattr(state, "get") else None
    if not (use_pose or use_vel) and fc1 is not None and fc1.dim() == 2 and int(fc1.shape[1]) in (100, 98, 28):
        # neither flag given: a checkpoint with pose / velocity inputs is evaluated as what it is (as before the flags were wired),
        # an explicit flag that contradicts the checkpoint is an error below
        use_pose, use_vel = int(fc1.shape[1]) >= 98, int(fc1.shape[1]) in (100, 28)
        say(f"--valuenet_path holds a network with {int(fc1.shape[1])} inputs: evaluating it with use_pose={use_pose} use_vel={use_vel}")
    valuenet = ValuePoseNet(use_pose=use_pose, use_vel=use_vel).to(task.device)
    try:
        valuenet.load_state_dict(state)
    except RuntimeError as e:
        raise SystemExit(f"run.py --test: --valuenet_path {args.valuenet_path} does not fit --input_init_pose={use_pose} "
                         f"--input_init_vel={use_vel}: {e}")
    valuenet.eval()
    if compare:
        _run_compare(args, env, bundle, valuenet, compare, int(games_num) if games_num else int(player.get("games_num", 200)),
                     int(max_steps) if max_steps else 27000, float(config.get("gamma", 0.99)), eval_out, eval_records, rank, world, say,
                     eval_tracks, capture, eval_crowd)
        return
    from .crowd_contacts import CrowdContactRefusal
    try:
        ev = LocoValEvaluator(env, bundle, valuenet, int(games_num) if games_num else int(player.get("games_num", 200)),
                              max_steps=int(max_steps) if max_steps else 27000, gamma=float(config.get("gamma", 0.99)), track=eval_tracks,
                              **_crowd_kw(eval_crowd))
    except (TrackRefusal, CrowdContactRefusal) as e:      # --eval_tracks / --eval_crowd on a task they cannot run on: a message, no traceback
        raise SystemExit(f"run.py --test: {e}")
    if capture is not None:
        ev.flight_recorder = capture.recorder.bind()
    t0 = time.time()
    rep = ev.run(say=say)
    torch.cuda.synchronize()
    rep["seconds"] = time.time() - t0
    say(f"{rep['steps']} steps of {ev.envs_total} envs in {rep['seconds']:.2f} s")
    if _spawn_of(task) is not None:          # --group_spawn: inside `crowd` with --eval_crowd, beside it otherwise (this rank's envs)
        from .crowd_spawn import report_line
        block = _spawn_of(task).totals()
        (rep["crowd"] if eval_crowd is not None else rep)["spawn"] = block
        say(report_line(block))
    if capture is not None:                  # --test: one drain at the end of the run
        rep.update(capture.end_epoch())
        say(f"flight recorder: {rep['captures']} captures in {capture.path}")
    recs = ev.records()
    pred_row = ev.pred_rows(recs)
    if pred_row is not None:                 # --pred_path: the table row every game walked joins a record to its sample / mode
        from numpy.lib import recfunctions
        recs = recfunctions.append_fields(recs, "pred_row", pred_row, dtypes="<i8", usemask=False)
    if eval_records:
        # per-game records of every rank (what the reference draws as scatter plots): gathered on rank 0
        parts = [recs]
        if world > 1:
            gathered = [None] * world
            torch.distributed.all_gather_object(gathered, recs)
            parts = gathered
        tcols = _gather_track_columns(ev, world) if eval_tracks else {}
        if eval_crowd is not None:
            tcols.update(_crowd_columns(ev, world))
        if rank == 0:
            cols = {k: np.concatenate([p[k] for p in parts]) for k in recs.dtype.names}
            cols["rank"] = np.concatenate([np.full(len(p), r, np.int32) for r, p in enumerate(parts)])
            cols.update(tcols)
            np.savez(eval_records, **cols)
    if eval_out and rank == 0:
        with open(eval_out, "w") as f:
            json.dump({k: v for k, v in rep.items()}, f, indent=1, default=float)
    if world > 1:
        torch.distributed.destroy_process_group()


def compare_columns(recs):
    """The --eval_records columns of N networks' record arrays (the same games): the shared per-game columns once, `value_<i>` and
    `sq_err_<i>` per network."""
    cols = {k: recs[0][k] for k in recs[0].dtype.names if k not in ("value", "sq_err")}
    for i, r in enumerate(recs):
        cols[f"value_{i}"], cols[f"sq_err_{i}"] = r["value"], r["sq_err"]
    return cols


def _run_compare(args, env, bundle, valuenet, compare, games_num, max_steps, gamma, eval_out, eval_records, rank, world, say,
                 eval_tracks=False, capture=None, eval_crowd=None):
    """--test with --compare_valuenet: the network of --valuenet_path and the added ones on the same games, played once."""
    import json
    from .learning.locoval_eval import LocoValEvaluator, TrackRefusal
    from .learning.value_pose_net import ValuePoseNet
    task = env.env.task
    nets, paths = [valuenet], [args.valuenet_path]
    for path, variant, state in compare:
        with torch.random.fork_rng(devices=[]):             # an added network's initialisation draws nothing from the run's random stream
            net = ValuePoseNet(use_pose=bool(variant & 2), use_vel=bool(variant & 1)).to(task.device)
        try:
            net.load_state_dict(state)
        except RuntimeError as e:
            raise SystemExit(f"run.py --test: --compare_valuenet {path} does not load as the network its fc1 width names: {e}")
        nets.append(net.eval())
        paths.append(path)
    from .crowd_contacts import CrowdContactRefusal
    try:
        ev = LocoValEvaluator(env, bundle, nets, games_num, max_steps=max_steps, gamma=gamma, track=eval_tracks, **_crowd_kw(eval_crowd))
    except (TrackRefusal, CrowdContactRefusal) as e:      # --eval_tracks / --eval_crowd on a task they cannot run on: a message, no traceback
        raise SystemExit(f"run.py --test: {e}")
    if capture is not None:
        ev.flight_recorder = capture.recorder.bind()
    t0 = time.time()
    rep = ev.run(say=say)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    say(f"{ev.steps_run} steps of {ev.envs_total} envs in {seconds:.2f} s, {len(nets)} networks on the same games")
    if _spawn_of(task) is not None:          # --group_spawn: inside `crowd` with --eval_crowd, beside it otherwise (this rank's envs)
        from .crowd_spawn import report_line
        block = _spawn_of(task).totals()
        (rep["crowd"] if eval_crowd is not None else rep)["spawn"] = block
        say(report_line(block))
    if capture is not None:                  # one drain at the end of the run
        say(f"flight recorder: {capture.end_epoch()['captures']} captures in {capture.path}")
    if eval_records:
        parts = [compare_columns(ev.records())]
        pred_row = ev.pred_rows(ev.records(0))
        if pred_row is not None:
            parts[0]["pred_row"] = pred_row
        if world > 1:
            gathered = [None] * world
            torch.distributed.all_gather_object(gathered, parts[0])
            parts = gathered
        tcols = _gather_track_columns(ev, world) if eval_tracks else {}
        if eval_crowd is not None:
            tcols.update(_crowd_columns(ev, world))
        if rank == 0:
            cols = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
            cols["rank"] = np.concatenate([np.full(len(p["env"]), r, np.int32) for r, p in enumerate(parts)])
            cols.update(tcols)
            np.savez(eval_records, **cols)
    if eval_out and rank == 0:
        for r in rep["networks"]:
            r["seconds"] = seconds
        with open(eval_out, "w") as f:
            out = {"networks": [dict(path=p, variant=n.variant, report=r) for p, n, r in zip(paths, nets, rep["networks"])],
                   "paired": rep["paired"]}
            if eval_tracks:
                out["tracking"] = rep["tracking"]
            if eval_crowd is not None:
                out["crowd"] = rep["crowd"]
            elif "spawn" in rep:
                out["spawn"] = rep["spawn"]
            json.dump(out, f, indent=1, default=float)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

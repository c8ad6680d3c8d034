"""Argument parsing and config loading with the reference's flag names.

Mirror of pacer/pacer/utils/config.py (get_args :177-529, load_cfg :64-138, parse_sim_params :141-174) for the
flags that reach the rollout hot path.  rl_games / wandb / viewer options are accepted and ignored.
"""
import os

import yaml

from ..gym import gymapi, gymutil

SIM_TIMESTEP = 1.0 / 60.0
_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CFG_ENV = os.path.join(_HERE, "data", "cfg", "pacer.yaml")


def get_args(argv=None):
    custom_parameters = [
        {"name": "--test", "action": "store_true", "default": False},
        {"name": "--debug", "action": "store_true", "default": False},
        {"name": "--headless", "action": "store_true", "default": True},
        {"name": "--task", "type": str, "default": "HumanoidPedestrianTerrain"},
        {"name": "--rl_device", "type": str, "default": "cuda:0"},
        {"name": "--seed", "type": int, "default": -1},
        {"name": "--num_envs", "type": int, "default": 0},
        {"name": "--episode_length", "type": int, "default": 0},
        {"name": "--cfg_env", "type": str, "default": DEFAULT_CFG_ENV},
        {"name": "--cfg_train", "type": str, "default": ""},
        {"name": "--motion_file", "type": str, "default": "synthetic"},
        {"name": "--motion_build", "type": str, "default": "host", "choices": ["host", "device"],
         "help": "how the clips of a --motion_file pickle are built, at the first load and at every resample: on the host in float64 "
                 "(clip_cache) or on the device in float32 (emloco_motion_build)"},
        {"name": "--network_path", "type": str, "default": "output/"},
        {"name": "--exp_name", "type": str, "default": "emloco"},
        {"name": "--epoch", "type": int, "default": 0},
        {"name": "--horovod", "action": "store_true", "default": False},
        {"name": "--small_terrain", "action": "store_true", "default": False},
        {"name": "--random_heading", "action": "store_true", "default": False},
        {"name": "--init_heading", "action": "store_true", "default": False},
        {"name": "--heading_inversion", "action": "store_true", "default": False},
        {"name": "--adjust_root_vel", "action": "store_true", "default": False},
        {"name": "--input_init_pose", "action": "store_true", "default": False},
        {"name": "--input_init_vel", "action": "store_true", "default": False},
        {"name": "--add_noise", "action": "store_true", "default": False},
        {"name": "--vru", "action": "store_true", "default": False},
        {"name": "--real_path", "type": str, "default": ""},
        {"name": "--real_mesh", "action": "store_true", "default": False},
        {"name": "--valuenet_path", "type": str, "default": ""},
        {"name": "--follow", "action": "store_true", "default": False},
        {"name": "--server_mode", "action": "store_true", "default": False},
        {"name": "--pred_path", "action": "store_true", "default": False},
        {"name": "--pred_traj_file", "type": str, "default": ""},       # the table --pred_path walks (default: cfg env.pred_traj_data, then data/traj/traj_pred_data.pkl)
        {"name": "--real_traj_file", "type": str, "default": ""},       # the tables --real_path walks, comma-separated (default: cfg env.traj_data)
        {"name": "--no_virtual_display", "action": "store_true", "default": True},
        {"name": "--show_sensors", "action": "store_true", "default": False},
        {"name": "--add_proj", "action": "store_true", "default": False},
        # the training driver (run.py; CommonAgent.train, common_agent.py:151-273)
        {"name": "--experiment", "type": str, "default": "",
         "help": "name of the run: checkpoints and NAME_log.jsonl go to --network_path/NAME (turns the game statistics on)"},
        {"name": "--max_iterations", "type": int, "default": 0, "help": "number of training epochs (instead of --steps)"},
        {"name": "--save_freq", "type": int, "default": 200, "help": "a checkpoint every K epochs, an intermediate one every 5 K"},
        {"name": "--resume", "action": "store_true", "default": False,
         "help": "continue --experiment from its checkpoint: network, optimiser state, learning-rate schedule, epoch and frame numbering "
                 "carry on and the log is appended.  The simulator's state and the random streams are not restored: a valid continuation "
                 "of the run, not a bit-identical one"},
        {"name": "--stats", "action": "store_true", "default": False, "help": "game statistics and the per-epoch line without --experiment"},
    ]
    args = gymutil.parse_arguments(description="EmLoco rollout on MI355X", custom_parameters=custom_parameters, argv=argv)
    args.device_id = args.compute_device_id
    args.device = args.sim_device_type if args.use_gpu_pipeline else "cpu"
    return args


def load_cfg(args):
    with open(args.cfg_env, "r") as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    if args.num_envs > 0:
        cfg["env"]["numEnvs"] = args.num_envs            # config.py:72-73
    if args.episode_length > 0:
        cfg["env"]["episodeLength"] = args.episode_length
    cfg["name"] = args.task
    cfg["headless"] = args.headless
    cfg["env"]["motion_file"] = args.motion_file
    cfg["env"]["motion_build"] = getattr(args, "motion_build", "host")
    if getattr(args, "pred_traj_file", ""):
        cfg["env"]["pred_traj_data"] = args.pred_traj_file
    if getattr(args, "real_traj_file", ""):
        cfg["env"]["traj_data"] = [p for p in args.real_traj_file.split(",") if p]
    cfg["args"] = args
    cfg_train = {"params": {"config": {"player": {"use_pose": args.input_init_pose, "use_vel": args.input_init_vel}}},
                 "seed": args.seed}
    return cfg, cfg_train, args.network_path


def parse_sim_params(args, cfg, cfg_train=None):
    sim_params = gymapi.SimParams()
    sim_params.dt = SIM_TIMESTEP
    sim_params.num_client_threads = args.slices
    sim_params.physx.solver_type = 1
    sim_params.physx.num_position_iterations = 4
    sim_params.physx.num_velocity_iterations = 0
    sim_params.physx.num_threads = 4
    sim_params.physx.use_gpu = args.use_gpu
    sim_params.physx.num_subscenes = args.subscenes
    sim_params.use_gpu_pipeline = args.use_gpu_pipeline
    if "sim" in cfg:
        gymutil.parse_sim_config(cfg["sim"], sim_params)
    if args.num_threads > 0:
        sim_params.physx.num_threads = args.num_threads
    return sim_params

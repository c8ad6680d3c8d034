"""CPU-only: the host side of the get-up task -- the `pre_epoch` schedule, the task registry, the configuration file and the
hand-written mirror of EmlocoGetupBufs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest
import yaml

from emloco_amd import _abi, _lib as L

CFG = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "data", "cfg")
GETUP_KEYS = dict(getup_schedule=True, recoverySteps=60, recoveryEpisodeProb=0.2, fallInitProb=0.1)


class _Task:
    """what pre_epoch touches of HumanoidPedestrianTerrainGetup: the schedule's own code, on a stub"""
    has_shape_variation = False
    getup_schedule = True

    def __init__(self):
        self._recovery_episode_prob_tgt = self._recovery_episode_prob = 0.2
        self._fall_init_prob_tgt = self._fall_init_prob = 0.1

    from emloco_amd.env.tasks.humanoid_pedestrain_terrain_getup import HumanoidPedestrianTerrainGetup as _T
    update_getup_schedule = _T.update_getup_schedule


@pytest.mark.parametrize("epoch, weights, probs", [(1, (0, 1), (0, 1)), (10000, (0, 1), (0, 1)), (10001, (0.5, 0.5), (0.2, 0.1))])
def test_pre_epoch_follows_the_getup_schedule(epoch, weights, probs):
    from emloco_amd.learning.pre_epoch import pre_epoch
    task, agent = _Task(), types.SimpleNamespace(_task_reward_w=0.7, _disc_reward_w=0.3)
    assert pre_epoch(task, epoch, say=None, agent=agent) is False            # (no resampling: the return value speaks of that alone)
    assert (agent._task_reward_w, agent._disc_reward_w) == weights
    assert (task._recovery_episode_prob, task._fall_init_prob) == probs
    # without an agent the task alone follows; the schedule goes back and forth with the epoch
    task = _Task()
    pre_epoch(task, epoch, say=None)
    assert (task._recovery_episode_prob, task._fall_init_prob) == probs
    pre_epoch(task, 20000, say=None)
    assert (task._recovery_episode_prob, task._fall_init_prob) == (0.2, 0.1)


def test_pre_epoch_leaves_a_task_without_the_schedule_alone():
    from emloco_amd.learning.pre_epoch import pre_epoch
    for task in (types.SimpleNamespace(has_shape_variation=False), types.SimpleNamespace(has_shape_variation=False, getup_schedule=False)):
        before = dict(vars(task))
        agent = types.SimpleNamespace(_task_reward_w=0.7, _disc_reward_w=0.3)
        assert pre_epoch(task, 5, say=None, agent=agent) is False
        assert vars(task) == before and (agent._task_reward_w, agent._disc_reward_w) == (0.7, 0.3)


def test_amp_agent_hands_itself_to_pre_epoch():
    from emloco_amd.learning.amp_agent import AMPAgent
    agent = types.SimpleNamespace(task=_Task(), _task_reward_w=0.7, _disc_reward_w=0.3)
    AMPAgent.pre_epoch(agent, 3)
    assert (agent._task_reward_w, agent._disc_reward_w) == (0, 1) and agent.task._fall_init_prob == 1
    AMPAgent.pre_epoch(agent, 10001)
    assert (agent._task_reward_w, agent._disc_reward_w) == (0.5, 0.5) and agent.task._fall_init_prob == 0.1


def test_parse_task_knows_the_task():
    from emloco_amd.env.tasks.humanoid_pedestrain_terrain import HumanoidPedestrianTerrain
    from emloco_amd.env.tasks.humanoid_pedestrain_terrain_getup import HumanoidPedestrianTerrainGetup
    from emloco_amd.utils.parse_task import TASKS
    assert TASKS["HumanoidPedestrianTerrainGetup"] is HumanoidPedestrianTerrainGetup
    assert issubclass(HumanoidPedestrianTerrainGetup, HumanoidPedestrianTerrain) and TASKS["HumanoidPedestrianTerrain"] is HumanoidPedestrianTerrain


def test_getup_configuration_is_pacer_yaml_plus_the_four_keys():
    base = yaml.safe_load(open(os.path.join(CFG, "pacer.yaml")))
    getup = yaml.safe_load(open(os.path.join(CFG, "pacer_getup.yaml")))
    assert {k: getup["env"].pop(k) for k in GETUP_KEYS} == GETUP_KEYS
    assert getup == base
    from emloco_amd.utils.config import get_args, load_cfg
    cfg, _, _ = load_cfg(get_args(["--task", "HumanoidPedestrianTerrainGetup", "--cfg_env", os.path.join(CFG, "pacer_getup.yaml"), "--num_envs", "8"]))
    assert cfg["env"]["recoverySteps"] == 60 and cfg["env"]["getup_schedule"] is True and cfg["env"]["numEnvs"] == 8


def test_launch_arrangements_are_refused_without_a_device():
    """the switches are properties of the class: off reads False and may be set to False, on raises and says why"""
    from emloco_amd.env.tasks.humanoid_pedestrain_terrain_getup import HumanoidPedestrianTerrainGetup as T
    task = T.__new__(T)
    for name in ("fused_chain", "overlap_obs", "overlap_reset"):
        assert getattr(task, name) is False
        setattr(task, name, False)
        with pytest.raises(RuntimeError, match=f"sequential launch arrangement: {name}"):
            setattr(task, name, True)
    with pytest.raises(RuntimeError, match="sequential launch arrangement.*attach_returns"):
        task.attach_returns(object())
    task.attach_returns(None)


def test_getup_bufs_mirror_follows_the_header(tmp_path):
    """EmlocoGetupBufs is a tagged structure (the untagged ones are held to their mirrors by tests/test_abi_cpu.py): field by field
    against the header's text, and the compiler's size"""
    body = re.search(r"typedef\s+struct\s+EmlocoGetupBufs\s*\{([^{}]*)\}\s*EmlocoGetupBufs\s*;", _abi.source("emloco_task.h")).group(1)
    fields = []
    for decl in filter(str.strip, body.split(";")):
        first, *more = decl.replace("*", " * ").split(",")
        base, *first = [w for w in first.split() if w != "const"]
        for d in [first] + [m.split() for m in more]:
            fields.append((d[-1], "ptr" if "*" in d else _abi.SCALARS[base]))
    assert [(f, "ptr" if t is C.c_void_p else t) for f, t in L.GetupBufs._fields_] == fields
    consts = dict(re.findall(r"\b(EMLOCO_GETUP_\w+)\s*=?\s+(\d+)", open(os.path.join(_abi.INCLUDE, "emloco_task.h")).read()))
    consts.update(re.findall(r"\b(EMLOCO_GETUP_STAT_\w+) = (\d+)", open(os.path.join(_abi.INCLUDE, "emloco_task.h")).read()))
    for py in ("GETUP_STATS", "GETUP_STAT_RECOVER", "GETUP_STAT_FALL", "GETUP_STAT_NORMAL", "GETUP_STAT_COUNTER_SUM", "GETUP_STAT_FLAG_CALLS",
               "GETUP_STAT_HELD"):
        assert getattr(L, py) == int(consts["EMLOCO_" + py]), py
    if shutil.which("gcc") is None:
        return
    (tmp_path / "size.c").write_text('#include "emloco_task.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(EmlocoGetupBufs)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "size"), str(tmp_path / "size.c")])
    assert int(subprocess.check_output([str(tmp_path / "size")], text=True)) == C.sizeof(L.GetupBufs)


def test_the_four_entry_points_are_declared_and_bound():
    protos = _abi.prototypes()
    vp, ci, cf, u32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_uint64
    assert protos["emloco_getup_split"] == (ci, [vp, vp, ci, vp, u64, cf, cf, ci, u32, vp, vp, vp, vp, vp])
    assert protos["emloco_getup_apply"] == (ci, [vp, vp, vp, vp, vp, vp, ci, vp, vp, u64, vp, vp])
    assert protos["emloco_getup_amp_default"] == (ci, [vp, vp, ci, vp])
    assert protos["emloco_getup_flags"] == (ci, [vp, vp])
    lib = L.load()
    assert all(hasattr(lib, n) for n in ("emloco_getup_split", "emloco_getup_apply", "emloco_getup_amp_default", "emloco_getup_flags"))

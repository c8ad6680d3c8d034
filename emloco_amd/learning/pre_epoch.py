"""`pre_epoch` of the reference's AMP agent (pacer/pacer/learning/amp_continuous.py:203-220), which its value agent inherits: the task's
motion clips are redrawn every `shape_resampling_interval` epochs (:205-210), and a task with `getup_schedule` (HumanoidPedestrianTerrainGetup
under pacer_getup.yaml) follows the get-up schedule (:212-220): up to epoch 10000 every reset starts from a fallen pose and the agent is
rewarded by the discriminator alone (task / discriminator reward weights 0 / 1); beyond it the task's configured probabilities hold and
the weights are 0.5 / 0.5."""

GETUP_UPDATE_EPOCH = 10000


def getup_schedule(task, epoch_num, agent=None):
    """amp_continuous.py:212-220 for a task whose `getup_schedule` is set; anything else is left alone.  `agent` (optional): the object
    whose `_task_reward_w` / `_disc_reward_w` the rollout reads every epoch (AMPAgent).  True when the schedule was applied."""
    if not getattr(task, "getup_schedule", False):
        return False
    task.update_getup_schedule(epoch_num, getup_udpate_epoch=GETUP_UPDATE_EPOCH)
    if agent is not None:
        if epoch_num > GETUP_UPDATE_EPOCH:
            agent._task_reward_w, agent._disc_reward_w = 0.5, 0.5
        else:
            agent._task_reward_w, agent._disc_reward_w = 0, 1
    return True


def pre_epoch(task, epoch_num, say=print, agent=None):
    """To be called at the top of every epoch with that epoch's number -- the reference counts the first epoch as 1.  Resamples when the
    task has `has_shape_variation`, `epoch_num > 0` and `epoch_num % shape_resampling_interval == 0`; an interval of 0 switches it
    off.  True when the task was asked to resample.  The get-up schedule (see above) follows for a task that has it set; without
    `getup_schedule` nothing else changes."""
    interval = int(getattr(task, "shape_resampling_interval", 0) or 0)
    resampled = False
    if getattr(task, "has_shape_variation", False) and interval > 0 and epoch_num > 0 and epoch_num % interval == 0:
        info = task.resample_motions()
        if info is not None:                 # None: a motion library that is built once (MotionLibSynthetic)
            say(f"epoch {epoch_num}: resampled motions: {info['distinct_clips']} distinct clips for {info['num_motions']} envs in "
                f"{info['seconds']:.3f} s ({info['build']} build" + (", frame arrays reallocated)" if info["reallocated"] else ")"))
        resampled = True
    getup_schedule(task, epoch_num, agent)
    return resampled

"""`pre_epoch` of the reference's AMP agent (pacer/pacer/learning/amp_continuous.py:203-210), which its value agent inherits: the task's
motion clips are redrawn every `shape_resampling_interval` epochs.  The getup schedule of the same hook is not part of this project."""


def pre_epoch(task, epoch_num, say=print):
    """To be called at the top of every epoch with that epoch's number -- the reference counts the first epoch as 1.  Resamples when the
    task has `has_shape_variation`, `epoch_num > 0` and `epoch_num % shape_resampling_interval == 0`; an interval of 0 switches it
    off.  True when the task was asked to resample."""
    interval = int(getattr(task, "shape_resampling_interval", 0) or 0)
    if not getattr(task, "has_shape_variation", False) or interval <= 0 or epoch_num <= 0 or epoch_num % interval != 0:
        return False
    info = task.resample_motions()
    if info is not None:                 # None: a motion library that is built once (MotionLibSynthetic)
        say(f"epoch {epoch_num}: resampled motions: {info['distinct_clips']} distinct clips for {info['num_motions']} envs in "
            f"{info['seconds']:.3f} s ({info['build']} build" + (", frame arrays reallocated)" if info["reallocated"] else ")"))
    return True

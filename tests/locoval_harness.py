"""TEST INFRASTRUCTURE ONLY: the game state of the LocoVal evaluation for the tests that drive its kernels themselves -- on host arrays
for the CPU emulator (tests/emu), on a torch device for the library.  The buffers and the two structs come from the product's own tables
and builders (emloco_amd/learning/locoval_eval.py: EVAL_BUFFERS, TRACK_BUFFERS, eval_state, track_state), so a test holds the state the
evaluator holds.  Also the one pointer helper and the size table of the four LocoVal networks, shared by the CPU and the GPU tests.
"""
import ctypes as C

import numpy as np

from emloco_amd.learning import locoval_eval as LE

# variant ((use_pose << 1) | use_vel) -> (inputs, hidden 1, hidden 2, parameters)
DIMS = {3: (100, 49, 24, 6174), 2: (98, 48, 24, 5953), 1: (28, 13, 6, 468), 0: (26, 12, 6, 409)}


def _addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _ptr(a):
    """A numpy array or a torch tensor as a pointer argument; None is NULL."""
    return None if a is None else C.c_void_p(_addr(a))


def _zeros(device):
    if device is None:
        return lambda shape, dt: np.zeros(shape, dt)
    import torch
    return lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device=device)


def eval_state(E, G, step_to_pred=144, gamma=0.99, device=None, **inputs):
    """(EmlocoLocoValEval, {field: array}) of E envs that record G games each; numpy arrays, or torch tensors on `device`.  inputs: the
    test's own waypoint_traj / init_pose / init_vel (zeros otherwise); they are kept in the dict beside the buffers."""
    zeros = _zeros(device)
    assert set(inputs) <= {k for k, _ in LE.EVAL_INPUTS}, inputs.keys()
    inputs = {k: inputs[k] if k in inputs else zeros((E, *shape), "float32") for k, shape in LE.EVAL_INPUTS}
    st, b = LE.eval_state(E, step_to_pred, G, gamma, inputs, zeros, _addr)
    b.update(inputs)
    return st, b


def track_state(case, device=None):
    """(EmlocoLocoValTrack, {field: array}) for a case of tests/track_cases.py; root_pos / traj_verts / progress_buf are the caller's to set."""
    from track_cases import ROOT_STRIDE
    return LE.track_state(case["E"], _zeros(device), _addr, stride=case["stride"], root_stride=ROOT_STRIDE, dt=float(case["dt"]),
                          traj_dur=float(case["traj_dur"]))

"""The split launch's hand-over on the CPU emulator (tests/emu, the plain C++ variants of the hand-over helpers in
emloco_amd/csrc/sim_kernels.hip): 2 and 4 parts per env against the one-part launch from the same initial state, bit for bit,
with uneven load -- one env airborne, one standing, one lying with more than 14 contacts (packed contact matrix).  The same
check runs on the device in tests/test_gpu_sim_handover.py.
"""
import numpy as np
import pytest

import emu
from helpers import oracle_sim, scene_state, varied_models

NAMES = ("root_state", "dof_state", "rb_state", "contact_force", "dof_force", "lambda_ws")
STEPS = 3


def _scene():
    E = 3
    models = varied_models(E, seed=61)
    root, dof, tgt = scene_state(E, seed=62, perturbed_from=0)
    root[0, 2] = 3.0                                            # airborne
    dof[1] = 0.0                                                # standing
    root[1, 7:13] *= 0.25
    s = np.float32(np.sin(np.pi / 4))
    root[2, 2] = 0.06                                           # lying on its back, pressed into the ground
    root[2, 3:7] = [s, 0.0, 0.0, s]
    return models, root, dof, tgt


def _run(scene, keys=None):
    """every step's arrays; `keys` takes the contact-work key of each step (sum over its 4 substeps of 10 + contacts, 0 without any)"""
    models, root, dof, tgt = scene
    sim = oracle_sim(models, root, dof, tgt, self_collision=True, n_sub=4)
    out = []
    for k in range(STEPS):
        emu.sim_step(sim, 1, cost_ticks=None if keys is None else keys[k])
        out.append([getattr(sim, n).copy() for n in NAMES])
    return out


@pytest.fixture(scope="module")
def one_part():
    import os
    assert "EMLOCO_EMU_PARTS" not in os.environ
    scene = _scene()
    keys = np.zeros((STEPS, 3), np.uint32)
    ref = _run(scene, keys)
    assert (keys[:, 0] == 0).all(), "env 0 is airborne"
    assert (keys[1:, 1] > 0).all(), "env 1 stands on its feet (it starts a few millimetres above the ground)"
    assert keys[:, 2].max() > 4 * (10 + 14), "env 2 lies on more than 14 contacts"
    return scene, ref


@pytest.mark.parametrize("parts", [2, 4])
def test_emulated_split_launch_equals_the_one_part_launch(parts, one_part, monkeypatch):
    scene, ref = one_part
    monkeypatch.setenv("EMLOCO_EMU_PARTS", str(parts))
    got = _run(scene)
    for k in range(STEPS):
        for name, a, b in zip(NAMES, got[k], ref[k]):
            assert np.array_equal(a, b), f"parts={parts} step {k} {name}"
    assert np.isfinite(ref[-1][2]).all()

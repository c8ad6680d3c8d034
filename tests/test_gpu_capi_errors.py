"""Refusals leave no trace on the device: two identical simulators, one of them refused again and again between its launches (by the
simulator, the task and the get-up units, each with its code and a text that names the call), step the same bytes -- down the three
paths of the step launch: every env, everything but the flagged envs, an id list.  Two envs, flat ground, no split, n_calls = 1."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_abi_cases as S                                                        # noqa: E402

SEVEN = ("root_state", "dof_state", "rigid_body_state", "contact_force", "dof_force", "pd_target", "warm_start")
OK, E_ARG = 0, -1


def _refused(lib, rc, name):
    assert rc == E_ARG, (name, rc, lib.emloco_last_error())
    assert name.encode() in lib.emloco_last_error(), (name, lib.emloco_last_error())


def _refusals(sim):
    """argument refusals only: nothing below reaches a launch"""
    lib, h, st = sim.lib, sim._h, sim._stream()
    _refused(lib, lib.emloco_sim_step_subset(h, 1, None, None, 0, st), "emloco_sim_step_subset")      # neither skip flags nor an id list
    _refused(lib, lib.emloco_sim_step(h, 0, st), "emloco_sim_step")                                   # n_calls = 0
    _refused(lib, lib.emloco_task_reset(h, None, None, 0, None, st), "emloco_task_reset")             # task unit: no buffers
    _refused(lib, lib.emloco_getup_apply(h, None, None, None, None, None, 0, None, None, 0, None, st), "emloco_getup_apply")   # get-up unit
    assert lib.emloco_sim_sync(h, st) == OK                                                          # and no error word was raised


def test_refusals_between_launches_leave_no_trace():
    from emloco_amd import _lib as L
    from emloco_amd.sim import NativeSim
    E = 2
    models, root, dof, tgt = S.split_scene(E)
    sims = [NativeSim(models, L.default_sim_params(n_sub=2)) for _ in range(2)]
    try:
        a, b = sims
        for s in sims:
            s.root_state.copy_(torch.from_numpy(root))
            s.dof_state.view(E, 69, 2).copy_(torch.from_numpy(dof))
            s.pd_target.copy_(torch.from_numpy(tgt))
            s.refresh_bodies()
        skip = torch.zeros(E, dtype=torch.int64, device=a.device)
        ids = torch.tensor([1], dtype=torch.int32, device=a.device)
        _refusals(a)
        for s in sims:
            s.step(1)
        _refusals(a)
        for s in sims:
            s.step_subset(1, skip=skip)
        _refusals(a)
        for s in sims:
            s.step_subset(1, ids=ids)
        _refusals(a)
        for s in sims:
            s.sync()
        for name in SEVEN:
            x, y = getattr(a, name).contiguous().view(torch.int32), getattr(b, name).contiguous().view(torch.int32)
            assert torch.equal(x, y), f"{name}: the refused simulator differs"
        assert not torch.equal(a.root_state.cpu(), torch.from_numpy(root))          # (the launches ran)
    finally:
        for s in sims:
            s.close()

"""The part plan of the rigid-body launch (emloco_sim_set_plan) on the device.

Companion of tests/test_sim_plan_cpu.py (builder, checker and the emulated kernel).  Here the workgroups of a plan really run beside
each other: at 700 envs plan T is 3500 one-wave workgroups on 3072 wave slots, so later parts queue for a slot and consumers meet
hand-overs that are still being written.  Every plan must leave the six state buffers (and the cost key, when the cost order is on)
on the bytes of the one-part launch, emloco_sim_set_split(1), of a second simulator that is fed the same writes: six steps back to
back, with an indexed write of root and joint state between the third and the fourth.  Class boundaries are no multiples of 64 (467
of 700).  The plans are those of tests/sim_plan_cases.py: T, C, S (one stage behind), S- (one stage ahead), T+C.

What the public ABI cannot show is the launch geometry itself, so "set_split after set_plan restores the uniform launch" is held by
what can be seen: the call succeeds, the steps after it stay on the reference's bytes, and a plan can be set again.  No lost
hand-over is provoked here; tests/test_gpu_sim.py has the one device case."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_abi_cases as S                                                        # noqa: E402
import sim_plan_cases as P                                                       # noqa: E402

STEPS, WRITE_BEFORE = 6, 3
OK, E_ARG, E_STATE = 0, -1, -3
SIX = (("root_state", "root_state"), ("dof_state", "dof_state"), ("rb_state", "rigid_body_state"), ("contact_force", "contact_force"),
       ("dof_force", "dof_force"), ("lambda_ws", "warm_start"))


@functools.lru_cache(maxsize=None)
def _scene(n_env):
    return S.split_scene(n_env)


def _native(n_env):
    from emloco_amd import _lib as L
    from emloco_amd.sim import NativeSim
    models, root, dof, tgt = _scene(n_env)
    g = NativeSim(models, L.default_sim_params(n_sub=P.N_SUB), self_collision=True)
    g.root_state.copy_(torch.from_numpy(root))
    g.dof_state.view(n_env, 69, 2).copy_(torch.from_numpy(dof))
    g.pd_target.copy_(torch.from_numpy(tgt))
    g.refresh_bodies()
    return g


def _indexed_write(g, n_env):
    """every third env is set down again, turned and spun, through the indexed setters (their forward kinematics included)"""
    ids = torch.arange(0, n_env, 3, dtype=torch.int32, device=g.device)
    rows = ids.long()
    g.root_state[rows, 2] = 1.1
    g.root_state[rows, 7:13] = 0.3
    g.dof_state.view(n_env, 69, 2)[rows, :, 1] *= -0.5
    g.set_root_state_indexed(g.root_state, ids)
    g.set_dof_state_indexed(g.dof_state, ids)


def _snapshot(g, ordered):
    torch.cuda.synchronize()
    out = {name: getattr(g, attr).cpu().numpy().copy() for name, attr in SIX}
    if ordered:
        keys = np.zeros(g.num_envs, np.uint32)
        assert g.lib.emloco_sim_cost_ticks(g._h, keys.ctypes.data, None, g.num_envs) == OK
        out["step_ticks"] = keys
    return out


def _rollout(g, n_env, ordered, before_step=None):
    g.set_cost_order(ordered)
    out = []
    for t in range(STEPS):
        if t == WRITE_BEFORE:
            _indexed_write(g, n_env)
        if before_step is not None:
            before_step(g, t)
        g.step(1)
        out.append(_snapshot(g, ordered))
    g.sync()
    return out


@functools.lru_cache(maxsize=None)
def _reference(n_env, ordered):
    """the one-part launch, once per scene; shared by the plans and read only"""
    g = _native(n_env)
    g.set_split(1)
    ref = _rollout(g, n_env, ordered)
    g.close()
    assert np.isfinite(ref[-1]["rb_state"]).all() and (n_env == 1 or np.abs(ref[-1]["contact_force"]).max() > 0)
    for step in ref:
        for v in step.values():
            v.setflags(write=False)
    return ref


def _same(ref, got, what):
    for t in range(STEPS):
        for k, v in ref[t].items():
            assert np.array_equal(v, got[t][k]), f"{what}: step {t} {k} differs from the one-part launch, max abs diff {np.abs(v.astype(np.float64) - got[t][k]).max():.3e}"


@pytest.mark.parametrize("name", ["T", "C", "S", "S-", "T+C"])
@pytest.mark.parametrize("ordered", [False, True], ids=["rank_is_env", "cost_order"])
@pytest.mark.parametrize("n_env", [1, 3, 700])
def test_a_launch_under_a_plan_is_the_one_part_launch(n_env, ordered, name):
    classes, tail, shift = P.plans(n_env)[name]
    assert n_env < 64 or all(lo % 64 and hi % 64 for lo, hi, _ in classes[1:])           # class boundaries off the wave size
    g = _native(n_env)
    g.set_plan(classes, tail, shift)
    got = _rollout(g, n_env, ordered)
    g.close()
    _same(_reference(n_env, ordered), got, f"plan {name}, {n_env} envs")


def test_plans_can_be_switched_between_steps():
    """plan T+C -> set_split(4) -> plan S -> set_split(2) -> plan T, a step or two under each"""
    n_env = 700
    todo = {0: lambda g: g.set_plan(*P.plans(n_env)["T+C"]), 2: lambda g: g.set_split(4), 3: lambda g: g.set_plan(*P.plans(n_env, 100)["S"]),
            4: lambda g: g.set_split(2), 5: lambda g: g.set_plan(*P.plans(n_env)["T"])}
    g = _native(n_env)
    got = _rollout(g, n_env, True, before_step=lambda g, t: todo[t](g) if t in todo else None)
    g.close()
    _same(_reference(n_env, True), got, "switching plans")


def test_skip_flags_and_the_id_list_under_a_plan():
    """the step as two launches (emloco_sim_step_subset): everything but the flagged envs under the plan, the flagged ones by an
    unsplit list launch"""
    n_env = 700
    g, r = _native(n_env), _native(n_env)
    r.set_split(1)
    g.set_plan(*P.plans(n_env)["T+C"])
    g.set_cost_order(True)
    for t in range(3):
        flagged = [e for e in range(n_env) if (e * 7 + t) % 5 == 0]
        skip = torch.zeros(n_env, dtype=torch.int64, device=g.device)
        skip[flagged] = 1
        ids = torch.full((n_env,), -1, dtype=torch.int32, device=g.device)
        ids[:len(flagged)] = torch.tensor(flagged, dtype=torch.int32)
        g.step_subset(1, skip=skip)
        g.step_subset(1, ids=ids)
        r.step(1)
        torch.cuda.synchronize()
        for nm, attr in SIX:
            assert torch.equal(getattr(g, attr), getattr(r, attr)), f"step {t}: {nm}"
    g.sync()
    g.close(); r.close()


def _refused(lib, rc, code, names):
    assert rc == code, (rc, code, lib.emloco_last_error())
    msg = lib.emloco_last_error()
    assert msg and any(n.encode() in msg for n in names), (msg, names)


def test_set_plan_refusals_and_set_split_beside_a_plan():
    from emloco_amd import _lib as L
    lib = L.require_device()
    n_env = 13
    name = ["emloco_sim_set_plan"]
    one = P.flat([(0, n_env, 4)])
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    # not prepared
    h = C.c_void_p()
    params = L.default_sim_params()
    assert lib.emloco_sim_create(C.byref(params), 0, C.byref(h)) == OK
    try:
        _refused(lib, lib.emloco_sim_set_plan(h, ptr(one), 1, 1, 0, 1), E_STATE, name)
    finally:
        lib.emloco_sim_destroy(h)
    _refused(lib, lib.emloco_sim_set_plan(None, ptr(one), 1, 1, 0, 1), E_ARG, name)
    g = _native(n_env)
    r = _native(n_env)
    r.set_split(1)
    g.set_plan([(0, n_env, 4)], 1, 0)
    for classes, tail, shift in (([(0, 8, 4), (6, 13, 2)], 0, 0), ([(0, 8, 4), (13, 8, 2)], 0, 0), ([(5, 13, 4), (0, 5, 2)], 0, 0),
                                 ([(0, 12, 4)], 0, 0), ([(0, 13, 3)], 0, 0), ([(0, 13, 4)], 2, 0), ([(0, 13, 4)], 0, 5)):
        c = P.flat(classes)
        _refused(lib, lib.emloco_sim_set_plan(g._h, ptr(c), len(c), tail, shift, 1), E_ARG, name)
    _refused(lib, lib.emloco_sim_set_plan(g._h, None, 1, 0, 0, 1), E_ARG, name)
    _refused(lib, lib.emloco_sim_set_plan(g._h, ptr(one), 0, 0, 0, 1), E_ARG, name)
    _refused(lib, lib.emloco_sim_set_plan(g._h, ptr(one), 1, 0, 0, 0), E_ARG, name)         # n_calls
    _refused(lib, lib.emloco_sim_set_plan(g._h, ptr(one), 1, 0, 0, 2), E_ARG, name)         # 4 x 2 substeps: beyond the plan word
    _refused(lib, lib.emloco_sim_set_split(g._h, 5), E_ARG, ["emloco_sim_set_split"])       # five parts stay refused beside a five-workgroup plan
    _refused(lib, lib.emloco_sim_set_split(g._h, 0), E_ARG, ["emloco_sim_set_split"])

    def both(what):
        g.step(1); r.step(1)
        torch.cuda.synchronize()
        for nm, attr in SIX:
            assert torch.equal(getattr(g, attr), getattr(r, attr)), f"{what}: {nm}"

    both("plan T after the refusals")                 # the plan in force was kept
    g.set_split(4)                                    # clears the plan: the uniform launch
    both("set_split(4) after a plan")
    g.set_split(1)
    both("set_split(1) after a plan")
    g.set_plan(*P.plans(n_env)["T+C"])
    both("a plan set again")
    # a step of another substep count than the plan's runs as the uniform split
    g.step(2); r.step(2)
    torch.cuda.synchronize()
    for nm, attr in SIX:
        assert torch.equal(getattr(g, attr), getattr(r, attr)), f"n_calls = 2 under a plan: {nm}"
    g.sync(); r.sync()
    g.close(); r.close()

"""The split launch's hand-over on the device (through the C ABI): the substeps of a step as 2 or 4 dependent workgroups per env,
each continuing from the self-tagged granules its predecessor stored (sim_kernels.hip: part_ld80), against the ONE-part launch
from the same initial state -- bit equality on every state tensor after every step.

Sizes: 1 and 3 envs; 700 (2800 workgroups: every part resident at once, successors poll while their predecessors run) and 1024
(4096 workgroups on 3072 wave slots: successors queue behind running predecessors and find the granules complete -- or, with the
cost order off, not yet).  Load uneven on purpose: a third of the envs airborne (no contact), a third standing, a third lying on
the ground (>= 10 contacts, some above 14: the packed contact matrix).  Six steps go out back to back without a host
synchronisation (the per-step snapshots are device-side copies on the same stream), so the tags of consecutive launches meet in
the same hand-over buffer.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STEPS = 6
NAMES = ("root_state", "dof_state", "rigid_body_state", "contact_force", "dof_force", "warm_start")


def _kind(e):
    return (e + 2) % 3                 # 0: airborne, 1: standing, 2: lying (env 0 lies: the one-env case runs the contact phases)


def _scene(E):
    from helpers import scene_state, varied_models
    base = varied_models(min(E, 48), seed=61)
    models = [base[e % len(base)] for e in range(E)]
    root, dof, tgt = scene_state(E, seed=62, perturbed_from=0)
    s = np.float32(np.sin(np.pi / 4))
    for e in range(E):
        k = _kind(e)
        if k == 0:
            root[e, 2] = 3.0
        elif k == 1:
            root[e, 7:13] *= 0.25
            dof[e] = 0.0
        else:
            root[e, 2] = 0.06                                      # on the back, pressed into the ground (joint angles differ per env)
            root[e, 3:7] = [s, 0.0, 0.0, s]
    return models, root, dof, tgt


def _sim(scene, parts, order):
    from emloco_amd import _lib as L
    from emloco_amd.sim import NativeSim
    models, root, dof, tgt = scene
    E = len(models)
    sim = NativeSim(models, L.default_sim_params(n_sub=2), self_collision=True)
    sim.root_state.copy_(torch.from_numpy(root))
    sim.dof_state.view(E, 69, 2).copy_(torch.from_numpy(dof))
    sim.pd_target.copy_(torch.from_numpy(tgt))
    sim.set_cost_order(order)
    sim.set_split(parts)
    return sim


def _run(sim):
    """STEPS steps of 4 substeps back to back; every step's tensors as device-side copies, read once at the end"""
    snaps = []
    for _ in range(STEPS):
        sim.step(2)
        snaps.append([getattr(sim, n).clone() for n in NAMES])
    sim.sync()
    return [[t.cpu().numpy() for t in row] for row in snaps]


_REF = {}


def _keys(scene):
    """contact-work key of every env in each of the steps (sum over a step's 4 substeps of 10 + contacts, 0 without any), read from a
    one-part simulator of its own after every step"""
    sim = _sim(scene, 1, True)
    E = sim.num_envs
    keys = np.zeros((STEPS, E), np.uint32)
    for k in range(STEPS):
        sim.step(2)
        assert sim.lib.emloco_sim_cost_ticks(sim._h, keys[k].ctypes.data, None, E) == 0
    return keys


def _reference(E):
    """the one-part launch, plain dispatch order: computed once per size, shared by the cases and left unchanged"""
    if E not in _REF:
        scene = _scene(E)
        _REF[E] = (scene, _run(_sim(scene, 1, False)), _keys(scene))
    return _REF[E]


@pytest.mark.parametrize("order", [False, True], ids=["index-order", "cost-order"])
@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("E", [1, 3, 700, 1024])
def test_split_launch_equals_the_one_part_launch(E, parts, order):
    scene, ref, _ = _reference(E)
    sim = _sim(scene, parts, order)
    got = _run(sim)
    for k in range(STEPS):
        for name, a, b in zip(NAMES, got[k], ref[k]):
            assert np.array_equal(a, b), f"E={E} parts={parts} step {k} {name}: {int((a.reshape(E, -1) != b.reshape(E, -1)).any(axis=1).sum())} envs differ"
    assert np.isfinite(ref[-1][2]).all()


@pytest.mark.parametrize("E", [1, 3, 700, 1024])
def test_the_load_is_uneven(E):
    """what the comparison above runs on: airborne envs without a contact, standing ones on their feet, lying ones on at least 10
    contacts in every substep of the first step and some of them on more than 14 (the packed contact matrix)"""
    keys = _reference(E)[2]
    kind = np.array([_kind(e) for e in range(E)])
    print(f"E={E}: first-step keys lying min {keys[0, kind == 2].min()} max {keys[0, kind == 2].max()}; per step max {keys.max(axis=1)}")
    assert (keys[:, kind == 0] == 0).all(), "airborne envs have no contact"
    assert (keys[0, kind == 2] >= 4 * (10 + 10)).all(), "lying envs: at least 10 contacts per substep"
    assert keys[0, kind == 2].max() > 4 * (10 + 14), "some lying env above 14 contacts"
    if E >= 3:
        assert (keys[1:, kind == 1].max(axis=0) > 0).all(), "standing envs touch the ground"


def test_second_simulator_in_recycled_memory_starts_from_untagged_granules():
    """A simulator takes ONE step at split 2 and is destroyed: every granule of its hand-over block carries the tag of part 0 of
    launch 1.  A second simulator of the same size then gets the block back from the allocator, and in ITS first launch part 1
    awaits exactly that tag -- at 3 envs all six workgroups are resident at once, so part 1 polls while part 0 still runs and
    would take the destroyed simulator's state whole.  emloco_sim_set_split zeroes the block (no tag is 0), so part 1 waits for
    its own predecessor and the result is the one-part launch's.  (With the zeroing taken out of sim_capi.hip this case fails
    on the first step's root_state; the block really is recycled.)"""
    E = 3
    scene = _reference(E)[0]
    models, root, dof, tgt = scene
    other = (models, root, dof * np.float32(0.5), tgt)          # the second simulator's hand-over differs from the first one's
    want = _run(_sim(other, 1, False))
    first = _sim(scene, 2, False)
    first.step(2)
    first.sync()
    first.close()                                               # emloco_sim_destroy: the block goes back to the allocator
    got = _run(_sim(other, 2, False))
    for k in range(STEPS):
        for name, a, b in zip(NAMES, got[k], want[k]):
            assert np.array_equal(a, b), f"step {k} {name}"

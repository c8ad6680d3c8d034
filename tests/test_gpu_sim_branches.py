"""Device twin of the new scenes of tests/sim_branch_cases.py: the scenes that take the kernel branches no earlier scene entered
(tests/test_sim_branches_cpu.py measures that on the CPU emulator) through `NativeSim` against the CPU oracle.

Bar: bit equality on root_state, dof_state, rb_state, contact_force, dof_force and the warm start after every control step, as
test_gpu_sim_matrix._compare has it.  Each scene runs with the launch split in 1 and in 3 parts and with the cost-ordered dispatch
off and on (which workgroup steps which env must not matter), and carries its float64 regime assertion: joint angle at or beyond pi,
root spin above the limit, a bit-equal pair of candidates at the 20th contact place, more limb-limb hits than slots, the closest-point
region on the mesh -- so the scene cannot drift out of the branch it was built for.  The oracle's run of a scene is computed once and
shared by its four launch variants.  Every scene is at most 8 envs and 2 control steps.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_branch_cases as B                                                     # noqa: E402
from test_gpu_sim_matrix import _compare, _load                                  # noqa: E402

CASES = {c.name: c for c in B.new_cases()}
_reference = {}


class _Frozen:
    """the oracle's six outputs after one control step, under the names _compare reads"""

    def __init__(self, osim):
        for name in B.NAMES:
            a = getattr(osim, name).copy()
            a.setflags(write=False)
            setattr(self, name, a)


def reference(name):
    """(scene, oracle outputs per control step) of a case; the regime and after-run assertions of the scene run here, once"""
    if name not in _reference:
        case = CASES[name]
        sc = case.scene()
        case.regime(sc)
        osim = case.oracle(sc)
        steps = []
        for _ in range(case.steps):
            osim.step(1)
            steps.append(_Frozen(osim))
        if case.after is not None:
            case.after(osim)
        assert np.isfinite(osim.rb_state).all()
        _reference[name] = (sc, steps)
    return _reference[name]


@pytest.mark.parametrize("cost_order", [False, True], ids=["plain", "cost_order"])
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_new_branch_scenes_are_bit_exact_vs_oracle(name, parts, cost_order):
    from emloco_amd import _lib as L
    from emloco_amd.sim import NativeSim
    case = CASES[name]
    assert case.new and case.regime is not None and case.pre_step is None and case.steps <= 4
    sc, steps = reference(name)
    assert sc["root"].shape[0] <= 8
    gsim = NativeSim(sc["models"], L.default_sim_params(n_sub=case.n_sub, **sc.get("params", {})), self_collision=sc.get("sc"),
                     heightfield=sc.get("hf"))
    _load(gsim, sc["root"], sc["dof"], sc["tgt"])
    gsim.set_split(parts)
    gsim.set_cost_order(cost_order)
    for t, want in enumerate(steps):
        gsim.step(case.n_calls)
        _compare(want, gsim, f"{name} parts={parts} cost_order={cost_order} step {t}")
    gsim.sync()

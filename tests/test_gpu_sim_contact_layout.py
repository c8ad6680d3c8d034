"""The two LDS layouts of the contact matrix (square up to 14 contacts, packed lower triangle above) on the device, through the
C ABI: the HIP step stays on the oracle's bytes through every contact-count regime, in the plane and the height-field
instantiation of the kernel, as one workgroup per env and as the 4-part split launch the task uses.  Same scenes, seeds and
coverage assertion as tests/test_emu_sim_contact_layout.py (tests/contact_layout_cases.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import contact_layout_cases as K


def _pair(ground, n_sub_oracle, n_sub_device):
    from emloco_amd import _lib as L
    from emloco_amd.model import pack_self_collision
    from emloco_amd.sim import NativeSim
    from helpers import oracle_sim
    models, root, dof, tgt = K.scene(ground)
    hf = K.heightfield() if ground == "hf" else None
    sc = pack_self_collision(models)
    osim = oracle_sim(models, root, dof, tgt, self_collision=sc, heightfield=hf, n_sub=n_sub_oracle)
    gsim = NativeSim(models, L.default_sim_params(n_sub=n_sub_device), self_collision=sc, heightfield=hf)
    gsim.root_state.copy_(torch.from_numpy(root))
    gsim.dof_state.view(K.E, 69, 2).copy_(torch.from_numpy(dof))
    gsim.pd_target.copy_(torch.from_numpy(tgt))
    return osim, gsim, hf


def _compare(osim, gsim, what):
    torch.cuda.synchronize()
    E = K.E
    for name, a, b in (("root_state", gsim.root_state, osim.root_state), ("dof_state", gsim.dof_state, osim.dof_state),
                       ("rb_state", gsim.rigid_body_state, osim.rb_state), ("contact_force", gsim.contact_force, osim.contact_force),
                       ("dof_force", gsim.dof_force, osim.dof_force), ("lambda_ws", gsim.warm_start, osim.lambda_ws)):
        a = a.cpu().numpy().reshape(b.shape)
        assert np.array_equal(a, b), f"{what} {name}: not bit-exact, max abs diff {np.abs(a - b).max():.3e}"


@pytest.mark.parametrize("ground", ["plane", "hf"])
def test_every_contact_count_regime_is_bit_exact_vs_oracle(ground):
    """Single-substep launches, compared after every step; the env-substeps run include 0, 1-10, 11-14, exactly 14, exactly 15
    and more than 20 candidates inside the contact offset (asserted from the oracle's body states)."""
    osim, gsim, hf = _pair(ground, 1, 1)
    osim.fk()
    cov = K.Coverage()
    for t in range(K.STEPS):
        cov.add(osim, hf)
        osim.step(1)
        gsim.step(1)
        _compare(osim, gsim, f"{ground} step {t}")
    cov.check()
    assert np.abs(osim.contact_force).max() > 50


@pytest.mark.parametrize("ground", ["plane", "hf"])
def test_split_launch_is_bit_exact_through_the_layout_switch(ground):
    """The task's launch: 2 x 2 substeps as four dependent workgroups per env; an env changes layout between the parts of one
    step as its contact count crosses 14."""
    osim, gsim, _ = _pair(ground, 4, 2)
    gsim.set_split(4)
    for t in range(3):
        osim.step(1)
        gsim.step(2)
        _compare(osim, gsim, f"{ground} split step {t}")
    assert np.abs(osim.contact_force).max() > 50

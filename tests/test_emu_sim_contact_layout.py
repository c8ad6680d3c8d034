"""The two LDS layouts of the contact matrix (square up to 14 contacts, packed lower triangle above) on the CPU emulator: the
emulated kernel stays on the oracle's bytes through every contact-count regime, on the plane and on a height field, with limb-limb
contacts on, as one workgroup per env and as the 4-part split launch.  Scenes and counting: tests/contact_layout_cases.py."""
import numpy as np
import pytest

import emu
import contact_layout_cases as K
from helpers import oracle_sim


def _pair(ground, n_sub):
    models, root, dof, tgt = K.scene(ground)
    hf = K.heightfield() if ground == "hf" else None
    a = oracle_sim(models, root, dof, tgt, self_collision=True, heightfield=hf, n_sub=n_sub)
    b = oracle_sim(models, root, dof, tgt, self_collision=True, heightfield=hf, n_sub=n_sub)
    return a, b, hf


@pytest.mark.parametrize("ground", ["plane", "hf"])
def test_every_contact_count_regime_is_bit_exact_vs_oracle(ground):
    """Single-substep steps, compared after every step; the env-substeps run include 0, 1-10, 11-14, exactly 14, exactly 15 and
    more than 20 candidates inside the contact offset (asserted from the oracle's body states)."""
    a, b, hf = _pair(ground, n_sub=1)
    a.fk()
    cov = K.Coverage()
    for t in range(K.STEPS):
        cov.add(a, hf)                                   # the contacts this step detects: at the state it starts from
        a.step(1)
        emu.sim_step(b, 1)
        for name in K.NAMES:
            assert np.array_equal(getattr(a, name), getattr(b, name)), (name, t)
        triples = (np.abs(a.lambda_ws).sum(-1) > 0).sum(1)
        assert (triples <= K.MAXC).all()
    cov.check()
    assert np.abs(a.contact_force).max() > 50


@pytest.mark.parametrize("ground", ["plane", "hf"])
def test_split_launch_is_bit_exact_through_the_layout_switch(ground, monkeypatch):
    """The same scenes as four dependent workgroups per env (one substep each): an env changes layout between the parts of
    one step as its contact count crosses 14."""
    monkeypatch.setenv("EMLOCO_EMU_PARTS", "4")
    a, b, _ = _pair(ground, n_sub=4)
    for t in range(2):
        a.step(1)
        emu.sim_step(b, 1)
        for name in K.NAMES:
            assert np.array_equal(getattr(a, name), getattr(b, name)), (name, t)
    assert np.abs(a.contact_force).max() > 50

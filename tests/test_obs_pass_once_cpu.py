"""The observation / reset kernels after the "evaluate once" change against what the build before it wrote, byte for byte, through the
emulator (the kernel sources compiled for the CPU) -- no GPU.

Cases, inputs and the comparison are those of tests/obs_pass_cases.py; tests/golden/obs_pass_parent.npz was recorded by
tests/golden/gen_obs_pass_parent.py on the commit before the change (its emulator build and its device build agreed on every byte).  The
change moves work between lanes: root, mirrored-root and head heading in one pass over three lanes, self and mirrored self observation in
one pass over 48 lanes, the centre probes' loads ahead of that pass, one sincos per joint in exp_map_to_quat, one slerp pass over 24 lanes
per AMP history row.  Every value comes out of the same operations in the same order, so there is no tolerance and no row is exempt."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_pass_cases as OC        # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_pass_parent.npz")


@pytest.fixture(scope="module")
def fx():
    return OC.Fixture(FIXTURE)


@pytest.fixture(scope="module")
def exe():
    return OC.EmuExecutor()


def test_the_recorded_inputs_are_the_cases(fx):
    """the state the recording was made on is the one make_inputs describes (the exact-axis headings, the mirrored pair, the joint
    branches); it is read from the file, not regenerated"""
    rb, dof = fx.inp["rb_state"], fx.inp["dof_state"]
    assert OC.same_bits(rb[4:8, 0, 3:7], OC.AXIS_Q) and OC.same_bits(rb[9], OC.mirror_env(rb[8]))
    hx, hy = OC.heading_xy(rb[4:8, 0, 3:7])
    assert hx.tolist() == [1.0, 1.0, -1.0, -1.0] and (hy == 0).all() and np.signbit(hy).tolist() == [False, True, False, True]
    assert (dof[10, 0:3, 0] == 0).all()


@pytest.mark.parametrize("n", [OC.E, OC.E_ODD])
@pytest.mark.parametrize("name", list(OC.POST_CASES))
def test_post_physics_kernel_writes_the_recorded_bytes(fx, exe, name, n):
    mode, ring, reset0, indexed = OC.POST_CASES[name]
    got = exe.post(fx.inp, n, mode, ring, reset0, OC.indexed_ids(n) if indexed else None)
    fx.check(name if n == OC.E else f"{name}@{n}", got)


@pytest.mark.parametrize("name", list(OC.CHAIN_CASES))
def test_reset_obs_kernel_writes_the_recorded_bytes(fx, exe, name):
    """the reset role (chain + 14 back-filled history rows of the finished envs) and the live role (observations, AMP shift + row of the
    others) of the fused launch"""
    n, ids, ring = OC.CHAIN_CASES[name]
    fx.check(name, exe.chain(fx.inp, n, np.asarray(ids, np.int32), ring, OC.LIVE))

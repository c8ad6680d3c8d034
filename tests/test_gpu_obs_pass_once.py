"""The observation / reset kernels after the "evaluate once" change against what the build before it wrote, byte for byte, on the device
through the C ABI (emloco_task_post_physics, emloco_task_reset_obs).

The device twin of tests/test_obs_pass_once_cpu.py: same cases (tests/obs_pass_cases.py), same recording
(tests/golden/obs_pass_parent.npz, made by tests/golden/gen_obs_pass_parent.py on the commit before the change, whose device build and
emulator build agreed on every byte), no tolerance, no row exempt.  On the device this also pins what the emulator cannot see: the maths
library's double-precision sincos against its separate sin and cos on the joint angles of exp_map_to_quat (a zero vector, 1e-6, pi,
pi - 1e-4 and 350 generic ones per launch), and the v_readlane broadcast of the three heading quaternions."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_pass_cases as OC        # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_pass_parent.npz")


@pytest.fixture(scope="module")
def fx():
    return OC.Fixture(FIXTURE)


@pytest.fixture(scope="module")
def exe():
    e = OC.DeviceExecutor()
    yield e
    e.close()


@pytest.mark.parametrize("n", [OC.E, OC.E_ODD])
@pytest.mark.parametrize("name", list(OC.POST_CASES))
def test_post_physics_kernel_writes_the_recorded_bytes(fx, exe, name, n):
    mode, ring, reset0, indexed = OC.POST_CASES[name]
    got = exe.post(fx.inp, n, mode, ring, reset0, OC.indexed_ids(n) if indexed else None)
    fx.check(name if n == OC.E else f"{name}@{n}", got)


@pytest.mark.parametrize("name", list(OC.CHAIN_CASES))
def test_reset_obs_kernel_writes_the_recorded_bytes(fx, exe, name):
    """the reset role (chain + 14 back-filled history rows of the finished envs) and the live role (observations, AMP shift + row of the
    others) in ONE launch"""
    n, ids, ring = OC.CHAIN_CASES[name]
    fx.check(name, exe.chain(fx.inp, n, np.asarray(ids, np.int32), ring, OC.LIVE))

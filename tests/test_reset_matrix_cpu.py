"""The reset conformance matrix (tests/reset_cases.py) with the emulator as the executor -- no GPU.

The same case table, float64 references, oracle comparison and bars as tests/test_gpu_reset_matrix.py, run through tests/emu (the
kernel sources compiled for the CPU): reset_fill_rnd_kernel, reset_sample_kernel, fk_env over the list, reset_finish_kernel and
reset_amp_history_kernel with the launcher's own grid rule, and the reset roles of reset_obs_kernel.  Cases, references and bars are
proven here before they judge the device; the near-branch shares of the references alone are asserted here."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R            # noqa: E402
import reset_cases as RC           # noqa: E402
from tests import emu              # noqa: E402

POST_OBS, POST_AMP_ROW = 2, 32


def _host(case, init):
    W = RC.world()
    const = dict(RC.cache_np(), heightfield=W.hf.numpy(), valid_x=W.valid_x.numpy(), valid_y=W.valid_y.numpy(), betas=W.betas.numpy(),
                 real_traj=W.real.numpy())
    return emu.ResetHost(W.models, {k: v.copy() for k, v in init.items()}, const, RC.scalars(case))


def _run(case, init, stages=emu.RESET_ALL, **override):
    host = _host(case, init)
    host.stages(stages, case["ids"], len(case["ids"]), case["rnd"], **override)
    return host


def _task_host(host, case):
    """a TaskHost (the post-physics buffers) over the reset host's state"""
    W = RC.world()
    th = emu.TaskHost(RC.E, W.hf.numpy(), dt=RC.DT)
    th.rb_state, th.dof_state, th.contact_force = host.arr["rb_state"], host.arr["dof_state"], host.arr["contact_force"]
    th.betas, th.traj_verts, th.amp, th.progress = host.const["betas"], host.arr["traj_verts"], host.arr["amp"], host.arr["progress"]
    th.reset, th.terminate = host.arr["reset"], host.arr["terminate"]
    th.obs[:], th.flip_obs[:] = np.nan, np.nan
    return th


@pytest.fixture(scope="module")
def init():
    return RC.initial()


def test_near_branch_shares_of_the_references_stay_under_the_cap():
    RC.near_shares().check()


def test_reset_cases_through_the_emulator(init):
    tab, fails, shares = R.Table("reset", "emulator"), [], RC.Shares()
    for case in RC.cases():
        RC.judge(case, init, _run(case, init).arr, tab, fails, shares)
    assert not fails, fails
    shares.check()
    tab.check()


def test_history_alone_after_a_reset_without_it_equals_the_full_reset(init):
    for case in (RC.cases()[3], RC.cases()[5]):                  # amp_ring 0 and a non-zero head
        full = _run(case, init).arr
        host = _run(case, init, flags=case["flags"] | RC.NO_AMP_HISTORY, stages=emu.RESET_SAMPLE | emu.RESET_FK | emu.RESET_FINISH)
        tab, fails = R.Table("reset", "emulator"), []
        RC.judge(case, init, host.arr, tab, fails, history=False)
        assert not fails, fails
        tab.check()
        host.stages(emu.RESET_HISTORY, case["ids"], len(case["ids"]), case["rnd"])
        for k in RC.OUT_KEYS:
            assert RC.same_bits(host.arr[k], full[k]), (case["name"], k)


def test_random_rows_through_the_emulator(init):
    fails = []
    for case, seed in ((RC.cases()[4], 0x0123456789ABCDEF), (RC.cases()[6], 7), (RC.cases()[0], 1 << 63)):
        ids = case["ids"]
        ws0 = np.random.default_rng(1).normal(size=(len(ids) + 2, RC.RND)).astype(np.float32)
        ws = ws0.copy()
        _host(case, init).fill_rnd(ids, len(ids), seed, ws)
        RC.judge_rnd(ids, len(ids), seed, ws, ws0, fails)
    assert not fails, fails


def test_real_pick_perm_is_a_bijection():
    for n, key in ((1, 5), (4, 0), (5, 77), (16, 3), (17, 0xFFFFFFFF), (261, 0x1234ABCD)):
        assert sorted(R.real_pick_perm(i, n, key) for i in range(n)) == list(range(n))
    from emloco_amd import _lib as L
    assert all(R.real_pick_perm(i, 261, 99) == L.real_pick_perm(i, 261, 99) for i in range(261))


@pytest.mark.parametrize("index, seeded", [(4, False), (4, True), (7, True)])
def test_reset_roles_of_the_fused_launch_equal_the_separate_launches(init, index, seeded):
    """reset_obs_kernel's reset roles (rows supplied, and made from a seed) against reset_fill_rnd + the four reset launches + the
    post-physics pass (OBS | AMP_ROW) of the listed envs: every buffer, bit for bit.  The seeded runs are judged against the references
    too, on the rows the seed makes (unsteered) and, with real paths (case 7), on the permutation key derived from the seed."""
    case, seed = RC.cases()[index], 0xC0FFEE1234
    ids, n = case["ids"], len(case["ids"])
    key = R.seeded_real_key(seed) if seeded else case["real_key"]
    a, b = _host(case, init), _host(case, init)
    ws_a = np.full((n, RC.RND), np.nan, np.float32)
    ws_b = ws_a.copy()
    rnd = case["rnd"]
    if seeded:
        a.fill_rnd(ids, n, seed, ws_a)
        rnd = ws_a
    a.stages(emu.RESET_ALL, ids, n, rnd, real_pick_key=key)
    if seeded:                                                   # the rows of the seed drive a reset that the references accept
        tab, fails = R.Table("reset", "emulator"), []
        RC.judge(dict(case, rnd=ws_a, real_key=key), init, a.arr, tab, fails)
        assert not fails, fails
        tab.check()
    ta, tb = _task_host(a, case), _task_host(b, case)
    ta.post_physics(POST_OBS | POST_AMP_ROW, ids[:case["n"]])
    b.reset_obs(tb, ids, n, seed=seed, rnd_ws=ws_b if seeded else None, rnd=None if seeded else case["rnd"])
    for k in RC.OUT_KEYS:
        assert RC.same_bits(a.arr[k], b.arr[k]), k
    assert RC.same_bits(ta.obs, tb.obs) and RC.same_bits(ta.flip_obs, tb.flip_obs) and RC.same_bits(ws_a, ws_b)
    assert np.isfinite(ta.obs[ids[:case["n"]]]).all() and np.isnan(ta.obs).any()


def test_reset_references_against_closed_forms():
    """the new kernel_refs functions against properties that do not depend on their own formulas"""
    g = R._gen(3)
    unit = lambda q: q / q.norm(dim=-1, keepdim=True)
    q0, q1 = unit(torch.randn(200, 4, generator=g, dtype=torch.float64)), unit(torch.randn(200, 4, generator=g, dtype=torch.float64))
    t = torch.rand(200, generator=g, dtype=torch.float64)
    q = R.slerp(q0, q1, t)
    # a slerp is a unit quaternion on the short arc: the angle from q0 is t x the angle between the two rotations, endpoints included
    ang = lambda a, b: torch.acos((a * b).sum(-1).abs().clamp(max=1.0))
    assert torch.allclose(q.norm(dim=-1), torch.ones(200, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(ang(q0, q), t * ang(q0, q1), atol=1e-9) and torch.allclose(ang(q, q1), (1 - t) * ang(q0, q1), atol=1e-9)
    assert torch.allclose(R.slerp(q0, q1, torch.zeros(200)), q0, atol=1e-12)
    assert torch.equal(R.slerp(q0, -q0, t), q0) and torch.equal(R.slerp(q0, q0.clone(), t), q0)
    # rotation vector <-> quaternion round trip below pi; w < 0 wraps to the same rotation; identity and w = 1 give zero
    e = torch.randn(300, 3, generator=g, dtype=torch.float64)
    e = e / e.norm(dim=-1, keepdim=True) * (torch.rand(300, 1, generator=g, dtype=torch.float64) * 3.1 + 1e-3)
    assert torch.allclose(R.quat_to_exp_map(R.rotvec_to_quat(e)), e, atol=1e-9)
    assert torch.allclose(R.quat_to_exp_map(-R.rotvec_to_quat(e)), e, atol=1e-9)
    assert torch.equal(R.quat_to_exp_map(torch.tensor([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, -1.0]])), torch.zeros(2, 3, dtype=torch.float64))
    # frame blend: clamped phase, unclamped weight, the last frame, negative time
    i0, i1, w = R.frame_blend(torch.tensor([0.0, 0.3125, 1.25, 1.625, -0.2]), torch.full((5,), 1.25), torch.full((5,), 0.125), torch.full((5,), 11))
    assert i0.tolist() == [0, 2, 10, 10, 0] and i1.tolist() == [1, 3, 10, 10, 1]
    assert torch.allclose(w, torch.tensor([0.0, 0.5, 0.0, 3.0, 0.0], dtype=torch.float64), atol=1e-12)
    # quat_apply of a unit quaternion is the rotation
    v = torch.randn(200, 3, generator=g, dtype=torch.float64)
    assert torch.allclose(R.quat_apply(q0, v), R.quat_rotate(q0, v), atol=1e-12)
    # the lowest point of a sphere, of a capsule standing on end and of a tilted box, by hand
    rot = torch.tensor([[[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [math.sin(math.pi / 8), 0.0, 0.0, math.cos(math.pi / 8)]]], dtype=torch.float64)
    pos = torch.tensor([[[0.0, 0.0, 5.0], [0.0, 0.0, 5.0], [0.0, 0.0, 5.0]]])
    ga = torch.tensor([[[0.0, 0.0, 0.5], [0.0, 0.0, 0.3], [0.0, 0.0, 0.0]]])
    gb = torch.tensor([[[0.0, 0.0, 0.0], [0.0, 0.0, -0.4], [1.0, 1.0, 1.0]]])
    gr = torch.tensor([[0.25, 0.1, 0.0]])
    low = lambda types, keep: R.lowest_collision_point(pos[:, keep], rot[:, keep], [types[k] for k in keep], ga[:, keep], gb[:, keep], gr[:, keep]).item()
    types = (R.GEOM_SPHERE, R.GEOM_CAPSULE, R.GEOM_BOX)
    assert abs(low(types, [0]) - 5.25) < 1e-6 and abs(low(types, [1]) - 4.5) < 1e-6 and abs(low(types, [2]) - (5.0 - math.sqrt(2.0))) < 1e-6
    # the device generator's rows: 24-bit uniforms, different per row, entry and seed
    a, b = R.reset_rnd_row(5, 0), R.reset_rnd_row(5, 1)
    assert (a >= 0).all() and (a < 1).all() and (a * 2 ** 24 == torch.round(a * 2 ** 24)).all() and abs(a.mean().item() - 0.5) < 0.05
    assert not torch.equal(a, b) and not torch.equal(a, R.reset_rnd_row(5 + (1 << 32), 0)) and a.unique().numel() > 500

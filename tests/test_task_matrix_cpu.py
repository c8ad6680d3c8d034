"""The task-kernel conformance matrix (tests/task_cases.py) with the emulator as the executor -- no GPU.

The same case tables, float64 references, oracle comparisons and bars as tests/test_gpu_task_matrix.py, run through tests/emu (the
kernel sources compiled for the CPU): cases, references and bars are proven here before they judge the device.  Every case that
costs the emulator under about a second runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R            # noqa: E402
import task_cases as TC            # noqa: E402
from tests import emu              # noqa: E402


def P(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _np(t, dt=np.float32):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=dt)


class EmuExecutor:
    def pd_targets(self, actions, offset, scale, zero_mask):
        return emu.task_pd_targets(_np(actions), _np(offset), _np(scale), _np(zero_mask, np.uint8))

    def amp_rows(self, a, subset):
        n = a["root_pos"].shape[0]
        out = np.full((n, 206), np.nan, np.float32)
        arrs = [_np(a[k]) for k in ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "key_pos", "betas")]
        sub = _np(subset, np.int32)
        fn = emu.lib().emu_task_amp_rows
        fn.argtypes = [C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p]
        assert fn(n, *[P(x) for x in arrs], P(sub), len(sub), P(out)) == 0
        return out

    def post_physics(self, c, hf, mode, amp0):
        E = c["rb_state"].shape[0]
        th = emu.TaskHost(E, _np(hf, np.int16), dt=c["dt"], episode_len=int(c["max_episode_length"]))
        assert np.float32(th.traj_dur) == np.float32(c["traj_dur"])
        for name in ("rb_state", "dof_state", "dof_force", "contact_force", "betas", "traj_verts"):
            getattr(th, name)[:] = _np(c[name])
        th.progress[:] = c["progress"].numpy()
        th.reset[:] = 7
        th.terminate[:] = 7
        th.amp[:] = amp0
        for name in ("obs", "flip_obs", "rew", "reward_raw"):
            getattr(th, name)[:] = np.nan
        th.post_physics(mode)
        return dict(obs=th.obs, flip_obs=th.flip_obs, rew=th.rew, reward_raw=th.reward_raw, amp=th.amp, progress=th.progress,
                    reset=th.reset, terminate=th.terminate)

    def heights(self, hf, pose7, grid):
        hf, pose7 = _np(hf, np.int16), _np(pose7)
        n, npt = pose7.shape[0], 1024 if grid else 9
        h, px, py = np.full((n, npt), np.nan, np.float32), np.full((n, npt), -9, np.int64), np.full((n, npt), -9, np.int64)
        fn = emu.lib().emu_task_get_heights
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        fn(P(hf), hf.shape[0], hf.shape[1], 0.1, 0.005, P(pose7), n, grid, P(h), P(px), P(py))
        return h, px, py

    def compact(self, flags):
        f = _np(flags, np.int64)
        ids = np.full(f.size + 1, 12345, np.int32)
        emu.lib().emu_compact_flags(P(f), f.size, P(ids))
        return ids


EXE = EmuExecutor()


@pytest.mark.parametrize("n", TC.PD_SIZES)
def test_pd_targets_cases_through_the_emulator(n):
    c = TC.case_pd(n, n)
    TC.judge_pd(c, EXE.pd_targets(c["actions"], c["offset"], c["scale"], c["zero_mask"]))


def test_amp_rows_cases_through_the_emulator():
    tab, fails = R.Table("task", "emulator"), []
    for n, seed in TC.AMP_CASES:
        c = R.case_task(n, seed)
        TC.judge_amp_row((n, seed), c, R.DOF_SUBSET, EXE.amp_rows(TC.amp_inputs(c), R.DOF_SUBSET), tab, fails)
    c = R.case_task(65, 13)
    got = EXE.amp_rows(TC.amp_inputs(c), R.DOF_SUBSET[:3])           # a 3-entry subset: 44 values per row, the rest of the row untouched
    TC.judge_amp_row((65, 13, "n_sub=3"), c, R.DOF_SUBSET[:3], got, tab, fails)
    assert np.isnan(got[:, 44:]).all()
    assert not fails, fails
    tab.check()


def test_post_physics_cases_through_the_emulator():
    tab, fails = R.Table("task", "emulator"), []
    hf = R.task_map()
    for E, seed in TC.POST_CASES:
        c = R.case_task(E, seed)
        amp0 = np.random.default_rng(seed).normal(size=(E, 15, 206)).astype(np.float32)
        for mode in (TC.POST_STEP, TC.POST_STEP & ~TC.POST_ADVANCE):
            TC.judge_post((E, seed, mode), c, hf, mode, amp0, EXE.post_physics(c, hf, mode, amp0), tab, fails)
        rb = c["rb_state"].numpy()
        for grid, pose in ((1, rb[:, R.HEAD_BODY, :7]), (0, rb[:, 0, :7])):
            px, py = TC.judge_heights((E, seed), hf.numpy(), pose, grid, EXE.heights(hf, pose, grid), fails)
            if E >= 63:                                      # the probes leave the non-square map on each of its four sides
                assert (px == 0).any() and (py == 0).any() and (px == hf.shape[0] - 2).any() and (py == hf.shape[1] - 2).any()
                assert ((px > 0) & (px < hf.shape[0] - 2) & (py > 0) & (py < hf.shape[1] - 2)).any()
    assert not fails, fails
    tab.check()


@pytest.mark.parametrize("n", [n for n in TC.COMPACT_SIZES if n <= 4096])
def test_compaction_cases_through_the_emulator(n):
    for pattern in TC.COMPACT_PATTERNS:
        flags = TC.compact_flags_case(n, pattern)
        TC.judge_compact(flags, EXE.compact(flags))

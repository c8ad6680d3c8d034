"""The pooled reset / observation launch (tests/chain_cases.py) with the emulator as the executor -- no GPU.

The same table, model of the pool rules and float64 judges as tests/test_gpu_chain.py, run through tests/emu: reset_obs_kernel with every
role (reset chain, pool draw, live observations, AMP history) behind emloco::chain_pool_error / emloco::chain_pack, the launcher's own
argument check and arithmetic (emloco_amd/csrc/chain_kernels.hip), which emloco_task_reset_obs_pooled calls on the device."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as CC           # noqa: E402
import kernel_refs as R            # noqa: E402
import reset_cases as RC           # noqa: E402
from tests import emu              # noqa: E402
from test_reset_matrix_cpu import _task_host      # noqa: E402


class EmuExec:
    """chain_cases' executor over host memory"""

    def __init__(self, su, k, zero_pool):
        W = RC.world()
        self.su, self.k = su, k
        self.case = dict(flags=su["flags"], amp_ring=su["amp_ring"], real_key=0, scalars=su["scalars"])
        cache, real = RC.const_of(su)
        const = dict({key: np.ascontiguousarray(v.numpy()) for key, v in cache.items()}, heightfield=W.hf.numpy(), valid_x=W.valid_x.numpy(),
                     valid_y=W.valid_y.numpy(), betas=W.betas.numpy(), real_traj=np.ascontiguousarray(real.numpy()))
        self.host = emu.ResetHost(W.models, {key: v.copy() for key, v in RC.initial().items()}, const, RC.scalars(self.case))
        self.th = _task_host(self.host, self.case)
        self.ws = np.full((CC.E, CC.RND), CC.WS_SENT, np.float32)
        self.pool = np.full((2, k, CC.POOL_FLOATS), 0.0 if zero_pool else CC.POOL_SENT, np.float32)
        self.tag = np.full((2, k), 0 if zero_pool else CC.TAG_SENT, np.uint64)

    def launch(self, ids, cap, seed, pool, live_mode=0, skip=None, rnd=None, real_pick=None):
        pl = None
        if pool is not None:
            at = lambda a, i: None if i is None else a[i]
            pl = (pool["k"], at(self.pool, pool["cur"]), at(self.tag, pool["cur_tag"]), at(self.pool, pool["next"]), at(self.tag, pool["next_tag"]),
                  pool["next_seed"])
        over = {}
        if real_pick is not None:
            self._pick = np.ascontiguousarray(real_pick, np.int32)
            over["real_pick"] = self._pick.ctypes.data
        return self.host.reset_obs(self.th, ids, cap, seed=seed, rnd_ws=self.ws, rnd=rnd, pool=pl, live_mode=live_mode, skip=skip, may_refuse=True,
                                   **over)

    def post_physics(self, mode, env_ids):
        self.th.post_physics(mode, env_ids)

    def refill(self):
        self.ws[:] = CC.WS_SENT
        self.th.obs[:], self.th.flip_obs[:] = np.nan, np.nan

    def snapshot(self):
        out = {key: self.host.arr[key].copy() for key in RC.OUT_KEYS}
        out.update(obs=self.th.obs.copy(), flip_obs=self.th.flip_obs.copy(), ws=self.ws.copy(), pool=self.pool.copy(), tag=self.tag.copy())
        return out


@pytest.mark.parametrize("cid, seq, su", CC.matrix(), ids=[m[0] for m in CC.matrix()])
def test_pooled_call_equals_the_direct_call(cid, seq, su):
    res = CC.run_sequence(EmuExec, seq, su)
    if seq in CC.FLAG_SEQUENCES or seq == "stride":
        tab, fails = R.Table("chain", "emulator"), []
        CC.judge_direct(cid, su, res, tab, fails)
        assert not fails, fails
        tab.check()


@pytest.mark.parametrize("name", list(CC.direct_cases()))
def test_direct_edge_rows_against_float64(name):
    tab, fails = R.Table("chain", "emulator"), []
    case, before, out = CC.run_direct(EmuExec, name, tab, fails)
    assert not fails, fails
    tab.check()
    CC.check_direct_edges(name, case, out)


def test_live_role_beside_a_pool():
    """... with the diagnostic stamps on (emloco_task_chain_profile's buffer, which the product never passes): every role stamps its own
    slots of the 16 and nothing else, and the results are those of a launch without them (run_live's comparisons)"""
    prof = np.full(16, -1, np.int64)
    guard = np.full(16, -1, np.int64)
    both = np.concatenate([prof, guard])                        # the 16 stamps and a band behind them
    emu.chain_prof(both[:16])
    try:
        CC.run_live(EmuExec)
    finally:
        emu.chain_prof(None)
    assert (both[:16] == 0).all() and (both[16:] == -1).all(), both     # the emulator's clock reads 0


def test_traj_reset_kernel_stops_at_the_padding_of_its_list(golden):
    """traj_reset_kernel on a compacted list (valid ids first, -1 behind them): the listed envs as without the padding, no other row"""
    import ctypes as C
    from helpers import TRAJ_CASES, traj_reset_bufs, traj_rnd_rows
    name = "traj_reset_plain"
    g = golden(name)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rnd = traj_rnd_rows(g)
    ip, rv = np.ascontiguousarray(g["init_pos"], np.float32), np.ascontiguousarray(g["root_vel"], np.float32)
    got = []
    for ids in (np.array([5, 2, 9, -1, -1, -1], np.int32), np.array([5, 2, 9], np.int32)):
        verts = np.full((16, 101, 3), np.nan, np.float32)
        inverted = np.full(16, 7, np.uint8)
        b = traj_reset_bufs(TRAJ_CASES[name], g, verts.ctypes.data, inverted.ctypes.data, None, None)
        emu.lib().emu_task_traj_reset(C.byref(b), P(ids), len(ids), P(rnd), P(ip), P(rv))
        got.append(verts)
    assert RC.same_bits(got[0], got[1]) and np.isfinite(got[0][[5, 2, 9]]).all() and np.isnan(np.delete(got[0], [5, 2, 9], axis=0)).all()


def test_pd_targets_tail_and_action_copy():
    """pd_targets_kernel at a size that is no multiple of its 256-thread workgroups (3 envs: 207 elements), with the copy of the actions
    emloco_task_pd_targets_copy asks for: targets against float64, the copy bit for bit, nothing behind either"""
    g = R._gen(5)
    n = 3
    act, off, sc = torch.randn(n, 69, generator=g), torch.randn(69, generator=g), torch.rand(69, generator=g) + 0.5
    mask = (torch.rand(69, generator=g) < 0.2).to(torch.uint8)
    copy = np.full((n + 1, 69), np.nan, np.float32)
    out = emu.task_pd_targets(act.numpy(), off.numpy(), sc.numpy(), mask.numpy(), copy=copy)
    ref = R.pd_targets(act, off, sc, mask)
    f32 = R.pd_targets(act, off, sc, mask, dtype=torch.float32)
    assert R.err_max(out, ref) <= R.MARGIN * max(R.err_max(f32, ref), 2.0 ** -24)
    assert RC.same_bits(copy[:n], act.numpy()) and np.isnan(copy[n]).all()


def test_get_heights_kernel_with_either_output_left_out():
    """emloco_task_get_heights' outputs are each optional: heights alone and indices alone equal the full call's"""
    import ctypes as C
    W = RC.world()
    hf = np.ascontiguousarray(W.hf.numpy())
    g = R._gen(6)
    n = 5
    pose = torch.randn(n, 7, generator=g)
    pose[:, 0], pose[:, 1] = pose[:, 0].abs() + 2.0, pose[:, 1].abs() + 2.0
    pose = np.ascontiguousarray(pose.numpy())
    fn = emu.lib().emu_task_get_heights
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    new = lambda: (np.full((n, 9), np.nan, np.float32), np.full((n, 9), -1, np.int64), np.full((n, 9), -1, np.int64))
    h, px, py = new()
    fn(hf.ctypes.data, 83, 61, RC.HSCALE, RC.VSCALE, pose.ctypes.data, n, 0, h.ctypes.data, px.ctypes.data, py.ctypes.data)
    h1, px1, py1 = new()
    fn(hf.ctypes.data, 83, 61, RC.HSCALE, RC.VSCALE, pose.ctypes.data, n, 0, h1.ctypes.data, None, None)
    h2, px2, py2 = new()
    fn(hf.ctypes.data, 83, 61, RC.HSCALE, RC.VSCALE, pose.ctypes.data, n, 0, None, px2.ctypes.data, py2.ctypes.data)
    assert np.isfinite(h).all() and (px >= 0).all() and RC.same_bits(h1, h) and (px1 == -1).all() and (py1 == -1).all()
    assert np.isnan(h2).all() and np.array_equal(px2, px) and np.array_equal(py2, py)


def test_refused_pool_arguments_write_nothing():
    CC.run_refusals(EmuExec)


def test_pool_model_counts():
    """the model itself, by hand: draw counts and which entries hit"""
    assert [CC.draw_count(64, n) for n in (0, 1, 10, 40)] == [32, 33, 44, 64] and CC.draw_count(8, 12) == 8 and CC.draw_count(256, 258) == 256
    for name, hits in CC.EXPECT_HITS.items():
        k, calls = CC.plan(name)
        m = CC.pool_model(k, calls, 0 if name == "seed zero" else CC.TAG_SENT)
        assert int(m[-1][0].sum()) == hits, name
    k, calls = CC.plan("draw count")
    hits, tags = CC.pool_model(k, calls, CC.TAG_SENT)[-1]
    assert hits[:33].all() and not hits[33:].any()
    k, calls = CC.plan("stale tags")
    hits, _ = CC.pool_model(k, calls, CC.TAG_SENT)[-1]
    assert hits[:42].all() and not hits[42:].any()
    assert (CC.pool_model(k, calls, CC.TAG_SENT)[2][1][1][42:] == CC.SEEDS[1]).all()            # B[42..63] still carry the seed of the second call

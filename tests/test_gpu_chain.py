"""Device run of the pooled reset / observation launch: emloco_task_reset_obs_pooled (include/emloco_task.h) through the C ABI on NativeSims
of 300 varied models, against the table, the model of the pool rules and the float64 judges of tests/chain_cases.py.

tests/test_chain_cpu.py runs the same table through the emulator; the device run differs in the executor only.  The buffers are those of
tests/test_gpu_reset_matrix.py's Scene (guarded outputs, padded inputs, the simulator's tensors started from garbage), with a guarded pair
of pool buffers and tag arrays beside them.  A sequence runs on two executors side by side (the pooled call and the same call with
pool = NULL from the same state), so two simulators are held.

Bars: bit for bit between the pooled and the direct call in every buffer; the direct call of every flag set against float64 with the
bars of the reset matrix (MARGIN x the float32 reference's own error; the figures are printed, `pytest -s`); tags, draw counts, pool
floats behind the draw count and the rows of the random workspace against the model, exactly.  Refused pool arguments (k out of range, a
buffer without its tags, cur == next, cur_tag == next_tag) return non-zero and write nothing."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as CC                                                          # noqa: E402
import kernel_refs as R                                                           # noqa: E402
import reset_cases as RC                                                          # noqa: E402
from test_gpu_kernel_matrix import DEV, _ptr, _stream                            # noqa: E402
from test_gpu_task_matrix import _GuardedInt, _dev, _fout, _padded              # noqa: E402
from test_gpu_reset_matrix import Scene, _lib, _release_device_tensors, sim      # noqa: E402,F401

E = RC.E
_I64 = lambda x: x - (1 << 64) if x >= (1 << 63) else x


@pytest.fixture(scope="module")
def sim2():
    from emloco_amd.sim import NativeSim
    s = NativeSim(RC.world().models)
    yield s
    torch.cuda.synchronize()
    s.close()


@pytest.fixture
def make(sim, sim2):
    """executors on the two simulators in turn"""
    turn = itertools.cycle((sim, sim2))
    return lambda su, k, zero_pool: DevExec(next(turn), su, k, zero_pool)


class DevExec(Scene):
    """chain_cases' executor over the C ABI"""

    def __init__(self, sim, su, k, zero_pool):
        case = dict(ids=np.full(E + 1, -1, np.int32), rnd=np.zeros((E + 1, RC.RND), np.float32), flags=su["flags"], amp_ring=su["amp_ring"], real_key=0,
                    scalars=su["scalars"])
        super().__init__(sim, case, RC.initial())
        for key, v in su["const"].items():
            self.inp[key] = _padded(v)
        self.k = k
        self.pool = _fout(2 * k, CC.POOL_FLOATS)
        self.pool.fill(torch.full((1, 2 * k, CC.POOL_FLOATS), 0.0 if zero_pool else CC.POOL_SENT, device=DEV))
        self.tag = _GuardedInt(2 * k, fill=torch.full((2 * k,), 0 if zero_pool else _I64(CC.TAG_SENT), dtype=torch.int64))
        self.refill_ws()

    def refill_ws(self):
        self.ws.fill(torch.full((1, E + 1, RC.RND), CC.WS_SENT, device=DEV))

    def refill(self):
        self.refill_ws()
        for o in self.obs.values():
            o.fill()

    def _pool(self, p):
        fp = lambda i: None if i is None else self.pool.ptr().value + i * self.k * CC.POOL_FLOATS * 4
        tp = lambda i: None if i is None else self.tag.ptr().value + i * self.k * 8
        return self.L.ResetPool(p["k"], fp(p["cur"]), tp(p["cur_tag"]), fp(p["next"]), tp(p["next_tag"]), p["next_seed"])

    def launch(self, ids, cap, seed, pool, live_mode=0, skip=None, rnd=None, real_pick=None):
        assert len(ids) == cap + 1 <= E + 1
        self.ids[:cap + 1].copy_(torch.from_numpy(ids))
        if rnd is not None:
            self.rnd[:len(rnd)].copy_(torch.from_numpy(rnd))
        over = {} if real_pick is None else dict(real_pick=_dev(torch.from_numpy(np.ascontiguousarray(real_pick, np.int32))).data_ptr())
        b, pb = self.bufs(**over), self.task_bufs(self.case["amp_ring"])
        pl = None if pool is None else self._pool(pool)
        sk = None if skip is None else _ptr(_dev(torch.from_numpy(skip)))
        rc = _lib().emloco_task_reset_obs_pooled(self.h(), C.byref(b), C.byref(pb), live_mode, sk, _ptr(self.ids), cap, C.c_uint64(seed), self.ws.ptr(),
                                                 None if rnd is None else _ptr(self.rnd), None if pl is None else C.byref(pl), _stream())
        torch.cuda.synchronize()
        return rc

    def post_physics(self, mode, env_ids):
        pb = self.task_bufs(self.case["amp_ring"])
        ids = _dev(torch.from_numpy(np.ascontiguousarray(env_ids, np.int32)))
        assert _lib().emloco_task_post_physics(C.byref(pb), mode, _ptr(ids), len(env_ids), _stream()) == 0
        torch.cuda.synchronize()

    def snapshot(self):
        out = self.out()
        x = self.extras()
        out.update(obs=x["obs"], flip_obs=x["flip_obs"], ws=x["ws"][:E],
                   pool=self.pool.got()[1][0].cpu().numpy().reshape(2, self.k, CC.POOL_FLOATS),
                   tag=self.tag.got().cpu().numpy().view(np.uint64).reshape(2, self.k))
        return out


@pytest.mark.parametrize("cid, seq, su", CC.matrix(), ids=[m[0] for m in CC.matrix()])
def test_pooled_call_equals_the_direct_call(make, cid, seq, su):
    res = CC.run_sequence(make, seq, su)
    if seq in CC.FLAG_SEQUENCES or seq == "stride":
        tab, fails = R.Table("chain"), []
        CC.judge_direct(cid, su, res, tab, fails)
        assert not fails, fails
        tab.check()


@pytest.mark.parametrize("name", list(CC.direct_cases()))
def test_direct_edge_rows_against_float64(make, name):
    tab, fails = R.Table("chain"), []
    case, before, out = CC.run_direct(make, name, tab, fails)
    assert not fails, fails
    tab.check()
    CC.check_direct_edges(name, case, out)


def test_live_role_beside_a_pool(make):
    CC.run_live(make)


def test_refused_pool_arguments_write_nothing(make):
    CC.run_refusals(make)

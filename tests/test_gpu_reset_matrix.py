"""Device conformance matrix of the reset path (emloco_amd/csrc/reset_kernels.hip and the reset roles of reset_obs_kernel) against
float64 and the fp32 oracle.

Companion of tests/test_gpu_task_matrix.py: every case calls the public C ABI (emloco_task_reset, emloco_task_reset_seeded,
emloco_task_reset_amp_history, emloco_task_reset_obs) on a NativeSim of 300 varied models.  Every buffer of EmlocoResetBufs that a reset
writes is a guarded buffer (a sentinel band before and behind it that must survive; NaN / an integer sentinel / random AMP rows in the
logical output before the launch), every input carries garbage outside its logical extent, and the simulator's own tensors start from
garbage.  The case table, the float64 references and the judges are those of tests/reset_cases.py, which tests/test_reset_matrix_cpu.py
runs through the emulator on a CPU: the device run differs in the executor only.

Covered: the motion sample (frame blend, slerp, rotation vectors) on a synthetic motion cache with random, single-frame, exactly
representable and near-identity clips; random heading and forward speed; fixed and sampled placement on a non-square sloped map;
the centre-height mean; kinematics; the height fix; buffer zeroing; LocoVal pose capture; the 14 AMP history rows (amp_ring 0 and a
non-zero head); the device random rows; the real-path permutation; lists of 1, 2, 65 and 257 entries, scattered and -1 padded; the
history alone against the full reset; one call against chunks; the fused launch against the separate calls (rows supplied and seeded);
refused calls.

Bars.  Copies, ids, flags, zeros, envs that are not listed, random rows, chunk-vs-whole, fused-vs-separate, history-alone-vs-full: bit
for bit.  ground_h: equal to the fp32 oracle's centre probes of the written pose, averaged in torch's order.  motion_times: one rounding
of u len.  Every other float: MARGIN (8) x the largest float32-vs-float64 error of the same kernel_refs function over the cases,
measured as max error over the tensor's max ("height fix": metres).

Measured on an MI355X (every run prints the figures, `pytest -s`; tests/test_reset_matrix_cpu.py prints the float32 column and the
emulator's figures on any machine):

    output                              float32 reference     bar (8 x)     emulator      device
    dof_pos                             7.549e-06             6.039e-05     7.549e-06     7.549e-06
    dof_pos 180                         2.151e-07             1.721e-06     2.151e-07     2.151e-07
    dof_pos near-identity               3.163e-06             2.531e-05     3.163e-06     3.163e-06
    dof_vel                             8.830e-06             7.064e-05     8.830e-06     8.830e-06
    root rot                            5.817e-06             4.653e-05     5.846e-06     5.846e-06
    root vel                            1.540e-05             1.232e-04     1.540e-05     1.540e-05
    root ang_vel                        4.579e-06             3.663e-05     4.579e-06     4.579e-06
    fk position                         1.836e-06             1.469e-05     1.836e-06     1.836e-06
    fk rotation                         3.088e-07             2.470e-06     2.976e-07     2.976e-07
    height fix [m]                      1.051e-07             8.411e-07     2.489e-07     2.489e-07
    history rotation                    5.984e-05             4.787e-04     5.984e-05     5.984e-05
    history velocity                    1.609e-05             1.287e-04     1.609e-05     1.609e-05
    history dof_pos                     1.422e-05             1.138e-04     1.427e-05     1.427e-05
    history dof_vel                     7.149e-06             5.719e-05     7.149e-06     7.149e-06
    history key_pos                     3.229e-05             2.583e-04     3.229e-05     3.229e-05

(The float32 column is stock float32 torch on the host that runs the test: its last digits move with the host's math library, e.g. root
rot 5.817e-06 / 5.846e-06 and history dof_pos 1.422e-05 / 1.433e-05 on two hosts.  The emulator and the device agree to every digit
shown.  dof_pos, dof_vel and the history blocks: the 1e-5 class is the float32 rounding of the blend weight (time - i0 dt) / dt at times
of 1 - 2.5 s over a frame time of 1 / 30 s, which the float32 reference shows as well.  Near-branch elements left out: 0 in every
family; joints at 180 degrees are judged -- up to the +-pi sign in dof_pos, as they are in the history rows, whose tangent | normal form
does not see the wrap.)

emloco_task_reset_seeded refuses everything emloco_task_reset refuses before anything is launched (it used to fill the random rows
first, so a NULL buffer struct, a missing buffer or a NULL simulator got rows written and then the error code, and an n above the
simulator's env count reached the fill): test_refused_calls_write_nothing holds every reset entry point to that.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R                                                          # noqa: E402
import reset_cases as RC                                                         # noqa: E402
from test_gpu_kernel_matrix import DEV, TAIL, _bits, _ptr, _stream               # noqa: E402
from test_gpu_task_matrix import _GuardedInt, _dev, _fout, _padded, _KEEP       # noqa: E402

POST_OBS, POST_AMP_ROW = 2, 32
OBS = 1422
SIM_KEYS = {"root_state": "root_state", "dof_state": "dof_state", "rb_state": "rigid_body_state", "contact_force": "contact_force",
            "warm_start": "warm_start"}
FLOAT_OUT = ("traj_verts", "waypoint_traj", "init_pose", "init_vel", "amp", "motion_times", "ground_h")
INT_OUT = ("progress", "reset", "terminate", "motion_ids")
FIELD = {"progress": "progress_buf", "reset": "reset_buf", "terminate": "terminate_buf", "amp": "amp_obs_buf"}


def _lib():
    from emloco_amd import _lib as L
    return L.require_device()


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


@pytest.fixture(scope="module")
def sim():
    from emloco_amd.sim import NativeSim
    s = NativeSim(RC.world().models)
    yield s
    torch.cuda.synchronize()
    s.close()


@pytest.fixture(scope="module")
def init():
    return RC.initial()


class Scene:
    """the simulator's tensors set to the initial garbage, the buffers of one EmlocoResetBufs by hand: guarded outputs, padded inputs"""

    def __init__(self, sim, case, init):
        from emloco_amd import _lib as L
        W = RC.world()
        self.sim, self.case, self.init, self.L = sim, case, init, L
        for k, attr in SIM_KEYS.items():
            getattr(sim, attr).view(-1).copy_(torch.from_numpy(init[k]).view(-1))
        c = W.cache
        self.inp = {k: _padded(c[k]) for k in c}
        self.inp.update(heightfield=_padded(W.hf), valid_x=_padded(W.valid_x), valid_y=_padded(W.valid_y), betas=_padded(W.betas),
                        real_traj=_padded(W.real))
        self.keys = _dev(torch.tensor(R.KEY_BODIES, dtype=torch.int32))
        self.sub = _dev(torch.tensor(R.DOF_SUBSET, dtype=torch.int32))
        self.l2r = _dev(torch.tensor(R.LEFT_TO_RIGHT, dtype=torch.int32))
        self.ids = _padded(torch.from_numpy(case["ids"]))
        self.rnd = _padded(torch.from_numpy(case["rnd"]))
        self.f = {}
        for k in FLOAT_OUT:
            v = init[k].reshape(RC.E, -1)
            self.f[k] = _fout(RC.E, v.shape[1])
            self.f[k].fill(torch.from_numpy(v).to(DEV)[None])
        self.i = {k: _GuardedInt(RC.E, fill=torch.from_numpy(init[k])) for k in INT_OUT}
        self.inv = torch.full((TAIL + RC.E + TAIL,), 9, dtype=torch.uint8, device=DEV)
        self.inv[TAIL:TAIL + RC.E] = torch.from_numpy(init["inverted"]).to(DEV)
        self.inv0 = self.inv.clone()
        self.obs = {k: _fout(RC.E, OBS) for k in ("obs", "flip_obs")}
        nl = len(case["ids"])
        self.ws0 = np.random.default_rng(2).normal(size=(nl, RC.RND)).astype(np.float32)
        self.ws = _fout(nl, RC.RND)
        self.ws.fill(torch.from_numpy(self.ws0).to(DEV)[None])

    def bufs(self, **override):
        b = self.L.ResetBufs()
        for k, v in {**RC.scalars(self.case), **override}.items():
            setattr(b, k, v)
        for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs", "motion_len", "motion_dt", "motion_nframes", "motion_start", "heightfield", "valid_x",
                  "valid_y", "betas"):
            setattr(b, k, self.inp[k].data_ptr())
        b.real_traj = self.inp["real_traj"].data_ptr() if b.n_real > 0 else None
        b.key_bodies, b.dof_subset = self.keys.data_ptr(), self.sub.data_ptr()
        for k in FLOAT_OUT:
            setattr(b, FIELD.get(k, k), self.f[k].ptr().value)
        for k in INT_OUT:
            setattr(b, FIELD.get(k, k), self.i[k].ptr().value)
        b.inverted = self.inv.data_ptr() + TAIL
        return b

    def task_bufs(self, amp_ring=0):
        s, p = self.sim, lambda t: t.data_ptr()
        vert_dt = 168 * RC.DT / 100.0
        return self.L.TaskBufs(RC.E, 83, 61, R.HEAD_BODY, 57, RC.DT, 101 * vert_dt, 0.4, RC.HSCALE, RC.VSCALE, 0.0005, 4.0, 168.0,
                               p(s.rigid_body_state), p(s.dof_state), p(s.dof_force), p(s.contact_force), p(self.inp["betas"]),
                               self.f["traj_verts"].ptr().value, p(self.inp["heightfield"]), p(self.l2r), None, p(self.keys), p(self.sub),
                               self.i["progress"].ptr().value, self.i["reset"].ptr().value, self.i["terminate"].ptr().value,
                               self.obs["obs"].ptr().value, self.obs["flip_obs"].ptr().value, None, None, self.f["amp"].ptr().value, amp_ring)

    def h(self):
        return self.sim._h

    def n(self):
        return len(self.case["ids"])

    def reset(self, lo=0, hi=None, **override):
        hi = self.n() if hi is None else hi
        b = self.bufs(**override)
        rc = _lib().emloco_task_reset(self.h(), C.byref(b), _ptr(self.ids, lo), hi - lo, _ptr(self.rnd, lo * RC.RND), _stream())
        torch.cuda.synchronize()
        return rc

    def history(self):
        b = self.bufs()
        rc = _lib().emloco_task_reset_amp_history(C.byref(b), _ptr(self.ids), self.n(), _stream())
        torch.cuda.synchronize()
        return rc

    def seeded(self, seed):
        b = self.bufs()
        rc = _lib().emloco_task_reset_seeded(self.h(), C.byref(b), _ptr(self.ids), self.n(), C.c_uint64(seed), self.ws.ptr(), _stream())
        torch.cuda.synchronize()
        return rc

    def post(self, mode):
        pb = self.task_bufs(self.case["amp_ring"])
        rc = _lib().emloco_task_post_physics(C.byref(pb), mode, _ptr(self.ids), self.n(), _stream())
        torch.cuda.synchronize()
        return rc

    def reset_obs(self, seed=None):
        b, pb = self.bufs(), self.task_bufs(self.case["amp_ring"])
        rc = _lib().emloco_task_reset_obs(self.h(), C.byref(b), C.byref(pb), 0, None, _ptr(self.ids), self.n(), C.c_uint64(seed or 0),
                                          self.ws.ptr() if seed is not None else None, None if seed is not None else _ptr(self.rnd), _stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        """every buffer a reset may write as CPU numpy arrays shaped like the initial ones, after the guard bands were checked"""
        o = {k: getattr(self.sim, a).cpu().numpy().reshape(self.init[k].shape) for k, a in SIM_KEYS.items()}
        o.update({k: v.got()[1][0].cpu().numpy().reshape(self.init[k].shape) for k, v in self.f.items()})
        o.update({k: v.got().cpu().numpy() for k, v in self.i.items()})
        assert torch.equal(self.inv[:TAIL], self.inv0[:TAIL]) and torch.equal(self.inv[TAIL + RC.E:], self.inv0[TAIL + RC.E:])
        o["inverted"] = self.inv[TAIL:TAIL + RC.E].cpu().numpy()
        return o

    def extras(self):
        return {"obs": self.obs["obs"].got()[1][0].cpu().numpy(), "flip_obs": self.obs["flip_obs"].got()[1][0].cpu().numpy(),
                "ws": self.ws.got()[1][0].cpu().numpy()}

    def untouched(self):
        """nothing was written: the reset buffers, the observations, the random workspace, the simulator's tensors"""
        bufs = list(self.f.values()) + list(self.obs.values()) + [self.ws]
        return (all(torch.equal(_bits(o.buf), _bits(o.before)) for o in bufs) and all(o.untouched() for o in self.i.values())
                and torch.equal(self.inv, self.inv0)
                and all(RC.same_bits(getattr(self.sim, a).cpu().numpy().reshape(self.init[k].shape), self.init[k]) for k, a in SIM_KEYS.items()))

    def inputs_unchanged(self):
        W = RC.world()
        ref = dict(W.cache, heightfield=W.hf, valid_x=W.valid_x, valid_y=W.valid_y, betas=W.betas, real_traj=W.real)
        return all(torch.equal(_bits(v.cpu()), _bits(ref[k])) for k, v in self.inp.items())


def _same(a, b, what):
    for k in a:
        assert RC.same_bits(a[k], b[k]), (what, k)


def test_reset_cases_against_float64_and_the_oracle(sim, init):
    tab, fails, shares = R.Table("reset"), [], RC.Shares()
    for case in RC.cases():
        s = Scene(sim, case, init)
        assert s.reset() == 0
        RC.judge(case, init, s.out(), tab, fails, shares)
        assert s.inputs_unchanged(), "an input was written"
        assert torch.equal(_bits(s.ws.buf), _bits(s.ws.before)), "the random workspace was written by a call with supplied rows"
        _KEEP.clear()
    assert not fails, fails
    shares.check()
    tab.check()


def test_history_alone_after_a_reset_without_it_equals_the_full_reset(sim, init):
    for case in (RC.cases()[3], RC.cases()[5]):                  # amp_ring 0 and a non-zero head
        s = Scene(sim, case, init)
        assert s.reset() == 0
        full = s.out()
        s = Scene(sim, case, init)
        assert s.reset(flags=case["flags"] | RC.NO_AMP_HISTORY) == 0
        tab, fails = R.Table("reset"), []
        RC.judge(case, init, s.out(), tab, fails, history=False)
        assert not fails, fails
        tab.check()
        assert s.history() == 0
        _same(s.out(), full, case["name"])


def test_one_call_above_256_entries_equals_chunks(sim, init):
    case = RC.cases()[6]
    s = Scene(sim, case, init)
    assert s.reset() == 0
    whole = s.out()
    s = Scene(sim, case, init)
    for lo in range(0, case["n"], 100):
        assert s.reset(lo, min(lo + 100, case["n"])) == 0
    _same(s.out(), whole, "chunks of 100")


@pytest.mark.parametrize("index, seed", [(4, 0x0123456789ABCDEF), (6, 7), (7, 0xC0FFEE1234)])
def test_seeded_reset_fills_the_rows_of_the_present_entries_and_resets_from_them(sim, init, index, seed):
    """the rows the seed makes (unsteered) drive a reset that is judged like the table's cases, float figures included; with real paths
    (case 7) the rows of traj_verts follow the permutation key derived from the seed"""
    case = RC.cases()[index]
    s = Scene(sim, case, init)
    assert s.seeded(seed) == 0
    ws, tab, fails = s.extras()["ws"], R.Table("reset"), []
    RC.judge_rnd(case["ids"], len(case["ids"]), seed, ws, s.ws0, fails)
    rows = np.where(np.isfinite(case["rnd"]), ws, np.nan).astype(np.float32)       # (rows behind the valid entries are not read)
    RC.judge(dict(case, rnd=rows, real_key=R.seeded_real_key(seed)), init, s.out(), tab, fails)
    assert not fails, fails
    tab.check()


@pytest.mark.parametrize("index", [0, 6])
@pytest.mark.parametrize("seeded", [False, True])
def test_fused_launch_equals_the_separate_calls(sim, init, index, seeded):
    """emloco_task_reset_obs (rows supplied / seeded) against emloco_task_reset[_seeded] followed by emloco_task_post_physics(OBS | AMP_ROW)
    of the same list: every buffer, the observations and the random workspace, bit for bit, at n = 1 and n = 257"""
    case, seed = RC.cases()[index], 0xC0FFEE1234 if seeded else None
    a = Scene(sim, case, init)
    assert (a.seeded(seed) if seeded else a.reset()) == 0
    assert a.post(POST_OBS | POST_AMP_ROW) == 0
    sep, sep_x = a.out(), a.extras()
    b = Scene(sim, case, init)
    assert b.reset_obs(seed) == 0
    _same(b.out(), sep, "reset_obs")
    _same(b.extras(), sep_x, "reset_obs")
    env = case["ids"][:case["n"]]
    assert np.isfinite(sep_x["obs"][env]).all() and np.isnan(sep_x["obs"]).any()


def test_refused_calls_write_nothing(sim, init):
    """a null or short argument set, or an n out of range: non-zero return, and every guarded buffer, the random workspace and the
    simulator's tensors as they were"""
    lib = _lib()
    case = RC.cases()[2]
    s = Scene(sim, case, init)
    n, E = case["n"], RC.E
    ids, rnd, ws, st, h = _ptr(s.ids), _ptr(s.rnd), s.ws.ptr(), _stream(), s.h()
    good, pb = s.bufs(), s.task_bufs()
    bad_bufs = []
    for field in ("gts", "lrs", "motion_len", "heightfield", "amp_obs_buf", "ground_h", "valid_x"):
        b = s.bufs()
        setattr(b, field, None)
        bad_bufs.append((field, b))
    b = s.bufs(flags=RC.REAL_PATH, n_real=RC.N_REAL)
    b.real_traj = None
    bad_bufs.append(("real_traj", b))
    b = s.bufs(n_motions=0)
    bad_bufs.append(("n_motions", b))
    R_ = lambda x: C.byref(x)
    calls = [("reset: null sim", lambda: lib.emloco_task_reset(None, R_(good), ids, n, rnd, st)),
             ("reset: null bufs", lambda: lib.emloco_task_reset(h, None, ids, n, rnd, st)),
             ("reset: null ids", lambda: lib.emloco_task_reset(h, R_(good), None, n, rnd, st)),
             ("reset: null rows", lambda: lib.emloco_task_reset(h, R_(good), ids, n, None, st)),
             ("reset: n < 0", lambda: lib.emloco_task_reset(h, R_(good), ids, -1, rnd, st)),
             ("reset: n > n_env", lambda: lib.emloco_task_reset(h, R_(good), ids, E + 1, rnd, st)),
             ("seeded: null sim", lambda: lib.emloco_task_reset_seeded(None, R_(good), ids, n, C.c_uint64(5), ws, st)),
             ("seeded: null bufs", lambda: lib.emloco_task_reset_seeded(h, None, ids, n, C.c_uint64(5), ws, st)),
             ("seeded: null ids", lambda: lib.emloco_task_reset_seeded(h, R_(good), None, n, C.c_uint64(5), ws, st)),
             ("seeded: null workspace", lambda: lib.emloco_task_reset_seeded(h, R_(good), ids, n, C.c_uint64(5), None, st)),
             ("seeded: n < 0", lambda: lib.emloco_task_reset_seeded(h, R_(good), ids, -1, C.c_uint64(5), ws, st)),
             ("seeded: n > n_env", lambda: lib.emloco_task_reset_seeded(h, R_(good), ids, E + 1, C.c_uint64(5), ws, st)),
             ("history: null bufs", lambda: lib.emloco_task_reset_amp_history(None, ids, n, st)),
             ("history: null ids", lambda: lib.emloco_task_reset_amp_history(R_(good), None, n, st)),
             ("history: n < 0", lambda: lib.emloco_task_reset_amp_history(R_(good), ids, -1, st)),
             ("reset_obs: null sim", lambda: lib.emloco_task_reset_obs(None, R_(good), R_(pb), 0, None, ids, n, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: null reset bufs", lambda: lib.emloco_task_reset_obs(h, None, R_(pb), 0, None, ids, n, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: null task bufs", lambda: lib.emloco_task_reset_obs(h, R_(good), None, 0, None, ids, n, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: null ids", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), 0, None, None, n, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: n < 0", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), 0, None, ids, -1, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: n > n_env", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), 0, None, ids, E + 1, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: no rows, no workspace", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), 0, None, ids, n, C.c_uint64(5), None, None, st)),
             ("reset_obs: live role without snapshot", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), POST_OBS, None, ids, n, C.c_uint64(5), ws, rnd, st)),
             ("reset_obs: live role with a reward bit", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb), 4, _ptr(s.i["reset"].buf, TAIL), ids, n, C.c_uint64(5), ws, rnd, st))]
    for name, b in bad_bufs:
        calls.append(("reset: " + name, lambda b=b: lib.emloco_task_reset(h, R_(b), ids, n, rnd, st)))
        calls.append(("seeded: " + name, lambda b=b: lib.emloco_task_reset_seeded(h, R_(b), ids, n, C.c_uint64(5), ws, st)))
        calls.append(("reset_obs: " + name, lambda b=b: lib.emloco_task_reset_obs(h, R_(b), R_(pb), 0, None, ids, n, C.c_uint64(5), ws, None, st)))
        if name in ("gts", "lrs", "motion_len", "amp_obs_buf"):
            calls.append(("history: " + name, lambda b=b: lib.emloco_task_reset_amp_history(R_(b), ids, n, st)))
    pb_bad = s.task_bufs()
    pb_bad.n_env = E - 1
    calls.append(("reset_obs: env counts disagree", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb_bad), 0, None, ids, n, C.c_uint64(5), ws, rnd, st)))
    pb_bad2 = s.task_bufs()
    pb_bad2.obs_buf = None
    calls.append(("reset_obs: no observation buffer", lambda: lib.emloco_task_reset_obs(h, R_(good), R_(pb_bad2), 0, None, ids, n, C.c_uint64(5), ws, rnd, st)))
    wrote = []
    for name, call in calls:
        assert call() != 0, (name, "was accepted")
        torch.cuda.synchronize()
        if not s.untouched():
            wrote.append(name)
            s = Scene(sim, case, init)
            ids, rnd, ws, good, pb = _ptr(s.ids), _ptr(s.rnd), s.ws.ptr(), s.bufs(), s.task_bufs()
    assert not wrote, ("refused calls that wrote", wrote)
    # n = 0: nothing to do, nothing written
    assert lib.emloco_task_reset(h, R_(good), ids, 0, rnd, st) == 0 and lib.emloco_task_reset_seeded(h, R_(good), ids, 0, C.c_uint64(5), ws, st) == 0
    assert lib.emloco_task_reset_amp_history(R_(good), ids, 0, st) == 0
    assert lib.emloco_task_reset_obs(h, R_(good), R_(pb), 0, None, ids, 0, C.c_uint64(5), ws, None, st) == 0
    torch.cuda.synchronize()
    assert s.untouched()

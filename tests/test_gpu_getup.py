"""Device run of the get-up entry points (include/emloco_task.h: emloco_getup_split / _apply / _amp_default / _flags) and of the task
built on them (emloco_amd/env/tasks/humanoid_pedestrain_terrain_getup.py).

Split, flags, AMP default: the cases of tests/getup_cases.py against tests/getup_ref.py, as tests/test_emu_getup.py runs them on the
emulator -- integer logic and copies, compared exactly.  Apply: 64 envs, against EXISTING entry points (emloco_sim_set_*_indexed on a
second simulator for the body state, emloco_task_traj_reset with the same rows for the trajectory), bit for bit; the waypoints against
the float64 polyline at the bar tests/test_gpu_env.py holds waypoint_traj to (rtol = atol = 1e-5).  Task: 64 envs on the default flat
terrain with the synthetic motion library.

Task case (i) at probabilities (0, 0) is byte-equal to HumanoidPedestrianTerrain from the first reset on (the get-up task has run
its 150 pool frames on the simulator by then: every buffer they leave behind that a reset does not rewrite would show here).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import getup_cases as GC                                                         # noqa: E402
import getup_ref as GR                                                           # noqa: E402
import kernel_refs as R                                                          # noqa: E402

DEV = "cuda:0"
CASES = GC.split_cases()
CFG_GETUP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emloco_amd", "data", "cfg", "pacer_getup.yaml")


def _lib():
    from emloco_amd import _lib as L
    return L.require_device()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class DevState:
    """a state dict of getup_cases on the device, and its EmlocoGetupBufs"""

    def __init__(self, st):
        from emloco_amd import _lib as L
        self.t = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in st.items()}
        t = self.t
        self.bufs = L.GetupBufs(int(t["assign"].numel()), int(t["pool_taken"].numel()), *[t[k].data_ptr() for k in (
            "pool_root", "pool_dof", "pool_taken", "assign", "counter", "progress", "reset", "terminate", "split_ws", "stats")])

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _split(ds, case, out=None):
    n = case["n"]
    out = out or {k: torch.full((n + 1,), -77, dtype=torch.int32, device=DEV) for k in GC.LIST_KEYS}
    ids = torch.from_numpy(np.concatenate([case["ids"], [-1]]).astype(np.int32)).to(DEV)        # (an empty list still has an address)
    rnd = None if case["rnd"] is None or n == 0 else torch.from_numpy(case["rnd"]).to(DEV)
    rc = _lib().emloco_getup_split(C.byref(ds.bufs), _ptr(ids), n, _ptr(rnd), C.c_uint64(case["seed"]), case["recovery_prob"], case["fall_prob"],
                                   case["steps"], case["key"], *[_ptr(out[k]) for k in GC.LIST_KEYS], _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0]["name"] for c in CASES])
def test_split_equals_the_reference(index):
    case, st0 = CASES[index]
    ds = DevState(st0)
    rc, out = _split(ds, case)
    assert rc == 0
    GC.judge_split(case, st0, ds.host(), {k: v.cpu().numpy() for k, v in out.items()})


def test_flags_equal_the_reference():
    st0 = GC.flags_state()
    ds = DevState(st0)
    for _ in range(3):
        assert _lib().emloco_getup_flags(C.byref(ds.bufs), _stream()) == 0
        st0 = GR.flags(st0)
        got = ds.host()
        for k in ("counter", "reset", "terminate", "progress", "stats", "assign", "pool_taken"):
            assert np.array_equal(got[k], st0[k]), k


@pytest.mark.parametrize("ring", [0, 9])
def test_amp_default_fills_the_history_with_the_newest_row(ring):
    from emloco_amd import _lib as L
    amp0, ids = GC.amp_case(ring)
    amp, dids = torch.from_numpy(amp0).to(DEV), torch.from_numpy(ids).to(DEV)
    tb = L.TaskBufs()
    tb.n_env, tb.amp_obs_buf, tb.amp_ring = amp0.shape[0], amp.data_ptr(), ring
    assert _lib().emloco_getup_amp_default(C.byref(tb), _ptr(dids), len(ids), _stream()) == 0
    torch.cuda.synchronize()
    got = amp.cpu().numpy()
    assert np.array_equal(got.view(np.int32), GR.amp_default(amp0, ring, ids).view(np.int32))
    e = ids[0]
    assert all(np.array_equal(got[e, k], amp0[e, GR.phys_row(ring, 0)]) for k in range(GC.AMP_STEPS))
    others = np.setdiff1d(np.arange(amp0.shape[0]), ids[ids >= 0])
    assert np.array_equal(got[others], amp0[others])


# ---------------------------------------------------------------------------------------------- apply, 64 envs
E = 64
DT = 1.0 / 30.0
VERT_DT = 168 * DT / 100.0


@pytest.fixture(scope="module")
def sims():
    from emloco_amd.model import pack_models
    from emloco_amd.sim import NativeSim
    from helpers import varied_models
    models = pack_models(varied_models(E, seed=4))
    a, b = NativeSim(models), NativeSim(models)
    yield a, b
    torch.cuda.synchronize()
    a.close()
    b.close()


class ApplyScene:
    """two simulators in the same (consistent) state with garbage warm-start impulses and contact forces; a pool of other poses; the
    buffers of an EmlocoResetBufs that carries the trajectory fields"""

    def __init__(self, sims):
        from emloco_amd import _lib as L
        from helpers import scene_state
        self.L, self.a, self.b = L, *sims
        root, dof, _ = scene_state(E, seed=1)
        g = torch.Generator().manual_seed(21)
        self.all_ids = torch.arange(E, dtype=torch.int32, device=DEV)
        for s in sims:
            s.set_root_state_indexed(torch.from_numpy(root).to(DEV), self.all_ids)
            s.set_dof_state_indexed(torch.from_numpy(dof).to(DEV).view(E, -1), self.all_ids)
            s.warm_start.copy_(torch.randn(s.warm_start.shape, generator=g).to(DEV))
            s.contact_force.copy_(torch.randn(s.contact_force.shape, generator=g).to(DEV))
            g.manual_seed(21)
        proot, pdof, _ = scene_state(E, seed=2, height=0.4)
        proot[:, 7:13] = 0
        pdof[:, :, 1] = 0
        st = GC.state(np.random.default_rng(8))
        st = {k: v[:E].copy() if k not in ("stats",) else v.copy() for k, v in st.items()}
        st.update(pool_root=proot, pool_dof=pdof, pool_taken=np.zeros(E, np.uint8), assign=np.full(E, -1, np.int32),
                  terminate=(np.arange(E) % 3 != 0).astype(np.int64), split_ws=np.zeros(E, np.int32))
        st["pool_taken"][[5, 17]] = 1                                 # taken for good
        self.st0 = st
        self.ds = DevState(st)
        f = lambda *s: torch.full(s, float("nan"), device=DEV)
        self.verts, self.verts2 = f(E, 101 * 3), f(E, 101 * 3)
        self.inv, self.inv2 = torch.full((E,), 7, dtype=torch.uint8, device=DEV), torch.full((E,), 7, dtype=torch.uint8, device=DEV)
        self.way, self.pose, self.vel = f(E, 45), f(E, 72), f(E, 2)
        g.manual_seed(22)
        self.rnd_fall, self.rnd_rec = (torch.rand(E, L.RESET_RND, generator=g).to(DEV) for _ in range(2))
        self.lists = {k: torch.full((E + 1,), -77, dtype=torch.int32, device=DEV) for k in GC.LIST_KEYS}

    def reset_bufs(self, verts, inv):
        L = self.L
        b = L.ResetBufs()
        b.flags = L.RESET_INIT_HEADING | L.RESET_HEADING_INVERSION | L.RESET_ADJUST_ROOT_VEL
        b.dt, b.vert_dt, b.dtheta_max, b.speed_min, b.speed_max, b.accel_max, b.sharp_prob, b.hybrid_prob = DT, VERT_DT, 2.0, 0.0005, 3.0, 2.0, 0.02, 0.5
        b.traj_dur, b.sample_dt = 101 * VERT_DT, 0.4
        t = self.ds.t
        b.traj_verts, b.inverted = verts.data_ptr(), inv.data_ptr()
        b.progress_buf, b.reset_buf, b.terminate_buf = t["progress"].data_ptr(), t["reset"].data_ptr(), t["terminate"].data_ptr()
        b.waypoint_traj, b.init_pose, b.init_vel = self.way.data_ptr(), self.pose.data_ptr(), self.vel.data_ptr()
        return b

    def split(self):
        ids = torch.arange(E, dtype=torch.int32, device=DEV)
        u = torch.rand(E, 2, generator=torch.Generator().manual_seed(23)).to(DEV)
        rc = _lib().emloco_getup_split(C.byref(self.ds.bufs), _ptr(ids), E, _ptr(u), C.c_uint64(0), 0.4, 0.5, 60, 0xBEEF, *[_ptr(self.lists[k]) for k in GC.LIST_KEYS],
                                       _stream())
        assert rc == 0
        torch.cuda.synchronize()
        n = {k: int(v[E]) for k, v in self.lists.items()}
        assert n["fall"] >= 8 and n["recover"] >= 8 and n["normal"] >= 8, n
        return {k: v[:n[k]].long() for k, v in self.lists.items()}

    def apply(self, **kw):
        b = self.reset_bufs(self.verts, self.inv)
        a = dict(sim=self.a._h, b=C.byref(b), g=C.byref(self.ds.bufs), fall=_ptr(self.lists["fall"]), slot=_ptr(self.lists["fall_slot"]),
                 rec=_ptr(self.lists["recover"]), n=E, rf=_ptr(self.rnd_fall), rr=_ptr(self.rnd_rec), seed=C.c_uint64(0), ws=None)
        a.update(kw)
        rc = _lib().emloco_getup_apply(a["sim"], a["b"], a["g"], a["fall"], a["slot"], a["rec"], a["n"], a["rf"], a["rr"], a["seed"], a["ws"], _stream())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        torch.cuda.synchronize()
        s = {k: getattr(self.a, k).view(E, -1).clone() for k in ("root_state", "dof_state", "rigid_body_state", "warm_start", "contact_force")}
        s.update({"t_" + k: v.clone() for k, v in self.ds.t.items()})
        s.update(verts=self.verts.clone(), inv=self.inv.clone(), way=self.way.clone(), pose=self.pose.clone(), vel=self.vel.clone())
        return s


def test_apply_against_the_existing_entry_points(sims):
    sc = ApplyScene(sims)
    ids = sc.split()
    fall, slot, rec, normal = ids["fall"], ids["fall_slot"], ids["recover"], ids["normal"]
    before = sc.snapshot()
    assert sc.apply() == 0
    after = sc.snapshot()
    a, b, t = sc.a, sc.b, sc.ds.t
    # fall envs: the pool rows, byte for byte; impulses zero; the body state of the indexed setters on a second simulator
    V = lambda x: x.view(E, -1)
    assert _same(V(a.root_state)[fall], t["pool_root"][slot]) and _same(V(a.dof_state)[fall], t["pool_dof"][slot].view(len(fall), -1))
    assert not V(a.warm_start)[fall].any()
    full_root, full_dof = b.root_state.clone(), b.dof_state.clone()
    V(full_root)[fall], V(full_dof)[fall] = t["pool_root"][slot], t["pool_dof"][slot].view(len(fall), -1)
    fall32 = sc.lists["fall"][:len(fall)].contiguous()
    b.set_root_state_indexed(full_root, fall32)
    b.set_dof_state_indexed(full_dof, fall32)
    torch.cuda.synchronize()
    rb = lambda s: s.rigid_body_state.view(E, 24, 13)
    assert _same(rb(a)[fall], rb(b)[fall]) and not _same(rb(a)[fall], before["rigid_body_state"].view(E, 24, 13)[fall])
    root = V(a.root_state)
    # recovery envs: the simulator's state untouched, bit for bit
    for k in ("root_state", "dof_state", "rigid_body_state", "warm_start"):
        assert _same(after[k][rec], before[k][rec]), k
    # normal envs (not listed): nothing at all
    for k in before:
        if k not in ("t_split_ws", "t_stats") and before[k].shape[0] == E:
            assert _same(after[k][normal], before[k][normal]), k
    # both lists: flags, contact forces, trajectory = emloco_task_traj_reset with the same rows, root positions and velocities
    for env, rows, name in ((fall, sc.rnd_fall, "fall"), (rec, sc.rnd_rec, "recover")):
        for k in ("progress", "reset", "terminate"):
            assert not t[k][env].any(), (name, k)
        assert not _bits(a.contact_force.view(E, -1)[env]).any(), name
        b2 = sc.reset_bufs(sc.verts2, sc.inv2)
        pos, vel = root[env][:, 0:3].contiguous(), root[env][:, 7:10].contiguous()
        e32 = env.to(torch.int32).contiguous()
        assert _lib().emloco_task_traj_reset(C.byref(b2), _ptr(e32), len(env), _ptr(rows), _ptr(pos), _ptr(vel), _stream()) == 0
        torch.cuda.synchronize()
        assert _same(sc.verts[env], sc.verts2[env]) and torch.equal(sc.inv[env], sc.inv2[env]), name
        assert torch.isfinite(sc.verts[env]).all() and set(sc.inv[env].tolist()) <= {0, 1}
        v = sc.verts[env].view(-1, 101, 3).cpu()
        times = (torch.arange(15, dtype=torch.float64) * float(np.float32(0.4)))[None, :].expand(len(env), 15)
        want = R.traj_calc_pos(v, times, float(np.float32(101 * VERT_DT)))
        np.testing.assert_allclose(sc.way[env].view(-1, 15, 3).cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-5, err_msg=name)
        assert _same(sc.pose[env].view(-1, 24, 3), rb(a)[env][:, :, 0:3]) and _same(sc.vel[env], root[env][:, 7:9]), name
    assert set(sc.inv[torch.cat([fall, rec])].tolist()) == {0, 1}            # both outcomes of the inversion draw occur
    for k in ("t_pool_root", "t_pool_dof", "t_pool_taken", "t_assign", "t_counter"):
        assert _same(after[k], before[k]), k


def test_apply_with_rows_made_on_the_device(sims):
    """no rows supplied: the workspace's rows are the device hash of (seed | ~seed, entry), and the result is the call with those rows"""
    sc = ApplyScene(sims)
    ids = sc.split()
    seed = 0xC0FFEE1234
    ws = torch.full((2 * E, sc.L.RESET_RND), -3.0, device=DEV)
    assert sc.apply(rf=None, rr=None, seed=C.c_uint64(seed), ws=_ptr(ws)) == 0
    got = sc.snapshot()
    nf, nr = len(ids["fall"]), len(ids["recover"])
    assert _same(ws[0].cpu(), R.reset_rnd_row(seed, 0)) and _same(ws[nf - 1].cpu(), R.reset_rnd_row(seed, nf - 1))
    assert _same(ws[E + nr - 1].cpu(), R.reset_rnd_row(seed ^ 0xFFFFFFFFFFFFFFFF, nr - 1))
    assert (ws[nf:E] == -3.0).all() and (ws[E + nr:] == -3.0).all()
    sc2 = ApplyScene(sims)
    sc2.split()
    sc2.rnd_fall, sc2.rnd_rec = ws[:E].contiguous(), ws[E:].contiguous()
    assert sc2.apply() == 0
    want = sc2.snapshot()
    for k in got:
        assert _same(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------- refusals
def _refusals(sc, which):
    lib, st = _lib(), _stream()
    L, g, lists = sc.L, sc.ds.bufs, sc.lists
    R_ = C.byref
    ids = _ptr(sc.all_ids)
    lp = [_ptr(lists[k]) for k in GC.LIST_KEYS]
    u = torch.rand(E, 2, device=DEV)

    def without(field, value=None):
        b = type(g).from_buffer_copy(g)
        setattr(b, field, value)
        return b

    if which == "split":
        call = lambda g_=g, ids_=ids, n=E, out=lp: lib.emloco_getup_split(None if g_ is None else R_(g_), ids_, n, _ptr(u), C.c_uint64(1), 0.5, 0.5, 60, 7, *out, st)
        bad = [("null structure", lambda: call(g_=None)), ("null list", lambda: call(ids_=None)), ("n < 0", lambda: call(n=-1)),
               ("n > n_env", lambda: call(n=E + 1)), ("no pool", lambda: call(g_=without("n_pool", 0)))]
        bad += [("null output " + k, lambda i=i: call(out=lp[:i] + [None] + lp[i + 1:])) for i, k in enumerate(GC.LIST_KEYS)]
        bad += [("missing " + f, lambda f=f: call(g_=without(f))) for f in ("pool_root", "pool_taken", "assign", "recovery_counter", "terminate_buf", "split_ws")]
        return bad
    if which == "flags":
        call = lambda g_: lib.emloco_getup_flags(None if g_ is None else R_(g_), st)
        return [("null structure", lambda: call(None)), ("n_env 0", lambda: call(without("n_env", 0)))] + \
               [("missing " + f, lambda f=f: call(without(f))) for f in ("recovery_counter", "reset_buf", "terminate_buf", "progress_buf")]
    if which == "amp_default":
        amp = torch.zeros(E, 15, 206, device=DEV)
        sc.extra = amp

        def tb(**kw):
            b = L.TaskBufs()
            b.n_env, b.amp_obs_buf, b.amp_ring = E, amp.data_ptr(), 0
            for k, v in kw.items():
                setattr(b, k, v)
            return b
        call = lambda b, ids_=ids, n=E: lib.emloco_getup_amp_default(None if b is None else R_(b), ids_, n, st)
        return [("null structure", lambda: call(None)), ("null list", lambda: call(tb(), ids_=None)), ("n < 0", lambda: call(tb(), n=-1)),
                ("n > n_env", lambda: call(tb(), n=E + 1)), ("no AMP buffer", lambda: call(tb(amp_obs_buf=None))), ("bad ring", lambda: call(tb(amp_ring=16)))]
    assert which == "apply"
    good = sc.reset_bufs(sc.verts, sc.inv)

    def rb_without(field):
        b = sc.reset_bufs(sc.verts, sc.inv)
        setattr(b, field, None)
        return b
    real = sc.reset_bufs(sc.verts, sc.inv)
    real.flags |= L.RESET_REAL_PATH
    real.n_real = 5
    call = sc.apply
    ws = torch.zeros(2 * E, L.RESET_RND, device=DEV)
    sc.extra = ws
    bad = [("null sim", lambda: call(sim=None)), ("null reset structure", lambda: call(b=None)), ("null get-up structure", lambda: call(g=None)),
           ("null fall list", lambda: call(fall=None)), ("null slots", lambda: call(slot=None)), ("null recovery list", lambda: call(rec=None)),
           ("n < 0", lambda: call(n=-1)), ("n > n_env", lambda: call(n=E + 1)), ("one random block", lambda: call(rr=None)),
           ("the other random block", lambda: call(rf=None, ws=_ptr(ws))), ("no rows, no workspace", lambda: call(rf=None, rr=None)),
           ("real path without data", lambda: call(b=R_(real))), ("env counts disagree", lambda: call(g=R_(without("n_env", E - 1))))]
    bad += [("missing " + f, lambda f=f: call(b=R_(rb_without(f)))) for f in ("traj_verts", "inverted", "progress_buf", "waypoint_traj", "init_pose", "init_vel")]
    bad += [("missing " + f, lambda f=f: call(g=R_(without(f)))) for f in ("pool_root", "pool_dof", "assign")]
    return bad


@pytest.mark.parametrize("which", ["split", "apply", "amp_default", "flags"])
def test_refused_calls_write_nothing(sims, which):
    sc = ApplyScene(sims)
    sc.split()
    sc.extra = None
    calls = _refusals(sc, which)
    before, extra0 = sc.snapshot(), None if sc.extra is None else sc.extra.clone()
    lists0 = {k: v.clone() for k, v in sc.lists.items()}
    wrote = []
    for name, call in calls:
        assert call() != 0, (which, name, "was accepted")
        torch.cuda.synchronize()
        after = sc.snapshot()
        if not (all(_same(after[k], before[k]) for k in before) and all(torch.equal(sc.lists[k], lists0[k]) for k in lists0)
                and (extra0 is None or _same(sc.extra, extra0))):
            wrote.append(name)
    assert not wrote, (which, "refused calls that wrote", wrote)
    if which == "apply":                                              # n = 0: nothing to do, nothing written
        assert sc.apply(n=0) == 0 and all(_same(v, before[k]) for k, v in sc.snapshot().items())


# ---------------------------------------------------------------------------------------------- the task
def _make_env(num_envs=64, getup=True):
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    extra = ["--task", "HumanoidPedestrianTerrainGetup", "--cfg_env", CFG_GETUP] if getup else []
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", *extra])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    return create_rlgpu_env(args, cfg, cfg_train)


def _rows(seed, n=64):
    from emloco_amd import _lib as L
    return torch.rand(n, L.RESET_RND, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _actions(seed, scale, n=64):
    return (torch.randn(n, 69, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


STATE = ("obs_buf", "_root_states", "_dof_state", "_rigid_body_state", "progress_buf", "reset_buf", "_terminate_buf", "rew_buf", "_amp_obs_buf",
         "waypoint_traj", "init_pose", "init_vel")


def test_task_with_the_feature_off_is_the_parent_task():
    """(i) probabilities (0, 0): after reset() of all envs with explicit rows and after 3 steps with fixed actions, byte-equal to
    HumanoidPedestrianTerrain from the same configuration, seed, rows and actions"""
    eg, ep = _make_env(getup=True), _make_env(getup=False)
    tg, tp = eg.task, ep.task
    assert type(tp).__name__ == "HumanoidPedestrianTerrain" and type(tg).__name__ == "HumanoidPedestrianTerrainGetup"
    tg._recovery_episode_prob, tg._fall_init_prob = 0.0, 0.0
    all_ids = torch.arange(64, device=DEV)
    rnd = _rows(31)
    tg._fused_reset_envs(all_ids, rnd=rnd)
    tp._fused_reset_envs(all_ids, rnd=rnd)

    def compare(where):
        torch.cuda.synchronize()
        for name in STATE:
            assert _same(getattr(tg, name), getattr(tp, name)), (where, name)
        assert _same(tg._traj_gen._verts, tp._traj_gen._verts), (where, "trajectory")
        if isinstance(tg.inverted, torch.Tensor):
            assert torch.equal(tg.inverted, tp.inverted), (where, "inverted")
    compare("reset")
    assert not tg._recovery_counter.any() and (tg._fall_assign == -1).all()
    for k in range(3):
        act = _actions(40 + k, 0.3)
        eg.step(act)
        ep.step(act)
        compare(f"step {k}")
    # the sync-free reset of the finished envs, with rows: the same again
    tg.reset_buf[3:40:4] = 1
    tp.reset_buf[3:40:4] = 1
    rnd = _rows(32)
    n_done = int(tg.reset_buf.sum())
    tg.reset_done(rnd=rnd)
    tp.reset_done(rnd=rnd)
    compare("reset_done")
    s = tg.getup_epoch_stats()
    assert s["getup_normal_share"] == 1.0 and n_done >= 10 and s["getup_resets"] == 64 + n_done and s["getup_mean_recovery_counter"] == 0.0


def test_recovery_episodes_keep_the_fallen_state_and_cannot_terminate():
    """(ii) probabilities (1, 0)"""
    env = _make_env()
    t = env.task
    steps = t._recovery_steps
    t._recovery_episode_prob, t._fall_init_prob = 0.0, 0.0
    t._fused_reset_envs(torch.arange(64, device=DEV), rnd=_rows(51))
    for k in range(60):                                               # flail until some envs have fallen
        env.step(_actions(60 + k, 1.5))
        if int(t._terminate_buf.sum()) >= 6:
            break
    torch.cuda.synchronize()
    term = (t._terminate_buf == 1).nonzero().flatten()
    assert len(term) >= 6 and (t.reset_buf[term] == 1).all(), "no env fell: the test needs terminated envs"
    alive = (t.reset_buf == 0).nonzero().flatten()
    timed = alive[:3]                                                 # a timeout without a termination, as the post-physics pass leaves it
    t.reset_buf[timed] = 1
    t._terminate_buf[timed] = 0
    keep = ("_root_states", "_dof_state", "_rigid_body_state")
    before = {k: getattr(t, k).clone() for k in keep}
    warm = t.sim.native.warm_start.clone()
    t._recovery_episode_prob, t._fall_init_prob = 1.0, 0.0
    t.getup_epoch_stats()
    t.reset_done(rnd=_rows(52))
    torch.cuda.synchronize()
    for k in keep:
        rows = lambda x: x.view(64, -1)
        assert _same(rows(getattr(t, k))[term], rows(before[k])[term]), k
        assert not _same(rows(getattr(t, k))[timed], rows(before[k])[timed]), (k, "a timed-out env was not reset")
    assert _same(t.sim.native.warm_start.view(64, -1)[term], warm.view(64, -1)[term])
    assert (t._recovery_counter[term] == steps).all() and not t._recovery_counter[timed].any() and not t._recovery_counter[alive[3:]].any()
    assert not t.progress_buf[term].any() and not t.reset_buf.any() and not t.progress_buf[timed].any()
    s = t.getup_epoch_stats()
    assert s["getup_resets"] == len(term) + 3 and s["getup_recovery_share"] == len(term) / (len(term) + 3) and s["getup_fall_share"] == 0.0
    for k in range(steps):
        env.step(_actions(200 + k, 1.5))
        torch.cuda.synchronize()
        if k < steps - 1:
            assert (t._recovery_counter[term] == steps - 1 - k).all(), k
            assert not t.reset_buf[term].any() and not t._terminate_buf[term].any() and not t.progress_buf[term].any(), k
        else:
            assert not t._recovery_counter[term].any() and (t.progress_buf[term] == 1).all()
        t.reset_done()                                                # the others go on finishing (and turn into recovery episodes)
    assert t.getup_epoch_stats()["getup_mean_recovery_counter"] > 0


def test_fall_resets_start_from_distinct_pool_rows():
    """(iii) probabilities (0, 1)"""
    env = _make_env()
    t = env.task
    t._recovery_episode_prob, t._fall_init_prob = 0.0, 1.0
    free = int((t._fall_taken == 0).sum())
    assert free >= 60, "most pool rows must be usable"
    t.reset()
    torch.cuda.synchronize()
    slot = t._fall_assign.long()
    fell = (slot >= 0).nonzero().flatten()
    assert len(fell) == free and len(set(slot[fell].tolist())) == free and (t._fall_taken[slot[fell]] == 1).all()
    assert _same(t._root_states[fell], t._fall_root_states[slot[fell]])
    dof = t._dof_state.view(64, 69, 2)
    assert _same(dof[fell], t._fall_dof_state[slot[fell]]) and not dof[fell][:, :, 1].any()
    assert (t._recovery_counter[fell] == t._recovery_steps).all() and not t.progress_buf.any() and not t.reset_buf.any()
    amp = t._amp_obs_buf[fell]
    assert torch.isfinite(amp).all() and all(_same(amp[:, k], amp[:, 0]) for k in range(1, 15))
    assert torch.isfinite(t.obs_buf).all()
    # with the AMP history as a ring the rows still all equal the newest one
    t.enable_amp_ring(True)
    env.step(_actions(7, 0.1))
    t.reset_buf[:] = 1
    t.reset_done()
    torch.cuda.synchronize()
    logical = t.amp_obs_logical().view(64, 15, 206)[(t._fall_assign >= 0)]
    assert all(_same(logical[:, k], logical[:, 0]) for k in range(1, 15))


def test_launch_arrangements_raise_on_the_getup_task():
    """(iv)"""
    t = _make_env().task
    for name in ("fused_chain", "overlap_obs", "overlap_reset"):
        with pytest.raises(RuntimeError, match="sequential launch arrangement"):
            setattr(t, name, True)
        assert getattr(t, name) is False
    with pytest.raises(RuntimeError, match="sequential launch arrangement"):
        t.attach_returns(object())


def test_generate_fall_states_leaves_a_pool_of_fallen_poses():
    """(v)"""
    t = _make_env().task
    t._fall_assign[:5] = torch.arange(5, dtype=torch.int32, device=DEV)
    t._fall_taken[:5] = 1
    t._generate_fall_states()
    torch.cuda.synchronize()
    ok = t._fall_taken == 0
    assert int(ok.sum()) >= 60 and (t._fall_assign == -1).all()
    assert torch.isfinite(t._fall_root_states[ok]).all() and torch.isfinite(t._fall_dof_state[ok]).all()
    assert not t._fall_root_states[:, 7:13].any() and not t._fall_dof_state[:, :, 1].any()
    standing = float(t._initial_humanoid_root_states[:, 2].mean())
    assert float(t._fall_root_states[ok][:, 2].mean()) < standing, (float(t._fall_root_states[ok][:, 2].mean()), standing)
    # a row that blew up is taken for good
    bad = ~(torch.isfinite(t._fall_root_states).all(1) & torch.isfinite(t._fall_dof_state).flatten(1).all(1))
    assert torch.equal(t._fall_taken.bool(), bad)


def test_host_reset_path_restates_the_same_structure():
    """fused_reset off: `_reset_actors` in torch -- fall envs start from distinct pool rows with the history filled from the newest row,
    recovery envs keep their state, everything else takes the parent's reset; counters and slots as on the device path"""
    env = _make_env()
    t = env.task
    t._fused_reset = False
    steps = t._recovery_steps
    t._recovery_episode_prob, t._fall_init_prob = 0.0, 1.0
    free = int((t._fall_taken == 0).sum())
    t.reset()
    torch.cuda.synchronize()
    slot = t._fall_assign.long()
    fell = (slot >= 0).nonzero().flatten()
    assert len(fell) == free >= 60 and len(set(slot[fell].tolist())) == free and (t._fall_taken[slot[fell]] == 1).all()
    assert _same(t._root_states[fell], t._fall_root_states[slot[fell]]) and _same(t._dof_state.view(64, 69, 2)[fell], t._fall_dof_state[slot[fell]])
    assert (t._recovery_counter[fell] == steps).all() and not t.progress_buf.any() and not t.reset_buf.any()
    amp = t._amp_obs_buf[fell]
    assert torch.isfinite(amp).all() and all(_same(amp[:, k], amp[:, 0]) for k in range(1, 15)) and torch.isfinite(t.obs_buf).all()
    # recovery (terminated) beside normal (timed out)
    t._recovery_episode_prob, t._fall_init_prob = 1.0, 0.0
    ids = torch.arange(16, device=DEV)
    t.reset_buf[ids] = 1
    t._terminate_buf[:8] = 1
    t._recovery_counter[:] = 7
    before = (t._root_states.clone(), t._dof_state.clone())
    t.getup_epoch_stats()
    t.reset(ids)
    torch.cuda.synchronize()
    assert _same(t._root_states[:8], before[0][:8]) and _same(t._dof_state.view(64, -1)[:8], before[1].view(64, -1)[:8])
    assert not _same(t._root_states[8:16], before[0][8:16]) and _same(t._root_states[16:], before[0][16:])
    assert (t._recovery_counter[:8] == steps).all() and not t._recovery_counter[8:16].any() and (t._recovery_counter[16:] == 7).all()
    assert (t._fall_assign[:16] == -1).all() and int(t._fall_taken.sum()) == int((t._fall_assign >= 0).sum()) + (64 - free)
    assert not t.reset_buf.any() and not t._terminate_buf[:16].any() and not t.progress_buf[:16].any()
    s = t.getup_epoch_stats()
    assert s["getup_resets"] == 16 and s["getup_recovery_share"] == 0.5 and s["getup_normal_share"] == 0.5

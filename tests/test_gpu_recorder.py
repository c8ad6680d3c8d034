"""Device: the flight recorder (csrc/recorder_kernels.hip behind emloco_recorder_record / emloco_recorder_check, learning/flight_recorder.py)
-- the case tables of tests/recorder_cases.py that tests/test_emu_recorder.py runs on the emulator, the refusals, and the whole chain:
NativeSim runs whose captures are the ones the oracle's run predicts and replay clean, and a task run that the recorder leaves bit for
bit as it is without it."""
import ctypes as C

import numpy as np
import pytest
import torch

import flight_recorder_ref as R
import recorder_cases as cases

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5A5A5A5 - (1 << 32)             # (int32 tensors: the guard word as a signed value)


class DeviceBackend:
    """The recorder's buffers as device tensors and its two entry points; the interface of tests/emu_recorder.py: EmuBackend."""

    def __init__(self, E, R_, C_, cause_mask=31, speed2=0.0, ang2=0.0, early_fall=0, drive_mode=0, grid=0, request=True):
        from emloco_amd import _lib as L
        self.lib, self.L = L.require_device(), L
        self.E, self.R, self.C = E, R_, C_
        dev = torch.device("cuda", 0)
        host = R.synthetic_state(E, request=request)
        self.st = {k: (None if v is None else torch.from_numpy(v.copy()).to(dev)) for k, v in host.items()}
        n_ring, n_slots = E * R_ * R.REC_WORDS, C_ * R.slot_words(R_)
        self._ring_whole = torch.full((n_ring + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
        self._slots_whole = torch.full((n_slots + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
        self.ring, self.slots = self._ring_whole[GUARD:GUARD + n_ring], self._slots_whole[GUARD:GUARD + n_slots]
        self.ring.zero_()
        self.slots.zero_()
        self.counters = torch.zeros(R.COUNTERS, dtype=torch.int32, device=dev)
        self.last = torch.full((E,), R.NEVER, dtype=torch.int32, device=dev)
        self.cause_ws = torch.full((E,), -1, dtype=torch.int32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        s = self.st
        self.bufs = L.RecorderBufs(E, R_, C_, drive_mode, 0, cause_mask, early_fall, grid, speed2, ang2,
                                   p(s["root"]), p(s["dof"]), p(s["warm"]), p(s["drive"]), p(s["rb"]), p(s["cf"]), p(s["df"]),
                                   p(s["progress"]), p(s["reset"]), p(s["terminate"]), p(self.ring), p(self.slots), p(self.counters),
                                   p(self.last), p(self.cause_ws), p(s["request"]))
        self.t0 = None

    def push(self, st):
        for k, v in self.st.items():
            if v is not None:
                v.copy_(torch.from_numpy(np.ascontiguousarray(st[k])).reshape(v.shape))

    def record(self, t):
        if self.t0 is None:
            self.t0 = self.bufs.t0 = t
        self.L.check(self.lib.emloco_recorder_record(C.byref(self.bufs), t, None), "emloco_recorder_record")

    def check(self, t):
        self.L.check(self.lib.emloco_recorder_check(C.byref(self.bufs), t, None), "emloco_recorder_check")

    def pull(self):
        torch.cuda.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        ok = all(bool((w[:GUARD] == FILL).all()) and bool((w[-GUARD:] == FILL).all()) for w in (self._ring_whole, self._slots_whole))
        return dict(ring=u32(self.ring).reshape(self.E, self.R, R.REC_WORDS), slots=u32(self.slots).reshape(self.C, -1),
                    counters=self.counters.cpu().numpy(), last=self.last.cpu().numpy(), guards=ok,
                    request=None if self.st["request"] is None else self.st["request"].cpu().numpy())

    def snapshot(self):
        """every buffer an entry point may write, guards included"""
        torch.cuda.synchronize()
        return [t.clone() for t in (self._ring_whole, self._slots_whole, self.counters, self.last, self.cause_ws, self.st["request"])]


make = DeviceBackend


# ---------------------------------------------------------------------------------------------------- the synthetic-buffer cases
@pytest.mark.parametrize("E", [5, 65])
def test_ring_wraps_and_stays_inside(E):
    cases.ring(make, E)


@pytest.mark.parametrize("mask", [31, 31 & ~(R.SPEED | R.EARLY_FALL), R.SPEED, 31 & ~R.REQUEST])
def test_causes(mask):
    cases.causes(make, mask)


def test_claim_does_not_depend_on_the_grid():
    got = [cases.claim(make, grid) for grid in (0, 3)]
    assert all((got[1][k] == got[0][k]).all() for k in ("ring", "slots", "counters", "last", "request"))


def test_suppression_and_slot_content():
    cases.suppression(make)


REFUSALS = [("n_env", 0, "n_env"), ("depth", 0, "depth"), ("n_slots", 0, "n_slots"), ("speed2_limit", -1.0, "speed2_limit"),
            ("speed2_limit", float("nan"), "speed2_limit"), ("ang_speed2_limit", -0.5, "ang_speed2_limit"),
            ("ang_speed2_limit", float("nan"), "ang_speed2_limit")]
REFUSALS += [(f, None, f) for f in ("root_state", "dof_state", "warm_start", "drive", "rb_state", "contact_force", "dof_force", "progress_buf",
                                    "reset_buf", "terminate_buf", "ring", "slots", "counters", "last_capture_step", "cause_ws")]


def test_refusals_name_the_argument_and_write_nothing():
    from emloco_amd import _lib as L
    b = make(6, 2, 3, cause_mask=31, speed2=1.0, ang2=1.0, early_fall=5)
    st = R.quiet_state(6)
    st["rb"][2, 1, 7] = 9.0                               # (a state that would capture, were a call to go through)
    st["request"][4] = 1
    b.push(st)
    before = b.snapshot()
    lib = L.load()
    for entry in (lib.emloco_recorder_record, lib.emloco_recorder_check):
        assert entry(None, 0, None) == -1 and b"null structure" in lib.emloco_last_error()
        for field, bad, word in REFUSALS:
            bufs = L.RecorderBufs.from_buffer_copy(b.bufs)
            setattr(bufs, field, bad)
            assert entry(C.byref(bufs), 0, None) == -1, field
            assert word.encode() in lib.emloco_last_error() and entry.__name__.encode() in lib.emloco_last_error(), (field, lib.emloco_last_error())
        with pytest.raises(L.EmlocoError, match="n_env"):
            bufs = L.RecorderBufs.from_buffer_copy(b.bufs)
            bufs.n_env = -3
            L.check(entry(C.byref(bufs), 0, None), entry.__name__)
    for was, now in zip(before, b.snapshot()):
        assert torch.equal(was, now)
    b.record(0)                                           # and the untouched structure does go through
    b.check(0)
    assert cases.captures(b.pull()) == [(2, 0, R.SPEED), (4, 0, R.REQUEST)]


def test_a_task_with_overlap_reset_is_refused_by_name():
    import types
    from emloco_amd.learning.flight_recorder import FlightRecorder
    with pytest.raises(RuntimeError, match="overlap_reset"):
        FlightRecorder(types.SimpleNamespace(overlap_reset=True, device="cuda:0", num_envs=4))


# ---------------------------------------------------------------------------------------------------- 7. NativeSim runs
@pytest.mark.parametrize("ground", [None, "slope_x_risers"])
def test_whole_chain_on_the_simulator(ground, tmp_path):
    """E = 8 on flat ground, the four humanoids of hf_scene on the riser field; 20 control steps, self-collision on, depth 4, the
    speed cause with a limit between two envs' peak speeds of the oracle's own run, one request at a fixed step"""
    from emloco_amd import _lib as L
    from emloco_amd.learning import flight_recorder as FR
    from emloco_amd.sim import NativeSim
    sc = cases.chain_scene(8, 20, ground)
    sim = NativeSim(sc["models"], L.default_sim_params(**cases.SIM_PARAMS), self_collision=sc["sc"], heightfield=sc["hf"])
    dev = sim.device
    sim.root_state.copy_(torch.from_numpy(sc["root"]).to(dev))
    sim.dof_state.copy_(torch.from_numpy(sc["dof"]).to(dev).reshape(sim.dof_state.shape))
    sim.refresh_bodies()
    sim.set_pd_targets(torch.from_numpy(sc["tgt"]).to(dev).contiguous())
    view = FR.sim_view(sim, heightfield=sc["hf"])
    rec = FR.FlightRecorder(view, depth=cases.CHAIN_DEPTH, slots=cases.CHAIN_SLOTS, speed=1.0)
    rec.speed2_limit = sc["limit2"]                       # the squared limit itself, as the oracle's run chose it
    for t in range(sc["steps"]):
        view.progress_buf.fill_(t)
        rec.record()
        sim.step(1)
        if t == sc["request"][1]:
            rec.request([sc["request"][0]])
        rec.check()
    captured, missed = rec.drain()
    assert not any(missed.values()) and int(rec.counters.sum()) == 0
    path = str(tmp_path / "run.npz")
    rec.save(path, captured, missed)
    back = cases.chain_verify(sc, captured, FR.load(path), tmp_path)
    assert ("ground/samples" in back) == (ground is not None) and ("ground/move_x" in back) == (ground is not None)
    assert rec.drain()[0].shape[0] == 0                   # drained: the next epoch starts with every slot free
    sim.close()


# ---------------------------------------------------------------------------------------------------- 8. a task run
TASK_E, TASK_STEPS, TASK_DEPTH, TASK_SLOTS = 16, 30, 6, 64
TASK_EARLY_FALL = 10                 # with these actions every env falls within 16 steps: the falls before progress 10 are captured, the later
                                     # ones are not -- and the request of step 19 then finds their resets inside its window of 6 records
TASK_REQUESTS = {9: (0, 5, 11), 19: tuple(range(TASK_E)), 29: tuple(range(TASK_E))}      # step -> envs asked for
ENV_FLAGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel", "--input_init_pose", "--input_init_vel"]
STATE = ("root_state", "dof_state", "warm_start", "pd_target", "rigid_body_state", "contact_force", "dof_force")


def _task_run(recorder_on):
    from emloco_amd.learning import flight_recorder as FR
    from test_gpu_env import _make_env
    env = _make_env(TASK_E, ENV_FLAGS)
    task, n = env.task, env.task.sim.native
    dev = task.device
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    actions = torch.randn(TASK_STEPS, TASK_E, 69, device=dev, generator=g) * 0.5
    out = dict(env=env, pre=[], post=[])
    host = lambda t: t.detach().cpu().numpy().copy()

    def state(request):
        return dict(root=host(n.root_state), dof=host(n.dof_state).reshape(TASK_E, 69, 2), warm=host(n.warm_start), drive=host(n.pd_target),
                    rb=host(n.rigid_body_state).reshape(TASK_E, 24, 13), cf=host(n.contact_force).reshape(TASK_E, 24, 3),
                    df=host(n.dof_force).reshape(TASK_E, 69), progress=host(task.progress_buf), reset=host(task.reset_buf),
                    terminate=host(task._terminate_buf), request=request)
    rec = None
    if recorder_on:
        rec = out["rec"] = FR.FlightRecorder(task, depth=TASK_DEPTH, slots=TASK_SLOTS, early_fall=TASK_EARLY_FALL).bind()
    else:
        task.before_physics_launch = lambda: out["pre"].append(state(None))       # the test's hook: the step's inputs, read on the host
    env.reset(torch.arange(TASK_E, device=dev))
    for t in range(TASK_STEPS):
        if t:
            env.reset_done() if hasattr(env, "reset_done") else env.reset(task.reset_buf.nonzero(as_tuple=False).flatten())
        obs, rew, dones, _ = env.step(actions[t])
        req = np.zeros(TASK_E, np.uint8)
        req[list(TASK_REQUESTS.get(t, ()))] = 1
        if rec is not None:
            if t in TASK_REQUESTS:
                rec.request(list(TASK_REQUESTS[t]))
            rec.check()
        else:
            out["post"].append(state(req))
    torch.cuda.synchronize()
    out.update(obs=obs.clone(), rew=rew.clone(), dones=dones.clone(), state=[getattr(n, k).clone() for k in STATE],
               flags=[task.progress_buf.clone(), task.reset_buf.clone(), task._terminate_buf.clone()])
    task.before_physics_launch = None
    return out


def test_task_run_is_unchanged_and_its_captures_replay(tmp_path):
    """16 envs, 30 steps of seeded random actions, the early-fall and request causes: the run with the recorder is the run without it
    bit for bit; its captures are the ones the numpy restatement takes from the states of the run WITHOUT it (no oracle in that
    bookkeeping), and every one replays clean -- among them one that spans a reset, where the replay does not compare"""
    from emloco_amd.learning import flight_recorder as FR
    on, off = _task_run(True), _task_run(False)
    assert torch.equal(on["obs"], off["obs"]) and torch.equal(on["rew"], off["rew"]) and torch.equal(on["dones"], off["dones"])
    for a, b, name in zip(on["state"] + on["flags"], off["state"] + off["flags"], STATE + ("progress", "reset", "terminate")):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), name
    # the reference bookkeeping on the states of the run without the recorder
    ref = R.RefRecorder(TASK_E, TASK_DEPTH, TASK_SLOTS, cause_mask=R.NONFINITE | R.EARLY_FALL | R.REQUEST, early_fall=TASK_EARLY_FALL)
    assert len(off["pre"]) == len(off["post"]) == TASK_STEPS
    for t in range(TASK_STEPS):
        ref.record(off["pre"][t], t)
        ref.check(off["post"][t], t)
    falls = [c for c in ref.log if c[2] & R.EARLY_FALL]
    spans = []
    for k in range(len(ref.log)):
        prog = [r["progress"] for r in FR.parse_slot(ref.slots[k], TASK_DEPTH)["records"]]
        spans.append(any(b != a + 1 for a, b in zip(prog, prog[1:])))
    print("\n  captures:", ref.log, "\n  spans a reset:", spans)
    assert falls and any(c[2] & R.REQUEST for c in ref.log) and any(spans) and ref.counters[1:].sum() == 0       # not vacuous
    rec = on["rec"]
    captured, missed = rec.drain()
    assert not any(missed.values())
    assert [(int(s[0]), int(s[1]), int(s[2])) for s in captured] == ref.log
    assert (captured == ref.slots[:len(ref.log)]).all()
    path = str(tmp_path / "task.npz")
    rec.save(path, captured, missed)
    tool = cases._tool()
    skipped = 0
    for k in range(len(ref.log)):
        rep = tool.replay(path, k)
        assert rep["matched"], tool.describe(rep)
        skipped += sum(s["against"] is None for s in rep["steps"])
        assert any(s["against"] is None for s in rep["steps"]) == spans[k]
    assert skipped > 0


# ---------------------------------------------------------------------------------------------------- inside the rollout loop
def _loop(E, overlap_reset=False, horizon=16, before=None):
    """env, task and LocoValRollout; `before(task)` runs once the env stands and ahead of the loop's constructor"""
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    from emloco_amd.run import RLGPUEnv
    from test_gpu_env import _make_env
    env = RLGPUEnv(_make_env(E, ENV_FLAGS))
    task = env.env.task
    if before is not None:
        before(task)
    g = torch.Generator(device=task.device)
    g.manual_seed(77)
    pool = torch.randn(8, E, 69, device=task.device, generator=g) * 0.3
    k = [0]

    def pol(obs):
        k[0] += 1
        return pool[k[0] % 8]
    pol.reads_obs = not overlap_reset
    torch.manual_seed(5)
    return env, task, LocoValRollout(env, horizon_length=horizon, policy=pol, overlap_reset=overlap_reset, warmup_epochs=5, max_epochs=40)


def test_a_loop_that_switches_overlap_reset_on_is_refused_where_the_recorder_is_attached():
    """the flag is a loop's to set, after a recorder may have been built: attaching, binding, recording and the driver's make_capture
    all look at it again"""
    from emloco_amd.learning.flight_recorder import FlightRecorder
    from emloco_amd.run import make_capture
    made = []
    # the recorder is built ahead of the loop, the flag still off: accepted there
    _, task, agent = _loop(16, overlap_reset=True, before=lambda task: made.append(FlightRecorder(task, depth=2, slots=2)))
    rec = made[0]
    assert task.overlap_reset and rec.task is task
    with pytest.raises(RuntimeError, match="overlap_reset"):
        agent.attach_flight_recorder(rec)
    assert agent.flight_recorder is None and getattr(task, "before_physics_launch", None) is None
    for call in (rec.bind, rec.record):
        with pytest.raises(RuntimeError, match="overlap_reset"):
            call()
    with pytest.raises(SystemExit, match="overlap_reset"):
        make_capture(task, dict(path="unused.npz", depth=2, slots=2, speed=None, ang_speed=None, early_fall=None))
    agent.detach()
    task.overlap_reset = False


LOOP_E, LOOP_EPOCHS, LOOP_PER_FILE = 64, 2, 2            # (two captures a file: the three requests alone fill more than one)


def _loop_run(tmp_path, capture_on):
    from emloco_amd.learning import flight_recorder as FR
    from emloco_amd.run import LocoValTrainee
    env, task, agent = _loop(LOOP_E)
    assert task.fused_chain and task.overlap_obs and not task.overlap_reset      # the headline arrangement: what this test is about
    log = None
    if capture_on:
        rec = FR.FlightRecorder(task, depth=6, slots=16, early_fall=20)
        log = FR.CaptureLog(rec, str(tmp_path / "loop.npz"), per_file=LOOP_PER_FILE)
    trainee = LocoValTrainee(agent, 1, 0, None, log)
    infos = []
    for epoch in range(LOOP_EPOCHS):
        if log is not None and epoch == 1:
            log.recorder.request([1, 5, 9])               # served at the epoch's first check
        infos.append(trainee.run_epoch())
    agent._sync_fit()
    torch.cuda.synchronize()
    n = task.sim.native
    out = dict(infos=infos, log=log, params=torch.cat([p.detach().reshape(-1) for p in agent.valuenet.parameters()]).clone(),
               state=[getattr(n, k).clone() for k in STATE] + [task.progress_buf.clone(), task.reset_buf.clone(), task.obs_buf.clone()])
    if log is not None:
        agent.attach_flight_recorder(None)
        assert getattr(task, "before_physics_launch", None) is None
    agent.detach()
    return out


def test_rollout_loop_with_the_chain_fused_records_and_replays(tmp_path):
    """LocoValRollout under the driver's trainee with fused_chain and overlap_obs on, 64 envs, two epochs of 16 steps: the loop's
    network and the simulation end bit for bit where they end without the recorder, the epoch's dict carries the counts, the files
    hold at most `per_file` captures each, and every capture replays clean on the oracle"""
    from emloco_amd.learning import flight_recorder as FR
    on, off = _loop_run(tmp_path, True), _loop_run(tmp_path, False)
    assert torch.equal(on["params"], off["params"])
    for a, b in zip(on["state"], off["state"]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert all("captures" not in i for i in off["infos"])
    log = on["log"]
    taken = [i["captures"] for i in on["infos"]]
    print("\n  captures per epoch:", taken, [i["captures_missed"] for i in on["infos"]], log.paths)
    assert all(set(i["captures_missed"]) == set(FR.CAUSES) for i in on["infos"])
    assert sum(taken) == log.total >= 3 and taken[1] >= 3                     # at the least the three requests
    assert len(log.paths) == -(-log.total // LOOP_PER_FILE)
    tool, seen, requested = cases._tool(), 0, set()
    for path in log.paths:
        d = FR.load(path)
        n = d["captures"].shape[0]
        assert 1 <= n <= LOOP_PER_FILE and int(d["substeps"]) == int(d["params/n_sub"]) * int(d["n_calls"])
        seen += n
        for k in range(n):
            rep = tool.replay(d, k)
            assert rep["matched"] and rep["compared"] >= 1, tool.describe(rep)
            if rep["cause"] & R.REQUEST:
                requested.add(rep["env"])
    assert seen == log.total and requested == {1, 5, 9}

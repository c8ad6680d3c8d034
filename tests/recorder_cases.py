"""The flight recorder's case tables -- TEST INFRASTRUCTURE ONLY.  tests/test_emu_recorder.py runs them on the CPU emulator,
tests/test_gpu_recorder.py on the device; the two differ only in the `make(E, R, C, **config)` they hand in, which returns a backend
with push(state) / record(t) / check(t) / pull() / drain() (tests/emu_recorder.py: EmuBackend).  Every comparison is `==` on raw
words against the numpy restatement (tests/flight_recorder_ref.py) and, where the case states them, against values written out here."""
import numpy as np

import flight_recorder_ref as R


def same(dev, ref):
    """the backend's buffers against the reference's, word for word"""
    assert dev["guards"], "a write outside the ring or the slots"
    assert (dev["ring"] == ref.ring).all()
    assert (dev["counters"] == ref.counters).all(), (dev["counters"], ref.counters)
    assert (dev["last"] == ref.last).all()
    k = int(ref.counters[0])
    assert (dev["slots"][:k] == ref.slots[:k]).all()
    assert (dev["slots"][k:] == 0).all()          # (no case here drains and goes on: the slots behind the used ones were never written)


def captures(dev):
    return [(int(s[0]), int(s[1]), int(s[2])) for s in dev["slots"][:int(dev["counters"][0])]]


def step(b, ref, st, t, check=True):
    """one control step on the backend and on the reference, from the same state"""
    ref_st = {k: (None if v is None else v.copy()) for k, v in st.items()}
    b.push(st)
    b.record(t)
    ref.record(ref_st, t)
    if check:
        b.check(t)
        ref.check(ref_st, t)
    return ref_st


# ---------------------------------------------------------------------------------------------------- 1. the ring
def ring(make, E):
    Rr, steps = 3, 7
    b = make(E, Rr, 2, cause_mask=0, drive_mode=1)
    ref = R.RefRecorder(E, Rr, 2, cause_mask=0, drive_mode=1)
    states = [R.synthetic_state(E, seed=t) for t in range(steps)]
    for t, st in enumerate(states):
        step(b, ref, st, t, check=False)
        d = b.pull()
        same(d, ref)
        for back in range(min(t + 1, Rr)):                       # the rows of the last R steps, written out: header and payload
            u, s = t - back, states[t - back]
            row = d["ring"][:, u % Rr]
            assert (row[:, 0] == s["progress"].astype(np.uint32)).all() and (row[:, 1] == u).all()
            assert (row[:, 2] == 1).all() and (row[:, 3] == 0).all()
            assert (row[:, 4:17] == R.bits(s["root"])).all() and (row[:, 17:155] == R.bits(s["dof"]).reshape(E, -1)).all()
            assert (row[:, 155:443] == R.bits(s["warm"])).all() and (row[:, 443:] == R.bits(s["drive"])).all()
    assert np.unique(d["ring"][:, :, 4:]).size == E * Rr * 508     # every payload word distinct: no copy landed twice


# ---------------------------------------------------------------------------------------------------- 2. the causes
SPEED2, ANG2, EARLY = 9.0, 2.25, 10


def cause_state():
    E = 12
    st = R.quiet_state(E)
    rb = st["rb"]
    rb[0, 5, 10:13] = (1.5, 0.0, 0.0)                  # |w|^2 exactly at the limit: no cause
    rb[1, 3, 2] = np.nan
    rb[2, 0, 5] = np.inf
    rb[3, 23, 0] = -np.inf
    rb[4, 7, 7:10] = (3.0, 0.0, 0.0)                   # |v|^2 exactly at the limit: no cause
    rb[5, 7, 7:10] = (3.0, 2.0 ** -10, 0.0)            # 9 + 2^-20: the next float up
    rb[6, 2, 8] = np.nan                               # a NaN velocity: non-finite, not fast
    rb[11, 9, 10:13] = (1.5, 2.0 ** -11, 0.0)          # 2.25 + 2^-22: the next float up
    assert np.float32(9.0) + np.float32(2.0 ** -20) == np.nextafter(np.float32(9.0), np.float32(np.inf))
    assert np.float32(2.25) + np.float32(2.0 ** -22) == np.nextafter(np.float32(2.25), np.float32(np.inf))
    st["progress"][:] = 50
    st["progress"][7], st["terminate"][7] = EARLY, 1           # at the limit: no cause
    st["progress"][8], st["terminate"][8] = EARLY - 1, 1
    st["progress"][9] = 3                                      # early but not terminated
    st["request"][10] = 1
    return st


CAUSE_EXPECTED = {1: R.NONFINITE, 2: R.NONFINITE, 3: R.NONFINITE, 5: R.SPEED, 6: R.NONFINITE, 8: R.EARLY_FALL, 10: R.REQUEST, 11: R.ANG_SPEED}


def causes(make, cause_mask=31):
    st = cause_state()
    E = st["progress"].shape[0]
    cfg = dict(cause_mask=cause_mask, speed2=SPEED2, ang2=ANG2, early_fall=EARLY)
    b, ref = make(E, 2, 16, **cfg), R.RefRecorder(E, 2, 16, **cfg)
    step(b, ref, st, 0)
    d = b.pull()
    same(d, ref)
    assert captures(d) == [(e, 0, c & cause_mask) for e, c in sorted(CAUSE_EXPECTED.items()) if c & cause_mask]
    assert (d["counters"][1:] == 0).all()
    served = bool(cause_mask & R.REQUEST)
    assert d["request"][10] == (0 if served else 1) and d["request"].sum() == (0 if served else 1)     # cleared once it is served


# ---------------------------------------------------------------------------------------------------- 3. the claim
CLAIM_ENVS = (2, 9, 17, 33, 40, 41, 63, 64, 69)


def claim_state(E, envs, seed):
    """`envs` trigger: the even ones are fast, the odd ones carry a request, 64 both"""
    st = R.quiet_state(E, seed)
    for e in envs:
        if e % 2 == 0:
            st["rb"][e, e % 24, 7] = 5.0
        if e % 2 == 1 or e == 64:
            st["request"][e] = 1
    return st


def claim(make, grid):
    E, Rr = 70, 2
    cfg = dict(cause_mask=R.SPEED | R.REQUEST, speed2=SPEED2, grid=grid)
    # C = 5: the five lowest get slots 0..4, the rest are counted per cause; with no slot left a further step only counts
    b, ref = make(E, Rr, 5, **cfg), R.RefRecorder(E, Rr, 5, cause_mask=cfg["cause_mask"], speed2=SPEED2)
    step(b, ref, claim_state(E, CLAIM_ENVS, 0), 0)
    d = b.pull()
    same(d, ref)
    assert [c[0] for c in captures(d)] == [2, 9, 17, 33, 40]
    assert list(d["counters"]) == [5, 0, 1, 0, 0, 4, 0, 0]            # missed: 41 (request) 63 (request) 64 (both) 69 (request)
    assert list(np.nonzero(d["request"])[0]) == [41, 63, 64, 69]      # an unserved request stays
    step(b, ref, claim_state(E, (5, 6), 1), 1)
    d = b.pull()
    same(d, ref)
    assert list(d["counters"]) == [5, 0, 2, 0, 0, 5, 0, 0]            # 6 fast, 5 asked for: no slot
    # C = 12: a second step continues with the slots the first left free
    b, ref = make(E, Rr, 12, **cfg), R.RefRecorder(E, Rr, 12, cause_mask=cfg["cause_mask"], speed2=SPEED2)
    step(b, ref, claim_state(E, CLAIM_ENVS, 0), 0)
    step(b, ref, claim_state(E, (68, 3, 50, 21, 10), 1), 1)
    d = b.pull()
    same(d, ref)
    assert captures(d)[9:] == [(3, 1, R.REQUEST), (10, 1, R.SPEED), (21, 1, R.REQUEST)]
    assert list(d["counters"]) == [12, 0, 2, 0, 0, 0, 0, 0]           # 50 and 68: fast, no slot
    return d


# ---------------------------------------------------------------------------------------------------- 4, 5. suppression, slot content
def suppression(make):
    E, Rr, C = 6, 3, 8
    cfg = dict(cause_mask=R.SPEED | R.REQUEST, speed2=SPEED2)
    b, ref = make(E, Rr, C, **cfg), R.RefRecorder(E, Rr, C, **cfg)
    states = []
    for t in range(8):
        st = R.quiet_state(E, seed=t)
        st["rb"][2, 4, 9] = 4.0                         # env 2 is fast at every step
        if t in (1, 2, 4):
            st["request"][4] = 1                        # env 4: asked for at 1 (served), 2 (suppressed), 4 (served)
        states.append(st)
        after = step(b, ref, st, t)
        d = b.pull()
        same(d, ref)
        assert d["request"].sum() == 0 and after["request"].sum() == 0           # served or suppressed: cleared either way
    assert captures(d) == [(2, 0, R.SPEED), (4, 1, R.REQUEST), (2, 3, R.SPEED), (4, 4, R.REQUEST), (2, 6, R.SPEED)]
    # slot content, written out: the capture at t = 0 holds one record and zeros, the one at t = 6 the steps 4, 5, 6 in this order
    W = R.REC_WORDS
    s0, s6 = d["slots"][0], d["slots"][4]
    assert s0[3] == 1 and (s0[4:4 + W] == R.record_words(states[0], 2, 0)).all() and (s0[4 + W:4 + 3 * W] == 0).all()
    assert s6[3] == 3
    for j, u in enumerate((4, 5, 6)):
        assert (s6[4 + j * W:4 + (j + 1) * W] == R.record_words(states[u], 2, u)).all()
    assert (s6[4 + 3 * W:] == R.post_words(states[6], 2)).all()
    s1 = d["slots"][1]                                   # t = 1 < R: two records, the third zero
    assert s1[3] == 2 and [int(s1[4 + j * W + 1]) for j in range(3)] == [0, 1, 0] and (s1[4 + 2 * W:4 + 3 * W] == 0).all()


# ---------------------------------------------------------------------------------------------------- 7. the whole chain on the simulator
SIM_PARAMS = dict(n_sub=2, h=1.0 / 120.0)
CHAIN_DEPTH, CHAIN_SLOTS = 4, 16


def _tool():
    """tools/replay_capture.py as a module"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay_capture.py")
    spec = importlib.util.spec_from_file_location("replay_capture", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sim_state(s, t):
    """a recorder state dict over the arrays of an oracle.Sim-shaped holder; progress = t for every env, so that consecutive records
    continue one episode"""
    E = s.E
    return dict(root=s.root_state, dof=s.dof_state, warm=s.lambda_ws.reshape(E, -1), drive=s.pd_target, rb=s.rb_state, cf=s.contact_force,
                df=s.dof_force, progress=np.full(E, t, np.int64), reset=np.zeros(E, np.int64), terminate=np.zeros(E, np.int64),
                request=np.zeros(E, np.uint8))


def chain_scene(E, steps, ground=None, request_step=5):
    """The scene of the whole-chain case and what the ORACLE ALONE says about it: the speed limit between two envs' peak body speeds,
    the request, and the captures the numpy restatement takes from the oracle's states.  Nothing here touches the code under test."""
    import helpers
    import sim_abi_cases
    from emloco_amd.model import pack_models, pack_self_collision
    if ground is None:
        hf, (models, (root, dof, tgt)) = None, (helpers.varied_models(E), helpers.scene_state(E, 7, perturbed_from=0))
    else:
        hf = sim_abi_cases.offset_field(ground)
        models, root, dof, tgt = sim_abi_cases.hf_scene(hf)
        E = len(models)
    sc = pack_self_collision(models)
    o = helpers.oracle_sim(models, root, dof, tgt, self_collision=sc, heightfield=hf, **SIM_PARAMS)
    pre, post, peak = [], [], np.zeros(E, np.float32)
    copy = lambda st: {k: v.copy() for k, v in st.items()}
    for t in range(steps):
        pre.append(copy(sim_state(o, t)))
        o.step(1)
        post.append(copy(sim_state(o, t)))
        rb = o.rb_state
        assert np.isfinite(rb).all()
        v2 = (rb[:, :, 7] * rb[:, :, 7] + rb[:, :, 8] * rb[:, :, 8]) + rb[:, :, 9] * rb[:, :, 9]
        peak = np.maximum(peak, v2.max(axis=1))
    order = np.sort(peak)
    assert order[-3] < order[-2], "two envs share a peak speed: pick another seed"
    limit2 = float(np.float32(0.5) * (order[-3] + order[-2]))            # between the third-fastest env's peak and the second-fastest's
    fast, never = np.nonzero(peak > limit2)[0], np.nonzero(~(peak > limit2))[0]
    assert len(fast) >= 2 and len(never) >= 1                             # on the oracle's own run: the case cannot pass vacuously
    req_env = int(never[0])
    ref = R.RefRecorder(E, CHAIN_DEPTH, CHAIN_SLOTS, cause_mask=R.NONFINITE | R.SPEED | R.REQUEST, speed2=limit2)
    for t in range(steps):
        ref.record(pre[t], t)
        if t == request_step:
            post[t]["request"][req_env] = 1
        ref.check(post[t], t)
    envs = {c[0] for c in ref.log}
    assert set(fast) <= envs and req_env in envs and (req_env, request_step, R.REQUEST) in ref.log and ref.counters[1:].sum() == 0
    return dict(E=E, steps=steps, models=models, packed=pack_models(models), sc=sc, hf=hf, root=root, dof=dof, tgt=tgt, limit2=limit2,
                request=(req_env, request_step), ref=ref, params=o.params)


def chain_verify(scene, captured, file_dict, tmp_path):
    """`captured`: the slots the run under test drained; `file_dict`: its capture file.  The captured set against the oracle's
    prediction, the file's round trip, the replay of every capture."""
    from emloco_amd.learning import flight_recorder as FR
    ref = scene["ref"]
    assert [(int(s[0]), int(s[1]), int(s[2])) for s in captured] == ref.log
    assert (captured == ref.slots[:len(ref.log)]).all()        # the step under test matches the oracle bit for bit, so every word does
    path = str(tmp_path / "cap.npz")
    FR.write(path, file_dict)
    back = FR.load(path)
    assert sorted(back) == sorted(file_dict)
    for k, v in file_dict.items():
        assert back[k].dtype == np.asarray(v).dtype and (back[k] == np.asarray(v)).all(), k
    tool = _tool()
    for k in range(len(ref.log)):
        rep = tool.replay(back, k)
        assert rep["matched"] and rep["compared"] == rep["n_valid"] == min(ref.log[k][1] + 1, CHAIN_DEPTH), tool.describe(rep)
        assert (rep["env"], rep["t"], rep["cause"]) == ref.log[k]
    assert tool.main([path]) == 0
    return back

"""Device conformance matrix of the rigid-body step's C ABI (include/emloco_sim.h) against the CPU oracle and float64 contact counts.

Companion of tests/test_gpu_sim.py (scenarios: episodes of falling humanoids, all through n_sub = 2 x n_calls = 2, 2 or 4 parts, square
height fields at the world origin, indexed setters handed the simulator's own tensor).  This file walks the interface instead, through
`NativeSim` or its raw handle; the case tables are those of tests/sim_abi_cases.py, which tests/test_sim_abi_cpu.py runs through the
emulator on a CPU: the device run differs in the executor only, so a case that fails here and not there points at the hand-over or the
launch code.

Covered:
  1. split        every (n_sub, n_calls, n_parts) of SPLIT_CASES -- uneven and odd splits, substep totals 1 to 7, more parts than
                  substeps (clamped) -- every other case with the cost-ordered dispatch, two uneven cases also as skip flags + a
                  -1-padded id list (emloco_sim_step_subset)
  2. env counts   1, 2, 63, 64, 65 envs with 3 parts and cost order on (one env, both sides of a 64-lane wave)
  3. height field 90 x 41 samples starting at (48.3, 52.7), sloped along x / along y / with one-cell risers through
                  emloco_sim_set_ground_mesh_moves; humanoids inside the field, before its first row and behind its last one
  4. indexed setters from a foreign tensor (copy_rows_kernel, which no other test runs): the listed rows take the new values, their
                  body states are the oracle's forward kinematics, every other row of all seven tensors keeps its bits; -1-padded lists
                  and a 300-entry list (more entries than the forward-kinematics launch has workgroups; the one case above 65 envs:
                  a list may not be longer than n_env)
  5. emloco_sim_refresh_bodies after in-place edits of every env
  6. emloco_sim_set_params / get_params after prepare: n_sub and h take effect, drive_mode belongs to the last upload
  7. resume       the seven tensors copied into a freshly created simulator continue a rollout bit for bit, in position and in
                  effort mode (no hidden state besides them and the mode of the upload call)
  8. cost key     emloco_sim_cost_ticks equals 10 + the contacts kept (<= 20) of the float64 count at the state a step starts from,
                  in every contact regime of the `plane` and `hf` scenes of tests/contact_layout_cases.py and on the offset field
  9. refusals     every EMLOCO_E_STATE / EMLOCO_E_ARG return of the header that is decided before a launch: the code, a non-empty
                  emloco_last_error that names the call, and all seven tensors bit for bit as they were.  (Moves without a height
                  field are a call out of order: EMLOCO_E_STATE, as the header defines that code.)

Bars.  Every comparison with the oracle's step is bit equality on root_state, dof_state, rb_state, contact_force, dof_force and the
warm start.  Forward kinematics after a state write (4, 5): the bar of test_gpu_sim.test_fk_after_indexed_set_matches_oracle
(1e-5 relative + 2e-5) and, since the largest difference measured is zero, bit equality.  Cost key: exact on every env-step whose
float64 count is beyond doubt (no candidate within 1e-5 m of the contact offset); at most 10 % of the env-steps may be doubtful.

Measured (MI355X, the run that accompanied this file; every run prints the figures, `pytest -s`):

    largest |device - oracle| of the body states after indexed sets (4), all lists       0 (bit-exact)
    largest |device - oracle| of the body states after refresh_bodies (5)                0 (bit-exact)
    doubtful env-steps of the cost key (8): plane / hf / slope_x / slope_y               0 of 48 / 0 of 48 / 0 of 24 / 0 of 24
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_abi_cases as S                                                        # noqa: E402
from test_gpu_sim import _close                                                  # noqa: E402  (the forward-kinematics bar)

SEVEN = ("root_state", "dof_state", "rigid_body_state", "contact_force", "dof_force", "pd_target", "warm_start")
OK, E_ARG, E_STATE = 0, -1, -3


def _native(models, n_sub, **kw):
    from emloco_amd import _lib as L
    from emloco_amd.sim import NativeSim
    return NativeSim(models, L.default_sim_params(n_sub=n_sub), **kw)


def _load(gsim, root, dof, tgt):
    E = root.shape[0]
    gsim.root_state.copy_(torch.from_numpy(root))
    gsim.dof_state.view(E, 69, 2).copy_(torch.from_numpy(dof))
    gsim.pd_target.copy_(torch.from_numpy(tgt))


def _compare(osim, gsim, what):
    torch.cuda.synchronize()
    for name, a, b in (("root_state", gsim.root_state, osim.root_state), ("dof_state", gsim.dof_state, osim.dof_state),
                       ("rb_state", gsim.rigid_body_state, osim.rb_state), ("contact_force", gsim.contact_force, osim.contact_force),
                       ("dof_force", gsim.dof_force, osim.dof_force), ("lambda_ws", gsim.warm_start, osim.lambda_ws)):
        a = a.cpu().numpy().reshape(b.shape)
        assert np.array_equal(a, b), f"{what} {name}: not bit-exact, max abs diff {np.abs(a - b).max():.3e}"


def _snapshot(gsim):
    torch.cuda.synchronize()
    return {name: getattr(gsim, name).clone() for name in SEVEN}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _unchanged(gsim, snap, what, rows=None):
    """all seven tensors (or, with `rows` {name: bool mask over envs}, the masked env rows of them) equal their clones bit for bit"""
    torch.cuda.synchronize()
    E = gsim.num_envs
    for name in SEVEN:
        a, b = getattr(gsim, name).reshape(E, -1), snap[name].reshape(E, -1)
        if rows is not None:
            a, b = a[rows[name]], b[rows[name]]
        assert torch.equal(_bits(a), _bits(b)), f"{what}: {name} changed"


# ------------------------------------------------------------------------------------------------------------ 1. split
@pytest.mark.parametrize("case", range(len(S.SPLIT_CASES)), ids=["%d-%d-%d" % c for c in S.SPLIT_CASES])
def test_split_cases_are_bit_exact_vs_oracle(case):
    n_sub, n_calls, n_parts = S.SPLIT_CASES[case]
    E = S.SPLIT_ENVS_DEVICE
    models, root, dof, tgt = S.split_scene(E)
    osim = S.split_oracle(E, n_sub, n_calls)
    sims = [_native(models, n_sub, self_collision=True)]
    subset = (n_sub, n_calls, n_parts) in S.SPLIT_SUBSET_CASES
    if subset:
        sims.append(_native(models, n_sub, self_collision=True))
    for g in sims:
        _load(g, root, dof, tgt)
        g.set_split(n_parts)
        g.set_cost_order(case % 2 == 1)
    for t in range(S.SPLIT_STEPS):
        osim.step(1)
        sims[0].step(n_calls)
        _compare(osim, sims[0], f"{S.SPLIT_CASES[case]} step {t}")
        if subset:                     # the same step as two launches: everything but the flagged envs, then the flagged ones by list
            flagged = [e for e in range(E) if (e + t) % 2 == 1]
            skip = torch.zeros(E, dtype=torch.int64, device=sims[1].device)
            skip[flagged] = 1
            ids = torch.full((E,), -1, dtype=torch.int32, device=sims[1].device)
            ids[:len(flagged)] = torch.tensor(flagged, dtype=torch.int32)
            sims[1].step_subset(n_calls, skip=skip)
            sims[1].step_subset(n_calls, ids=ids)
            _compare(osim, sims[1], f"{S.SPLIT_CASES[case]} subset step {t}")
    assert np.abs(osim.contact_force).max() > 50.0


# ------------------------------------------------------------------------------------------------------------ 2. env counts
@pytest.mark.parametrize("E", S.ENV_COUNTS)
def test_env_counts_at_the_wave_and_sort_edges(E):
    models, root, dof, tgt = S.split_scene(E)
    osim = S.split_oracle(E, 2, 2)
    gsim = _native(models, 2, self_collision=True)
    _load(gsim, root, dof, tgt)
    gsim.set_split(3)
    gsim.set_cost_order(True)
    for t in range(2):
        osim.step(1)
        gsim.step(2)
        _compare(osim, gsim, f"{E} envs step {t}")
    assert np.abs(osim.contact_force).max() > 50.0


# ------------------------------------------------------------------------------------------------------------ 3. height field
@pytest.mark.parametrize("kind", S.HF_KINDS)
def test_offset_nonsquare_heightfield_is_bit_exact_vs_oracle(kind):
    osim, hf = S.hf_oracle(kind, 4)
    models, root, dof, tgt = S.hf_scene(hf)
    assert ("move_x" in hf) == kind.endswith("_risers")
    gsim = _native(models, 2, self_collision=True, heightfield=hf)
    _load(gsim, root, dof, tgt)
    gsim.set_split(4)
    for t in range(S.HF_STEPS):
        osim.step(1)
        gsim.step(2)
        _compare(osim, gsim, f"{kind} step {t}")
    assert np.abs(osim.contact_force).max() > 50.0


# ------------------------------------------------------------------------------------------------------------ 4. indexed setters
def _fk_scene(E):
    from helpers import oracle_sim, scene_state, varied_models
    base = varied_models(min(E, 16), 61)
    models = [base[e % len(base)] for e in range(E)]
    root, dof, tgt = scene_state(E, 62)
    new_root, new_dof, _ = scene_state(E, 63, height=1.1, perturbed_from=0)
    new_root[:, 1] += 1.5
    gsim = _native(models, 2)
    _load(gsim, root, dof, tgt)
    gsim.refresh_bodies()
    gsim.step(1)                       # forces, warm start and body states of a real step in all seven tensors
    osim = oracle_sim(models, root, dof, tgt)
    return gsim, osim, new_root, new_dof


@pytest.mark.parametrize("case", range(6), ids=[c[0] for c in S.id_lists()])
def test_indexed_setters_from_a_foreign_tensor(case):
    name, ids, E = S.id_lists()[case]
    gsim, osim, new_root, new_dof = _fk_scene(E)
    snap = _snapshot(gsim)
    full_root = torch.from_numpy(new_root).to(gsim.device)
    full_dof = torch.from_numpy(new_dof.reshape(E * 69, 2)).to(gsim.device)
    assert full_root.data_ptr() != gsim.root_state.data_ptr() and full_dof.data_ptr() != gsim.dof_state.data_ptr()
    dev_ids = torch.from_numpy(ids).to(gsim.device)
    gsim.set_root_state_indexed(full_root, dev_ids)
    gsim.set_dof_state_indexed(full_dof, dev_ids)
    gsim.sync()
    listed = np.zeros(E, bool)
    listed[ids[ids >= 0]] = True
    lt = torch.from_numpy(listed).to(gsim.device)
    written = {n: lt if n in ("root_state", "dof_state", "rigid_body_state") else torch.zeros_like(lt) for n in SEVEN}
    _unchanged(gsim, snap, name, rows={n: ~m for n, m in written.items()})
    assert torch.equal(_bits(gsim.root_state[lt]), _bits(full_root[lt])), f"{name}: listed root rows"
    assert torch.equal(_bits(gsim.dof_state.view(E, -1)[lt]), _bits(full_dof.view(E, -1)[lt])), f"{name}: listed dof rows"
    if listed.any():
        osim.root_state[listed] = new_root[listed]
        osim.dof_state[listed] = new_dof[listed]
        osim.fk()
        rb = gsim.rigid_body_state.view(E, 24, 13).cpu().numpy()
        diff = float(np.abs(rb[listed].astype(np.float64) - osim.rb_state[listed]).max())
        print(f"indexed set `{name}`: largest |device - oracle| of the listed body states {diff:.3e}")
        _close(rb[listed], osim.rb_state[listed], 1e-5, what=f"fk {name}")
        assert np.array_equal(rb[listed], osim.rb_state[listed]), f"{name}: body states not bit-exact, max abs diff {diff:.3e}"


# ------------------------------------------------------------------------------------------------------------ 5. refresh_bodies
def test_refresh_bodies_recomputes_every_env_and_nothing_else():
    E = 7
    gsim, osim, new_root, new_dof = _fk_scene(E)
    gsim.root_state.copy_(torch.from_numpy(new_root))                       # in-place edits of the simulator's own tensors
    gsim.dof_state.view(E, 69, 2).copy_(torch.from_numpy(new_dof))
    snap = _snapshot(gsim)
    gsim.refresh_bodies()
    gsim.sync()
    keep = torch.ones(E, dtype=torch.bool, device=gsim.device)
    _unchanged(gsim, snap, "refresh_bodies", rows={n: keep if n != "rigid_body_state" else ~keep for n in SEVEN})
    osim.root_state[:] = new_root
    osim.dof_state[:] = new_dof
    osim.fk()
    rb = gsim.rigid_body_state.view(E, 24, 13).cpu().numpy()
    diff = float(np.abs(rb.astype(np.float64) - osim.rb_state).max())
    print(f"refresh_bodies: largest |device - oracle| of the body states {diff:.3e}")
    _close(rb, osim.rb_state, 1e-5, what="fk refresh")
    assert np.array_equal(rb, osim.rb_state), f"body states not bit-exact, max abs diff {diff:.3e}"


# ------------------------------------------------------------------------------------------------------------ 6. params
PARAM_FIELDS = ("n_sub", "n_iter", "h", "gravity_z", "contact_offset", "erp", "max_depen_vel", "mu", "ang_damping", "max_ang_vel",
                "ground_z", "cfm", "warm")


def test_set_params_after_prepare():
    from helpers import oracle_sim
    E = S.SPLIT_ENVS_DEVICE
    models, root, dof, tgt = S.split_scene(E)
    osim = oracle_sim(models, root, dof, tgt, self_collision=True, n_sub=4)
    gsim = _native(models, 2, self_collision=True)
    _load(gsim, root, dof, tgt)
    p = gsim.get_params()
    assert p.n_sub == 2 and p.drive_mode == 0
    p.n_sub = 1
    gsim.set_params(p)
    assert gsim.get_params().n_sub == 1
    for t in range(2):
        osim.step(1)
        gsim.step(4)                                           # 4 calls of 1 substep = the oracle's 4
        _compare(osim, gsim, f"n_sub = 1 step {t}")
    p.h = p.h / 2                                              # halve the substep mid-run on both sides
    p.n_iter = 3
    gsim.set_params(p)
    osim.params.h, osim.params.n_iter = p.h, p.n_iter
    q = gsim.get_params()
    for f in PARAM_FIELDS:
        assert getattr(q, f) == getattr(p, f), f
    for t in range(2):
        osim.step(1)
        gsim.step(4)
        _compare(osim, gsim, f"h / 2 step {t}")
    # once prepared the drive mode belongs to the last upload: a parameter update carrying drive_mode = 0 leaves effort drives live
    torque = (np.random.default_rng(9).normal(size=(E, 69)) * 120.0).astype(np.float32)
    gsim.set_dof_actuation_force(torch.from_numpy(torque).to(gsim.device))
    p.drive_mode = 0
    gsim.set_params(p)
    assert gsim.get_params().drive_mode == 1
    osim.params.drive_mode = 1
    osim.pd_target[:] = torque
    for t in range(2):
        osim.step(1)
        gsim.step(4)
        _compare(osim, gsim, f"effort step {t}")
    p.drive_mode = 1                                           # and the other way round: the upload of targets switches back
    gsim.set_pd_targets(torch.from_numpy(tgt).to(gsim.device))
    gsim.set_params(p)
    assert gsim.get_params().drive_mode == 0
    osim.params.drive_mode = 0
    osim.pd_target[:] = tgt
    osim.step(1)
    gsim.step(4)
    _compare(osim, gsim, "position step")
    assert np.abs(osim.contact_force).max() > 50.0


# ------------------------------------------------------------------------------------------------------------ 7. resume
@pytest.mark.parametrize("mode", ["position", "effort"])
def test_resume_from_the_seven_tensors_in_a_fresh_simulator(mode):
    import contact_layout_cases as K
    from emloco_amd.model import pack_self_collision
    E = K.E
    models, root, dof, tgt = K.scene("hf")                     # two standing, six lying on the bumpy slope: contacts at every step
    hf = K.heightfield()
    sc = pack_self_collision(models)
    rng = np.random.default_rng(11)
    scale = 0.3 if mode == "position" else 40.0
    cmds = [torch.from_numpy((rng.normal(size=(E, 69)) * scale).astype(np.float32)).cuda() for _ in range(10)]

    def run(g, ks):
        for k in ks:
            (g.set_pd_targets if mode == "position" else g.set_dof_actuation_force)(cmds[k])
            g.step(2)
        g.sync()

    a = _native(models, 2, self_collision=sc, heightfield=hf)
    _load(a, root, dof, tgt)
    run(a, range(5))
    snap = _snapshot(a)
    assert float(snap["warm_start"].abs().max()) > 0.0 and float(snap["contact_force"].abs().max()) > 50.0
    run(a, range(5, 10))
    b = _native(models, 2, self_collision=sc, heightfield=hf)          # fresh: its drive mode comes from the upload call in run()
    for name in SEVEN:
        getattr(b, name).copy_(snap[name])
    run(b, range(5, 10))
    for name in SEVEN:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), f"{mode}: {name} differs after the resume"
    assert not torch.equal(a.root_state, snap["root_state"])


# ------------------------------------------------------------------------------------------------------------ 8. cost key
@pytest.mark.parametrize("scene", S.KEY_SCENES)
def test_cost_key_is_the_float64_contact_count(scene):
    import contact_layout_cases as K
    osim, hf = S.key_oracle(scene)
    if scene in ("plane", "hf"):
        models, root, dof, tgt = K.scene(scene)
    else:
        models, root, dof, tgt = S.hf_scene(hf)
    E = osim.E
    gsim = _native(models, 1, self_collision=True, heightfield=hf)
    _load(gsim, root, dof, tgt)
    gsim.set_cost_order(True)
    osim.fk()                                                  # (before the first step rb_state is all zeros)
    chk = S.KeyCheck()
    keys = np.full(E, 0xFFFFFFFF, np.uint32)
    for t in range(S.KEY_STEPS):
        chk.before_step(osim, hf)
        osim.step(1)
        gsim.step(1)
        _compare(osim, gsim, f"{scene} step {t}")
        assert gsim.lib.emloco_sim_cost_ticks(gsim._h, keys.ctypes.data, None, E) == OK
        chk.after_step(keys, f"{scene} step {t}")
    print(f"cost key {scene}: {chk.doubtful} of {chk.doubtful + chk.compared} env-steps doubtful")
    assert chk.share_doubtful() <= S.KEY_MAX_DOUBTFUL
    if scene in ("plane", "hf"):
        chk.cov.check()
    else:
        assert 0 in chk.cov.counts and any(n > 0 for n in chk.cov.counts), sorted(set(chk.cov.counts))


# ------------------------------------------------------------------------------------------------------------ 9. refusals
def _refused(lib, rc, code, names):
    """the code, and a non-empty emloco_last_error that names the call"""
    assert rc == code, (rc, code, lib.emloco_last_error())
    msg = lib.emloco_last_error()
    assert msg and any(n.encode() in msg for n in names), (msg, names)


def test_calls_out_of_order_and_bad_heightfields_are_refused_before_prepare():
    from emloco_amd import _lib as L
    from emloco_amd.model import pack_models
    lib = L.require_device()
    E = 2
    models, root, dof, tgt = S.split_scene(E)
    p = {k: np.ascontiguousarray(v) for k, v in pack_models(models).items()}
    f = lambda a: a.ctypes.data
    desc = L.ModelDesc(E, *[C.cast(f(p[k]), C.POINTER(C.c_int32 if k in ("parent", "geom_type") else C.c_float)) for k in
                            ("parent", "geom_type", "joint_off", "mass", "com", "inertia", "geom_a", "geom_b", "geom_r", "kp", "kd",
                             "armature", "effort")])
    params = L.default_sim_params()
    h = C.c_void_p()
    assert lib.emloco_sim_create(C.byref(params), 0, C.byref(h)) == OK
    try:
        some = torch.zeros(E, 69, device="cuda")
        ptr, shape = C.c_void_p(), (C.c_int64 * 2)()
        for stage in ("created", "models set"):
            _refused(lib, lib.emloco_sim_step(h, 1, None), E_STATE, ["emloco_sim_step"])
            _refused(lib, lib.emloco_sim_tensor(h, L.T_ROOT_STATE, C.byref(ptr), shape), E_STATE, ["emloco_sim_tensor"])
            assert ptr.value is None
            _refused(lib, lib.emloco_sim_set_split(h, 2), E_STATE, ["emloco_sim_set_split"])
            _refused(lib, lib.emloco_sim_set_cost_order(h, 1), E_STATE, ["emloco_sim_set_cost_order"])
            _refused(lib, lib.emloco_sim_set_pd_targets(h, some.data_ptr(), None), E_STATE, ["emloco_sim_set_pd_targets"])
            if stage == "created":
                assert lib.emloco_sim_set_models(h, C.byref(desc)) == OK
        hfn = ["emloco_sim_set_ground_heightfield"]
        mvn = ["emloco_sim_set_ground_mesh_moves"]
        smp = np.zeros((4, 5), np.int16)
        mv0, mv2 = np.zeros((4, 5), np.int8), np.zeros((4, 5), np.int8)
        mv2[1, 2], mv0[2, 2] = 2, 1
        _refused(lib, lib.emloco_sim_set_ground_heightfield(h, f(smp), 1, 5, 0.1, 0.005, 0.0, 0.0), E_ARG, hfn)
        _refused(lib, lib.emloco_sim_set_ground_heightfield(h, f(smp), 4, 1, 0.1, 0.005, 0.0, 0.0), E_ARG, hfn)
        _refused(lib, lib.emloco_sim_set_ground_heightfield(h, f(smp), 4, 5, 0.0, 0.005, 0.0, 0.0), E_ARG, hfn)
        _refused(lib, lib.emloco_sim_set_ground_heightfield(h, f(smp), 4, 5, 0.1, 0.0, 0.0, 0.0), E_ARG, hfn)
        _refused(lib, lib.emloco_sim_set_ground_mesh_moves(h, f(mv0), f(mv0)), E_STATE, mvn)       # moves without a field: out of order
        assert lib.emloco_sim_set_ground_heightfield(h, f(smp), 4, 5, 0.1, 0.005, 0.0, 0.0) == OK
        _refused(lib, lib.emloco_sim_set_ground_mesh_moves(h, f(mv2), f(mv0)), E_ARG, mvn)         # a move of 2 cells
        _refused(lib, lib.emloco_sim_set_ground_mesh_moves(h, f(mv0), f(-mv2)), E_ARG, mvn)        # a move of -2 cells
        _refused(lib, lib.emloco_sim_set_ground_mesh_moves(h, f(mv0), None), E_ARG, mvn)           # only one move array
        _refused(lib, lib.emloco_sim_set_ground_mesh_moves(h, None, f(mv0)), E_ARG, mvn)
        assert lib.emloco_sim_set_ground_mesh_moves(h, f(mv0), f(mv0)) == OK
        assert lib.emloco_sim_prepare(h) == OK
    finally:
        lib.emloco_sim_destroy(h)


def test_refused_calls_on_a_prepared_sim_write_nothing():
    from emloco_amd import _lib as L
    E = S.SPLIT_ENVS_DEVICE
    models, root, dof, tgt = S.split_scene(E)
    osim = S.split_oracle(E, 2, 2)
    gsim = _native(models, 2, self_collision=True)
    _load(gsim, root, dof, tgt)
    gsim.set_split(2)
    osim.step(1)
    gsim.step(2)
    _compare(osim, gsim, "before the refusals")
    lib, h, dev = gsim.lib, gsim._h, gsim.device
    snap = _snapshot(gsim)
    p0 = gsim.get_params()
    other = torch.full((E + 1, 13 * 24), 3.5, device=dev)                     # a foreign tensor no refused call may read from
    ids_long = torch.full((E + 1,), -1, dtype=torch.int32, device=dev)
    ids = torch.tensor([1, 0, -1], dtype=torch.int32, device=dev)
    skip = torch.zeros(E, dtype=torch.int64, device=dev)
    st = gsim._stream()
    # out of order
    _refused(lib, lib.emloco_sim_set_models(h, C.byref(L.ModelDesc())), E_STATE, ["emloco_sim_set_models"])
    _refused(lib, lib.emloco_sim_set_self_collision(h, C.byref(L.SelfCollisionDesc())), E_STATE, ["emloco_sim_set_self_collision"])
    smp = np.zeros((4, 5), np.int16)
    _refused(lib, lib.emloco_sim_set_ground_heightfield(h, smp.ctypes.data, 4, 5, 0.1, 0.005, 0.0, 0.0), E_STATE, ["emloco_sim_set_ground_heightfield"])
    # bad arguments
    _refused(lib, lib.emloco_sim_step(h, 0, st), E_ARG, ["emloco_sim_step"])
    sub = ["emloco_sim_step_subset"]
    _refused(lib, lib.emloco_sim_step_subset(h, 2, skip.data_ptr(), ids.data_ptr(), 3, st), E_ARG, sub)        # both selectors
    _refused(lib, lib.emloco_sim_step_subset(h, 2, None, None, 0, st), E_ARG, sub)                             # neither
    _refused(lib, lib.emloco_sim_step_subset(h, 2, None, ids_long.data_ptr(), E + 1, st), E_ARG, sub)          # n_ids > n_env
    _refused(lib, lib.emloco_sim_step_subset(h, 2, None, ids.data_ptr(), -1, st), E_ARG, sub)
    _refused(lib, lib.emloco_sim_step_subset(h, 0, skip.data_ptr(), None, 0, st), E_ARG, sub)
    _refused(lib, lib.emloco_sim_set_split(h, 0), E_ARG, ["emloco_sim_set_split"])
    _refused(lib, lib.emloco_sim_set_split(h, 5), E_ARG, ["emloco_sim_set_split"])
    ptr, shape = C.c_void_p(), (C.c_int64 * 2)()
    for kind in (L.T_WARM_START + 1, -1):
        _refused(lib, lib.emloco_sim_tensor(h, kind, C.byref(ptr), shape), E_ARG, ["emloco_sim_tensor"])
        assert ptr.value is None
    for field, bad in (("n_sub", 0), ("h", 0.0), ("drive_mode", 2), ("drive_mode", -1), ("n_iter", -1)):
        q = gsim.get_params()
        setattr(q, field, bad)
        _refused(lib, lib.emloco_sim_set_params(h, C.byref(q)), E_ARG, ["emloco_sim_set_params"])
    q = gsim.get_params()
    for fld, _ in L.SimParams._fields_:
        assert getattr(q, fld) == getattr(p0, fld), fld
    for fn in (lib.emloco_sim_set_root_state_indexed, lib.emloco_sim_set_dof_state_indexed):
        _refused(lib, fn(h, other.data_ptr(), ids.data_ptr(), -1, st), E_ARG, ["indexed"])
        _refused(lib, fn(h, other.data_ptr(), ids_long.data_ptr(), E + 1, st), E_ARG, ["indexed"])
        _refused(lib, fn(h, None, ids.data_ptr(), 2, st), E_ARG, ["indexed"])
    # nothing to do: OK, and nothing written
    assert lib.emloco_sim_step_subset(h, 2, None, ids.data_ptr(), 0, st) == OK
    assert lib.emloco_sim_set_root_state_indexed(h, other.data_ptr(), ids.data_ptr(), 0, st) == OK
    assert lib.emloco_sim_set_dof_state_indexed(h, other.data_ptr(), ids.data_ptr(), 0, st) == OK
    gsim.sync()
    _unchanged(gsim, snap, "after the refused calls")
    # and the simulator goes on as if they had not been made (2 parts, 2 substeps a call, position drives)
    osim.step(1)
    gsim.step(2)
    _compare(osim, gsim, "after the refusals")

"""Scene table of the rigid-body step's branch-coverage test (tests/test_sim_branches_cpu.py: the kernel sources under gcov on the CPU
emulator) and of its device twin (tests/test_gpu_sim_branches.py).

Every comparison of the rigid-body step is bit equality with oracle/oracle_sim.c, which cannot be made stricter; what a set of scenes
can still miss is a PATH of the kernel.  The table therefore has two halves:

  EXISTING   the scenes the suite already runs on the emulator and on the device (tests/sim_abi_cases.py, contact_layout_cases.py,
             test_emu_sim_handover.py, the `_mk` and special scenes of test_gpu_sim.py restated from their seeds), with episodes cut
             to the few control steps the coverage run can afford (the emulator runs some 20 env-substeps a second)
  NEW        one scene per branch that none of those takes: each at most 8 envs and 4 control steps, deterministic from a seed,
             built on `helpers.varied_models`, and each with a `regime` assertion in float64 that the start state really lies where
             the branch is decided (joint angle beyond pi, spin above the limit, tie at the 20th contact, hit count, region ...)

A `Case` is data: `scene()` gives models / root / dof / targets / params / self-collision pack / height field, from which the CPU run
builds two oracle.Sim state holders (one stepped by the oracle, one by the emulated kernel) and the device run a NativeSim.
"""
import numpy as np

import contact_layout_cases as K
import sim_abi_cases as S
from helpers import bumpy_heightfield, corrected_stairs, oracle_sim, scene_state, varied_models

NAMES = K.NAMES
PI32 = np.float32(np.pi)


class Case:
    """name; scene() -> dict(models, root, dof, tgt[, sc, hf, params]); n_sub x n_calls substeps per control step (the oracle runs
    their product as one call); `parts`: split launch; `launch`: "plain" | "order" (cost-ordered dispatch, ticks read back) |
    "subset" (skip flags + -1-padded id list: two launches per step); `pre_step(t, sims)`: edits targets / params of every state
    holder before control step t; `regime(scene)`: the float64 assertion that the start state is in the branch's regime;
    `after(oracle)`: an assertion on the oracle's state after the last step (the executor under test is on the same bytes);
    `closes`: the source lines (stripped text) whose never-taken branch the scene takes."""

    def __init__(self, name, scene, steps, n_sub=2, n_calls=2, parts=1, launch="plain", pre_step=None, regime=None, after=None,
                 new=False, closes=()):
        self.name, self.scene, self.steps, self.n_sub, self.n_calls, self.parts = name, scene, steps, n_sub, n_calls, parts
        self.launch, self.pre_step, self.regime, self.after, self.new, self.closes = launch, pre_step, regime, after, new, tuple(closes)

    def oracle(self, sc=None):
        s = sc if sc is not None else self.scene()
        params = dict(s.get("params", {}))
        params["n_sub"] = self.n_sub * self.n_calls
        return oracle_sim(s["models"], s["root"], s["dof"], s["tgt"], self_collision=s.get("sc"), heightfield=s.get("hf"), **params)

    def cost(self, sc):
        return sc["root"].shape[0] * self.steps * self.n_sub * self.n_calls


def same(a, b, what):
    for name in NAMES:
        x, y = getattr(a, name), getattr(b, name)
        assert np.array_equal(x, y), f"{what} {name}: not bit-exact, max abs diff {np.abs(x - y).max():.3e}"


def run_emulated(case, emu, log=None):
    """The case through oracle and emulated kernel, bit equality on all six outputs after every control step.  Returns the oracle."""
    sc = case.scene()
    if case.regime is not None:
        case.regime(sc)
    a, b = case.oracle(sc), case.oracle(sc)
    b.params.n_sub = case.n_sub                                  # the emulator multiplies by n_calls itself, as the launcher does
    E = a.E
    keys = np.zeros(E, np.uint32)
    for t in range(case.steps):
        if case.pre_step is not None:
            case.pre_step(t, (a, b))
        a.step(1)
        if case.launch == "subset":                              # everything but the flagged envs, then the flagged ones by list
            flagged = [e for e in range(E) if (e + t) % 2 == 1]
            skip = np.zeros(E, np.int64)
            skip[flagged] = 1
            ids = np.full(E, -1, np.int32)
            ids[:len(flagged)] = flagged
            emu.sim_step(b, case.n_calls, skip=skip, parts=case.parts, cost_ticks=keys, order=_order(keys))
            emu.sim_step(b, case.n_calls, ids=ids, parts=case.parts, cost_ticks=keys)
        elif case.launch == "order":
            emu.sim_step(b, case.n_calls, parts=case.parts, cost_ticks=keys, order=_order(keys))
        else:
            emu.sim_step(b, case.n_calls, parts=case.parts)
        same(a, b, f"{case.name} step {t}")
    if case.after is not None:
        case.after(a)
    if log is not None:
        log(case, sc)
    return a


def _order(keys):
    """emloco_sim_set_cost_order: most contact work first (any order within equal keys: results do not depend on it)"""
    return np.ascontiguousarray(np.argsort(-keys.astype(np.int64), kind="stable").astype(np.int32))


# ==================================================================================================== EXISTING scenes
def _mk_scene(E, seed, **extra):
    """tests/test_gpu_sim.py: _mk"""
    def scene():
        root, dof, tgt = scene_state(E, seed + 1)
        return dict(models=varied_models(E, seed), root=root, dof=dof, tgt=tgt, **extra)
    return scene


def _self_collision_episode():
    """test_gpu_sim.test_self_collision_step_is_bit_exact_and_changes_the_motion"""
    E = 4
    models = varied_models(E, 21)
    for m in models:
        m.kp = m.kp * 0.05
    root, dof, tgt = scene_state(E, 22, perturbed_from=0)
    dof[:, :, 0] *= 3.0
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)


def _folding_ragdolls():
    """test_emu_kernels.test_sim_step_kernel_with_self_collision_is_bit_exact_vs_oracle"""
    E = 3
    models = varied_models(E, seed=5)
    root, dof, tgt = scene_state(E, seed=6, perturbed_from=0)
    dof[:, :, 0] *= 4.0
    dof[:, :, 1] *= 2.0
    for m in models:
        m.kp = m.kp * 0.05
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)


def _bumpy_episode():
    """test_gpu_sim.test_heightfield_ground_is_bit_exact_and_tilts_the_contact_forces"""
    E = 4
    root, dof, tgt = scene_state(E, 32, perturbed_from=0)
    root[:, 2] += 0.2 * (root[:, 0] - 50.0) + 0.1
    return dict(models=varied_models(E, 31), root=root, dof=dof, tgt=tgt, sc=True, hf=bumpy_heightfield(seed=5, amp=0.12, slope=0.2))


def _large_targets():
    """test_gpu_sim.test_large_random_targets_stay_finite_and_match_the_oracle: the first envs, new targets every control step"""
    E = 4
    root, dof, tgt = scene_state(E, 42)
    return dict(models=varied_models(E, 41), root=root, dof=dof, tgt=tgt)


def _large_targets_pre():
    rng = np.random.default_rng(43)
    sig = np.where(np.arange(4) % 2 == 0, 0.3, 1.2)[:, None].astype(np.float32)

    def pre(t, sims):
        tg = rng.normal(size=(4, 69)).astype(np.float32) * sig
        for s in sims:
            s.pd_target[:] = tg
    return pre


def _saturated():
    """test_emu_kernels.test_sim_step_kernel_with_saturated_drives_is_bit_exact_vs_oracle"""
    E = 4
    root, dof, tgt = scene_state(E, seed=12)
    return dict(models=varied_models(E, seed=11), root=root, dof=dof, tgt=tgt)


def _saturated_pre():
    rng = np.random.default_rng(13)
    _, _, tgt = scene_state(4, seed=12)

    def pre(t, sims):
        big = (rng.normal(size=(4, 69)) * 2.0).astype(np.float32)
        big[0] = tgt[0]
        for s in sims:
            s.pd_target[:] = big
    return pre


def _effort():
    """test_gpu_sim.test_effort_drives_through_the_c_abi_are_bit_exact_and_switch_back"""
    E = 4
    root, dof, _ = scene_state(E, 52)
    torque = (np.random.default_rng(52).normal(size=(48, 69)) * 120.0).astype(np.float32)
    torque[:, ::7] *= 8.0
    return dict(models=varied_models(E, 51), root=root, dof=dof, tgt=torque[:E].copy(), sc=True, params=dict(drive_mode=1))


def _effort_pre(t, sims):
    if t == 3:                                                   # back to position drives
        for s in sims:
            s.params.drive_mode = 0
            s.pd_target[:] = 0.0


def _fallen():
    """test_emu_kernels.test_sim_step_kernel_fallen_humanoids_are_bit_exact_vs_oracle"""
    E = 3
    root, dof, tgt = scene_state(E, seed=6, height=0.06, perturbed_from=0)
    s = np.sin(np.pi / 4)
    for e, ax in enumerate([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)]):
        root[e, 3:7] = [ax[0] * s, ax[1] * s, ax[2] * s, np.cos(np.pi / 4)]
    return dict(models=varied_models(E, seed=5), root=root, dof=dof, tgt=tgt, sc=True)


def _stairs():
    """test_gpu_sim.test_stairs_and_map_border_stay_on_the_oracles_bytes"""
    E = 6
    root, dof, tgt = scene_state(E, 42, perturbed_from=0)
    n = 200
    steps = ((np.arange(n)[:, None] // 3) % 4 * 30 + 0 * np.arange(n)[None, :]).astype(np.int16)
    root[:, 0] = [0.04, 9.93, 19.88, 5.0, 5.15, 12.31]
    root[:, 1] = [0.03, 10.0, 19.86, 0.02, 8.0, 19.89]
    root[:, 2] = 1.05 + steps[np.clip((root[:, 0] / 0.1).astype(int), 0, n - 1), 0] * 0.005
    return dict(models=varied_models(E, 41), root=root, dof=dof, tgt=tgt, hf=dict(samples=steps, horizontal_scale=0.1, vertical_scale=0.005))


def _corrected_mesh():
    """test_gpu_sim.test_slope_corrected_mesh_stays_on_the_oracles_bytes (dropped from 0.98 as the emulator twin does)"""
    E = 6
    root, dof, tgt = scene_state(E, 52, perturbed_from=0)
    steps, hf = corrected_stairs()
    root[:, 0] = [0.04, 9.93, 10.21, 19.88, 5.15, 12.31]
    root[:, 1] = [0.03, 10.0, 9.62, 19.86, 8.0, 19.89]
    root[:, 2] = 0.98 + steps[np.clip((root[:, 0] / 0.1).astype(int), 0, 199), np.clip((root[:, 1] / 0.1).astype(int), 0, 199)] * 0.005
    root[:, 7] = [0.5, 1.5, -1.0, 0.0, 1.2, -0.8]
    root[:, 8] = [0.0, -1.0, 1.5, 0.0, 0.0, 0.3]
    return dict(models=varied_models(E, 51), root=root, dof=dof, tgt=tgt, hf=hf)


def _handover():
    """test_emu_sim_handover._scene: airborne / standing / lying on more than 14 contacts"""
    E = 3
    root, dof, tgt = scene_state(E, seed=62, perturbed_from=0)
    root[0, 2] = 3.0
    dof[1] = 0.0
    root[1, 7:13] *= 0.25
    s = np.float32(np.sin(np.pi / 4))
    root[2, 2] = 0.06
    root[2, 3:7] = [s, 0.0, 0.0, s]
    return dict(models=varied_models(E, seed=61), root=root, dof=dof, tgt=tgt, sc=True)


def _split(E=S.SPLIT_ENVS_EMU):
    def scene():
        models, root, dof, tgt = S.split_scene(E)
        return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)
    return scene


def _abi_hf(kind):
    def scene():
        hf = S.offset_field(kind)
        models, root, dof, tgt = S.hf_scene(hf)
        return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True, hf=hf)
    return scene


def _layout(ground):
    def scene():
        models, root, dof, tgt = K.scene(ground)
        return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True, hf=K.heightfield() if ground == "hf" else None)
    return scene


def existing_cases():
    c = [Case("mk_seed0", _mk_scene(4, 0), 2),
         Case("mk_seed3_episode", _mk_scene(4, 3), 6),
         Case("mk_seed21_order_split_subset", _mk_scene(5, 21), 3, parts=2, launch="subset"),
         Case("self_collision_episode", _self_collision_episode, 4),
         Case("folding_ragdolls", _folding_ragdolls, 3, n_sub=4, n_calls=1),
         Case("bumpy_field_episode", _bumpy_episode, 4),
         Case("large_targets", _large_targets, 6, pre_step=_large_targets_pre()),
         Case("saturated_drives", _saturated, 6, n_sub=1, n_calls=1, pre_step=_saturated_pre()),
         Case("effort_drives", _effort, 4, pre_step=_effort_pre),
         Case("fallen", _fallen, 3, n_sub=4, n_calls=1),
         Case("stairs_and_border", _stairs, 4),
         Case("corrected_mesh", _corrected_mesh, 6),
         Case("handover_2_parts", _handover, 3, n_sub=4, n_calls=1, parts=2, launch="order"),
         Case("handover_4_parts", _handover, 3, n_sub=4, n_calls=1, parts=4)]
    for i, (n_sub, n_calls, n_parts) in enumerate(S.SPLIT_CASES):
        launch = "subset" if (n_sub, n_calls, n_parts) in S.SPLIT_SUBSET_CASES else ("order" if i % 2 == 1 else "plain")
        c.append(Case("split_%d_%d_%d" % (n_sub, n_calls, n_parts), _split(), 2, n_sub=n_sub, n_calls=n_calls, parts=n_parts, launch=launch))
    for kind in S.HF_KINDS:
        c.append(Case("offset_field_" + kind, _abi_hf(kind), 5, parts=4))
    for ground in ("plane", "hf"):
        c.append(Case("contact_layout_" + ground, _layout(ground), K.STEPS, n_sub=1, n_calls=1, launch="order"))
    return c


# ==================================================================================================== NEW scenes
def _start_bodies(sc):
    """float64 world position [E][24][3] and rotation matrices [E][24][3][3] of the start state (the oracle's forward kinematics)"""
    o = oracle_sim(sc["models"], sc["root"], sc["dof"], sc["tgt"])
    rb = o.fk().astype(np.float64)
    q = rb[:, :, 3:7]
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))
    return rb[:, :, :3], R


# ---------------------------------------------------------------------------------------------------- joint angles at and beyond pi
# sim_math.h: fdet_sincos flips the sign of sin / cos for an odd half-period; frotvec2quat calls it with |e| / 2, so the flip is
# reached with |e| >= pi -- resets and motion clips produce such dof positions.  (joint body, axis, |e|) per env:
ANGLE_JOINTS = (1, 2, 11, 15, 17, 18, 21)                      # L_Hip, L_Knee, Chest, L_Shoulder, L_Wrist, L_Hand, R_Elbow: tree depths 1 .. 8
ANGLE_ENVS = ("pi", "pi_plus_ulp", "pi_minus_ulp", "beyond", "beyond_negative", "mixed")


def _angle_scene():
    E = len(ANGLE_ENVS)
    root, dof, tgt = scene_state(E, 72, height=1.6, perturbed_from=0)
    dof[:, :, 0] *= 0.3
    rng = np.random.default_rng(73)
    up, dn = np.nextafter(PI32, np.float32(4)), np.nextafter(PI32, np.float32(0))
    for e, kind in enumerate(ANGLE_ENVS):
        for n, b in enumerate(ANGLE_JOINTS):
            d0 = 3 * (b - 1)
            if kind in ("pi", "pi_plus_ulp", "pi_minus_ulp"):
                v = np.zeros(3, np.float32)                     # along one axis: |e| is the stored number itself
                v[n % 3] = {"pi": PI32, "pi_plus_ulp": up, "pi_minus_ulp": dn}[kind] * (1 if n % 2 == 0 else -1)
            else:
                ax = rng.normal(size=3)
                ax /= np.linalg.norm(ax)
                mag = (3.3 + 0.85 * n) if kind != "mixed" else (np.pi + 1e-3, 2 * np.pi, 3 * np.pi - 1e-3, 4.0, 2 * np.pi + 1e-3, 7.5, 9.4)[n]
                v = (ax * mag * (-1 if kind == "beyond_negative" else 1)).astype(np.float32)
            dof[e, d0:d0 + 3, 0] = v
    return dict(models=varied_models(E, 71), root=root, dof=dof, tgt=tgt, sc=True)


def _angle_regime(sc):
    e = sc["dof"][:, :, 0].astype(np.float64).reshape(-1, 23, 3)
    th = np.linalg.norm(e, axis=2)[:, [b - 1 for b in ANGLE_JOINTS]]
    assert (th[0] == float(PI32)).all() and (th[1] == float(np.nextafter(PI32, np.float32(4)))).all(), th[:2]
    assert (th[2] == float(np.nextafter(PI32, np.float32(0)))).all(), th[2]
    assert (th[3:] > np.pi).all() and (th[3:] < 3 * np.pi).all(), th[3:]
    assert th[3:].max() > 2 * np.pi + 0.5                       # the second odd half-period too (|e| / 2 in (pi, 3 pi / 2))


# ---------------------------------------------------------------------------------------------------- root spin
SPIN = 150.0                                                    # rad/s; EMLOCO_WH_MAX / h = 120 rad/s at h = 1 / 120


def _spin_scene(max_ang_vel):
    def scene():
        E = 4
        root, dof, tgt = scene_state(E, 82, perturbed_from=1)
        axes = np.array([[0.36, 0.48, 0.8], [0.8, -0.6, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
        root[:, 10:13] = (SPIN * axes).astype(np.float32)
        root[0, 2], root[1, 2] = 3.0, 2.5                       # airborne; env 2 stands, env 3 lies on its back
        root[2, 2] = 0.93
        s = np.sin(np.pi / 4)
        root[3, 2], root[3, 3:7] = 0.12, [s, 0.0, 0.0, s]
        hf = None
        if max_ang_vel > 1.0 / (1.0 / 120.0):                   # the cap-alone variant spins over the bumpy field: the height-field
            hf = K.heightfield()                                # instantiation of the kernel has its own copy of the limiter
            for e in range(E):
                root[e, 2] += K._hf_height(hf, float(root[e, 0]), float(root[e, 1]))
        return dict(models=varied_models(E, 81), root=root, dof=dof, tgt=tgt, sc=True, hf=hf, params=dict(max_ang_vel=max_ang_vel))
    return scene


def _spin_regime(max_ang_vel):
    def regime(sc):
        w = np.linalg.norm(sc["root"][:, 10:13].astype(np.float64), axis=1)
        h = 1.0 / 120.0
        assert (w > 149.0).all() and (w > 1.0 / h).all()         # above the link-rotation cap of one radian per substep
        if max_ang_vel < 1.0 / h:
            assert (w > max_ang_vel).all()                      # ... and above max_ang_vel, which undercuts it
        else:
            assert max_ang_vel > w.max()                        # max_ang_vel out of reach: the rotation cap binds alone
        ground = np.zeros(4) if sc["hf"] is None else np.array([K._hf_height(sc["hf"], float(r[0]), float(r[1])) for r in sc["root"]])
        assert (sc["root"][:2, 2] - ground[:2]).min() > 2.0 and (sc["root"][2:, 2] - ground[2:]).max() < 1.0
    return regime


# ---------------------------------------------------------------------------------------------------- limb-limb contacts
def _closest(p0, p1, q0, q1):
    """closest points of two segments in float64 (model._segment_distance, returning the points)"""
    d1, d2, rr = p1 - p0, q1 - q0, p0 - q0
    aa, ee, ff = d1 @ d1, d2 @ d2, d2 @ rr
    if aa <= 1e-12 and ee <= 1e-12:
        s = t = 0.0
    elif aa <= 1e-12:
        s, t = 0.0, np.clip(ff / ee, 0, 1)
    else:
        cc = d1 @ rr
        if ee <= 1e-12:
            t, s = 0.0, np.clip(-cc / aa, 0, 1)
        else:
            bb = d1 @ d2
            den = aa * ee - bb * bb
            s = np.clip((bb * ff - cc * ee) / den, 0, 1) if den > 1e-12 else 0.0
            t = (bb * s + ff) / ee
            if t < 0:
                t, s = 0.0, np.clip(-cc / aa, 0, 1)
            elif t > 1:
                t, s = 1.0, np.clip((bb - cc) / aa, 0, 1)
    return p0 + d1 * s, q0 + d2 * t


def limb_hits(sc):
    """Per env, at the start state in float64: (segment pairs that hit -- closer than their radii AND pushed apart, k pen - c v_n > 0,
    with the bodies' velocities --, the smallest margin of those decisions over all pairs: |distance - radii| in metres or
    |force| / k, the smallest distance of a hitting pair)."""
    from emloco_amd import model as M
    pack = sc["sc"] if isinstance(sc["sc"], dict) else M.pack_self_collision(sc["models"])
    pos, R = _start_bodies(sc)
    rb = oracle_sim(sc["models"], sc["root"], sc["dof"], sc["tgt"]).fk().astype(np.float64)
    out = []
    for e in range(pos.shape[0]):
        a = pack["cap_a"][e].astype(np.float64)
        b = pack["cap_b"][e].astype(np.float64)
        r = pack["cap_r"][e].astype(np.float64)
        sb = pack["seg_body"]
        wa = np.stack([pos[e, sb[i]] + R[e, sb[i]] @ a[i] for i in range(len(sb))])
        wb = np.stack([pos[e, sb[i]] + R[e, sb[i]] @ b[i] for i in range(len(sb))])
        n, margin, closest = 0, np.inf, np.inf
        for i, j in pack["pairs"]:
            c1, c2 = _closest(wa[i], wb[i], wa[j], wb[j])
            dist = float(np.linalg.norm(c1 - c2))
            margin = min(margin, abs(dist - (r[i] + r[j])))
            if dist < r[i] + r[j] and dist > 1e-6:
                nrm, pen = (c1 - c2) / dist, r[i] + r[j] - dist
                pt = c2 + nrm * (r[j] - 0.5 * pen)
                vi, vj = (rb[e, sb[k], 7:10] + np.cross(rb[e, sb[k], 10:13], pt - pos[e, sb[k]]) for k in (i, j))
                F = pack["k"] * min(pen, pack["max_pen"]) - pack["c"] * ((vi - vj) @ nrm)
                margin = min(margin, abs(F) / pack["k"])
                if F > 0:
                    n += 1
                    closest = min(closest, dist)
        out.append((n, margin, closest))
    return out


def _folded(E, seed, scale, rest):
    root, dof, tgt = scene_state(E, seed + 1, height=1.4, perturbed_from=0)
    dof[:, :, 0] *= scale
    if rest:
        dof[:, :, 1] = 0.0
        root[:, 7:13] = 0.0
    return varied_models(E, seed), root, dof, tgt


def _limb_rest_scene():
    models, root, dof, tgt = _folded(3, 97, 4.0, rest=True)
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)


def _limb_rest_regime(sc):
    assert not sc["dof"][:, :, 1].any() and not sc["root"][:, 7:13].any()          # every velocity zero: v_t = 0 at each hit
    hits = limb_hits(sc)
    assert all(n >= 1 and m > 1e-5 and c > 1e-3 for n, m, c in hits), hits


def _limb_mu0_scene():
    from emloco_amd.model import pack_self_collision
    models, root, dof, tgt = _folded(3, 93, 4.0, rest=False)
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=pack_self_collision(models, mu=0.0))


def _limb_mu0_regime(sc):
    assert sc["sc"]["mu"] == 0.0
    assert all(n >= 1 and m > 1e-5 for n, m, _ in limb_hits(sc)), limb_hits(sc)


def _tucked(E, seed, noise=0.03):
    """knees to the chest, shins against the thighs, the arms folded across the chest, the spine curled: every limb lies on others"""
    root, dof, tgt = scene_state(E, seed + 1, height=1.4, perturbed_from=0)
    rng = np.random.default_rng(seed + 2)
    root[:, 7:13] = 0.0
    pose = np.zeros((24, 3))
    pose[1] = pose[5] = [0, -2.5, 0]
    pose[2] = pose[6] = [0, 2.5, 0]
    pose[15], pose[20], pose[16], pose[21] = [0, 0, -1.6], [0, 0, 1.6], [0, 0, -2.6], [0, 0, 2.6]
    pose[9] = pose[10] = pose[11] = pose[12] = [0, 0.7, 0]
    for e in range(E):
        dof[e, :, 0] = (pose[1:] + rng.normal(size=(23, 3)) * noise).reshape(-1)
        dof[e, :, 1] *= 0.25                                    # moving: the hits rub (v_t > 0), none of them at rest
    return varied_models(E, seed), root, dof, tgt


SC_MAXHITS = 32


def _limb_cap_scene():
    models, root, dof, tgt = _tucked(3, 111)
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)


def _limb_cap_regime(sc):
    hits = limb_hits(sc)
    assert all(n > SC_MAXHITS + 2 and m > 1e-5 for n, m, _ in hits), hits    # float64: more overlapping pairs than hit slots


# A left / right symmetric humanoid: the left limbs mirrored onto the right side, the trunk centred.  IEEE arithmetic is symmetric
# in the sign, so with the root on the plane y = 0 mirrored joint angles give mirrored body states bit for bit.
SYM_PAIRS = ((1, 5), (2, 6), (3, 7), (4, 8), (14, 19), (15, 20), (16, 21), (17, 22), (18, 23))
SYM_CENTRE = (0, 9, 10, 11, 12, 13)
GEOM_BOX = 2


def symmetric(m):
    m = m.scaled(1.0, 1.0)
    for b in SYM_CENTRE:
        for arr in (m.joint_off, m.com, m.geom_a, m.geom_b):
            arr[b, 1] = 0.0
        m.inertia[b, 3] = m.inertia[b, 5] = 0.0
    for l, r in SYM_PAIRS:
        for arr in (m.joint_off, m.com, m.geom_a):
            arr[r] = arr[l] * [1, -1, 1]
        m.geom_b[r] = m.geom_b[l] * ([1, 1, 1] if m.geom_type[l] == GEOM_BOX else [1, -1, 1])      # half extents | second end
        m.inertia[r] = m.inertia[l] * [1, 1, 1, -1, 1, -1]
        m.mass[r], m.geom_r[r] = m.mass[l], m.geom_r[l]
        for arr in (m.kp, m.kd, m.armature, m.effort, m.lim_lower, m.lim_upper):
            arr[3 * (r - 1):3 * r] = arr[3 * (l - 1):3 * l]
    return m


def mirror_pose(dof_env):
    """joint angles / rates [69] with the right side the mirror image of the left (a rotation vector is a pseudo-vector: x and z flip)"""
    e = dof_env.reshape(23, 3).copy()
    for b in SYM_CENTRE[1:]:
        e[b - 1, 0] = e[b - 1, 2] = 0.0
    for l, r in SYM_PAIRS:
        e[r - 1] = e[l - 1] * np.array([-1, 1, -1], e.dtype)
    return e.reshape(-1)


def _limb_cross_scene():
    """Both forearms folded across the chest, mirror images of each other: each crosses the plane y = 0 and so they meet there"""
    E = 3
    models = [symmetric(m) for m in varied_models(E, 121)]
    root, dof, tgt = scene_state(E, 122, height=1.4, perturbed_from=0)
    root[:, 0] = root[:, 1] = 0.0                               # on the mirror plane: world coordinates round the same on both sides
    root[:, 3:7] = [0, 0, 0, 1]
    root[:, 7:13] = 0.0
    dof[:, :, 0] *= 0.5
    for e in range(E):
        dof[e, 3 * 14:3 * 14 + 3, 0] = [0, 0, -2.0 - 0.05 * e]   # L_Shoulder, L_Elbow about z (the right side by mirror_pose)
        dof[e, 3 * 15:3 * 15 + 3, 0] = [0, 0, -1.8 + 0.03 * e]
        dof[e, :, 0] = mirror_pose(dof[e, :, 0])                 # the POSE is mirrored; the joint rates are not, or every left-right hit
    return dict(models=models, root=root, dof=dof, tgt=tgt, sc=True)   # would have its relative velocity along its normal (v_t = 0)


def _limb_cross_regime(sc):
    from emloco_amd import model as M
    pack = M.pack_self_collision(sc["models"])
    assert [16, 21] in pack["pairs"].tolist()
    pos, R = _start_bodies(sc)
    for e in range(pos.shape[0]):
        w = [pos[e, b] + R[e, b] @ pack[k][e, b].astype(np.float64) for b in (16, 21) for k in ("cap_a", "cap_b")]
        assert w[0][1] > 0.02 and w[1][1] < -0.02, w            # the left forearm reaches across the mirror plane
        dist = M._segment_distance(w[0], w[1], w[2], w[3])
        assert dist < 1e-7, dist                                # 1e-6 m is where the kernel gives up on a normal (dist2 <= 1e-12)


# ---------------------------------------------------------------------------------------------------- ties at the 20th contact
# A symmetric humanoid upright with zero joint angles, pressed into the plane, contact_offset so large that all 68 candidates are
# inside: 48 are dropped, shallowest first, "ties -> highest candidate id".  Heights are made EXACT: every z of the model is a
# multiple of 2^-10 m, the rotations are identities, so each candidate's distance is a short sum of such multiples in fp32 and in
# float64 alike, and mirrored candidates have bit-equal distances.  The feet are arranged so that the deepest 16 are the toe boxes'
# corners and the next eight, all at one height, the bottom corners of the two ankle boxes: ids 5..8 (left) and 25..28 (right).  Four of
# the eight survive: the documented rule keeps the LEFT ankle's, the opposite rule the right ankle's -- the other ankle has no contact.
# The arms hang at pelvis height and the hip capsules start higher, so that candidates 0 | 64 (the two slots of lane 0) and 21 | 53
# (lanes 32 apart) have bit-equal distances while they are the shallowest left.
Q = 1024.0
TIE_OFFSET = 3.0
TIE_DEPEN = 0.1                                                 # every penetrating contact asks for the same (capped) push-out speed: heels carry load too
MAXCAND = 96


def _quant(x):
    return np.round(np.asarray(x, np.float64) * Q) / Q


def tie_model(m):
    m = symmetric(m)
    for arr in (m.joint_off, m.geom_a, m.geom_b):
        arr[:, 2] = _quant(arr[:, 2])
    m.geom_r[:] = _quant(m.geom_r)
    for a, t in ((3, 4), (7, 8)):                               # ankle box: its bottom 8 / 1024 m above the toe box's top
        toe_top = m.joint_off[t, 2] + m.geom_a[t, 2] + m.geom_b[t, 2]
        m.geom_a[a, 2] = toe_top + 8 / Q + m.geom_b[a, 2]

    def z_of(b):
        return 0.0 if b == 0 else z_of(m.parent[b]) + m.joint_off[b, 2]
    # the arms hang lower, by as much as puts candidate 64 = second end of the right elbow capsule (and 55, its mirror image) level
    # with the underside of the pelvis sphere, candidate 0
    drop = (z_of(16) + m.geom_b[16, 2] - m.geom_r[16]) - (m.geom_a[0, 2] - m.geom_r[0])
    for b in (14, 19):
        m.joint_off[b, 2] -= drop
    # the hip capsules' first ends (candidates 1 and 21) level with the second ends of the shoulder capsules (candidates 53 and 62)
    for hip, sh in ((1, 15), (5, 20)):
        m.geom_a[hip, 2] = (z_of(sh) + m.geom_b[sh, 2] - m.geom_r[sh]) + m.geom_r[hip] - z_of(hip)
    return m


def candidates(m):
    """(body, local point) of every contact candidate in the kernel's order (oracle_sim.c: find_contacts)"""
    out = []
    for b in range(24):
        ga, gb = m.geom_a[b], m.geom_b[b]
        if m.geom_type[b] == 0:
            out.append((b, ga))
        elif m.geom_type[b] == 1:
            out += [(b, ga), (b, gb)]
        else:
            out += [(b, ga + np.where([k & 1, k & 2, k & 4], gb, -gb)) for k in range(8)]
    return out


def tie_heights(m, root_z):
    """float64 distance of every candidate to the plane z = 0 in the start pose (identity rotations), exact for a `tie_model`"""
    z = np.zeros(24)
    for b in range(1, 24):
        z[b] = z[m.parent[b]] + m.joint_off[b, 2]
    return np.array([root_z + z[b] + lp[2] - m.geom_r[b] for b, lp in candidates(m)])


def kept_after_cut(dist, offset, highest_id_first):
    """ids of the contacts kept: candidates inside `offset`, the shallowest dropped until 20 are left, ties broken by id"""
    ids = [c for c in range(len(dist)) if dist[c] < offset]
    while len(ids) > K.MAXC:
        worst = max(ids, key=lambda c: (dist[c], c if highest_id_first else -c))
        ids.remove(worst)
    return ids


def _tie_root_z(m):
    z = np.zeros(24)
    for b in range(1, 24):
        z[b] = z[m.parent[b]] + m.joint_off[b, 2]
    return -(z[3] + m.geom_a[3, 2] - m.geom_b[3, 2]) - 4 / Q      # the ankle boxes' bottoms 4 / 1024 m under the plane


def _tie_scene():
    E = 4
    models = [tie_model(m) for m in varied_models(E, 131)]
    root, dof, tgt = scene_state(E, 132, perturbed_from=E)       # nothing perturbed: identity rotations, zero angles and rates
    root[:, 0] = np.arange(E) * 0.5
    root[:, 1] = 0.0
    for e in range(E):
        root[e, 2] = _tie_root_z(models[e])
    return dict(models=models, root=root, dof=dof, tgt=tgt, params=dict(contact_offset=TIE_OFFSET, max_depen_vel=TIE_DEPEN))


def _tie_regime(sc):
    assert not sc["dof"].any() and (sc["root"][:, 3:7] == [0, 0, 0, 1]).all()
    for e, m in enumerate(sc["models"]):
        assert float(np.float32(sc["root"][e, 2])) == _tie_root_z(m)
        d = tie_heights(m, float(sc["root"][e, 2]))
        assert (d * Q == np.round(d * Q)).all() and np.abs(d).max() < 4.0        # multiples of 2^-10 below 4: exact in fp32 too
        assert (d < TIE_OFFSET).all() and len(d) == 68
        hi, lo = kept_after_cut(d, TIE_OFFSET, True), kept_after_cut(d, TIE_OFFSET, False)
        assert sorted(set(hi) - set(lo)) == [5, 6, 7, 8] and sorted(set(lo) - set(hi)) == [25, 26, 27, 28], (hi, lo)
        assert d[5] == d[25] and d[8] == d[28] and d[5] < 0.0     # the tie straddles the 20th place, and the tied corners penetrate
        assert d[0] == d[64] == d[55] and d[21] == d[53] == d[1] == d[62]        # slot tie in lane 0; lanes 21 | 53: 32 apart
        order = sorted(range(68), key=lambda c: d[c])
        assert order.index(0) >= K.MAXC and order.index(21) >= K.MAXC             # ... both among the dropped: maxima in turn


def tie_bodies_with_force(osim):
    """after one single-substep step: the ankle whose corners were kept carries contact force, the other one none"""
    f = np.abs(osim.contact_force).sum(-1)
    assert (f[:, 3] > 0).all() and (f[:, 7] == 0).all(), f[:, [3, 4, 7, 8]]
    assert (np.abs(osim.lambda_ws[:, 5:9]).sum((1, 2)) > 0).all() and not osim.lambda_ws[:, 25:29].any()


# ---------------------------------------------------------------------------------------------------- slope-corrected mesh
# The sphere of the pelvis (candidate 0: its centre is the root position, bit for bit) against the vertical faces of a small mesh:
# a plateau whose top rises and falls along y (its wall triangles are not right-angled), with a second block on its diagonal (where
# risers along x and along y meet, vertex moves turn triangles over: both orientations in mesh_plane).  What follows restates
# mesh_vert / mesh_tri / mesh_plane / mesh_walls of csrc/sim_kernels.hip in float64.
MESH_HS, MESH_VS, MESH_N = 0.1, 0.005, 40
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "face")
BAND = 1e-5                                                     # doubt band [m]: a region must hold at every point this far around the centre


def region_field():
    from emloco_amd.gym import terrain_utils as T
    s = np.zeros((MESH_N, MESH_N), np.int16)
    j = np.arange(MESH_N)
    s[15:25, 10:30] = (100 + 6 * np.minimum(j, MESH_N - 1 - j))[None, 10:30]       # 0.8 to 1.07 m: 3 cm per cell up, then down
    s[25:32, 30:36] = 160
    verts, _ = T.convert_heightfield_to_trimesh(s, MESH_HS, MESH_VS, 0.9)
    mx, my = T.mesh_vertex_moves(verts, s.shape, MESH_HS)
    return dict(samples=s, horizontal_scale=MESH_HS, vertical_scale=MESH_VS, move_x=mx, move_y=my)


class Mesh64:
    def __init__(self, hf):
        import oracle
        self.hf, self.smp = hf, hf["samples"]
        self.mv = oracle.pack_mesh_moves(hf["move_x"], hf["move_y"])
        self.nx, self.ny = self.smp.shape

    def vert(self, ci, cj):
        b = int(self.mv[ci, cj])
        return np.array([ci + (b & 3) - 1, cj + ((b >> 2) & 3) - 1, MESH_VS * float(self.smp[ci, cj])])

    def tris(self, x, y):
        """(ci, cj, t, A, B, C) of the 3 x 3 cells around the regular cell of (x, y); vertices in grid units (z in metres); nothing
        where no vertex nearby has moved"""
        gx, gy = x / MESH_HS, y / MESH_HS
        i, j = int(np.clip(np.floor(gx), 0, self.nx - 2)), int(np.clip(np.floor(gy), 0, self.ny - 2))
        if not (self.mv[i, j] & 16):
            return
        for ci in range(max(i - 1, 0), min(i + 1, self.nx - 2) + 1):
            for cj in range(max(j - 1, 0), min(j + 1, self.ny - 2) + 1):
                A = self.vert(ci, cj)
                yield ci, cj, 0, A, self.vert(ci + 1, cj), self.vert(ci + 1, cj + 1)
                yield ci, cj, 1, A, self.vert(ci + 1, cj + 1), self.vert(ci, cj + 1)

    def plane(self, x, y):
        """mesh_plane: (height of the highest mesh triangle covering (x, y), its unit normal, orientation outcomes met on the way:
        the set of (sign of the area, which test failed or "in"))"""
        gx, gy = x / MESH_HS, y / MESH_HS
        best, seen = None, set()
        for ci, cj, t, A, B, C in self.tris(x, y):
            bx, by, qx, qy = B[0] - A[0], B[1] - A[1], C[0] - A[0], C[1] - A[1]
            ar = bx * qy - by * qx
            if ar == 0.0:
                continue
            px, py = gx - A[0], gy - A[1]
            eb, ec = px * qy - py * qx, bx * py - by * px
            sg = 1.0 if ar > 0 else -1.0
            what = "eb" if sg * eb < 0 else ("ec" if sg * ec < 0 else ("sum" if sg * (eb + ec) > sg * ar else "in"))
            seen.add((int(sg), what, float(min(abs(eb), abs(ec), abs(eb + ec - ar)))))
            if what != "in":
                continue
            zb, zc = B[2] - A[2], C[2] - A[2]
            sx, sy = (zb * qy - zc * by) / ar, (zc * bx - zb * qx) / ar
            z = A[2] + px * sx + py * sy
            if best is None or z > best[0]:
                best = (z, sx / MESH_HS, sy / MESH_HS)
        if best is None:
            zt, n, _ = K._hf_plane(self.hf, x, y)
            return zt, np.array(n), seen
        inv = 1.0 / np.sqrt(1.0 + best[1] ** 2 + best[2] ** 2)
        return best[0], np.array([-best[1] * inv, -best[2] * inv, inv]), seen

    def walls(self, P):
        """mesh_walls: per vertical (collapsed) triangle near P: (region of the closest point, its distance, side >= 0, outcomes of the
        region tests as a set of (source line, test, result))"""
        out = []
        for ci, cj, t, A, B, C in self.tris(P[0], P[1]):
            if (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0]) != 0.0:
                continue
            va, vb, vc = (np.array([V[0] * MESH_HS, V[1] * MESH_HS, V[2]]) - P for V in (A, B, C))
            ab, ac = vb - va, vc - va
            fn = np.cross(ab, ac)
            if fn @ fn == 0.0:
                continue
            d1, d2, d3, d4, d5, d6 = ab @ -va, ac @ -va, ab @ -vb, ac @ -vb, ab @ -vc, ac @ -vc
            vcc, vbb, vaa = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            rec = set()

            def T(line, name, val):
                rec.add((line, name, bool(val)))
                return val
            if T(285, "d1<=0", d1 <= 0) and T(285, "d2<=0", d2 <= 0):
                lab, q = "A", va
            elif T(286, "d3>=0", d3 >= 0) and T(286, "d4<=d3", d4 <= d3):
                lab, q = "B", vb
            elif T(287, "vc<=0", vcc <= 0) and T(287, "d1>=0", d1 >= 0) and T(287, "d3<=0", d3 <= 0):
                lab, q = "AB", va + ab * (d1 / (d1 - d3))
            elif T(288, "d6>=0", d6 >= 0) and T(288, "d5<=d6", d5 <= d6):
                lab, q = "C", vc
            elif T(289, "vb<=0", vbb <= 0) and T(289, "d2>=0", d2 >= 0) and T(289, "d6<=0", d6 <= 0):
                lab, q = "AC", va + ac * (d2 / (d2 - d6))
            elif T(290, "va<=0", vaa <= 0) and T(290, "d4-d3>=0", d4 - d3 >= 0) and T(290, "d5-d6>=0", d5 - d6 >= 0):
                lab, q = "BC", vb + (vc - vb) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
            else:
                den = 1.0 / (vaa + vbb + vcc)
                lab, q = "face", va + ab * (vbb * den) + ac * (vcc * den)
            out.append((lab, float(np.linalg.norm(q)), bool(-q @ fn >= 0.0), rec, P + q))
        return out

    def nearest_wall(self, P):
        """What mesh_walls selects for a centre outside the solid: (regions of the triangles whose closest point is the nearest,
        that distance, the point), or None where P is under the surface or no wall is nearer than the surface below"""
        zt, n, _ = self.plane(P[0], P[1])
        dsel = (P[2] - zt) * n[2]
        if dsel < 0.0:
            return None
        w = [x for x in self.walls(P) if x[2] and x[1] < dsel]
        if not w:
            return None
        dmin = min(x[1] for x in w)
        return {x[0] for x in w if x[1] < dmin + 1e-9}, dmin, next(x[4] for x in w if x[1] == dmin)


def _band(P):
    return [P + BAND * np.array(d) for d in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
                                                (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, -1, 1))]


GAP = 0.008                                                     # the sphere's surface this far from the closest point: inside the contact offset

# (region the nearest wall triangle must report, a centre found by sampling; the scene keeps its closest point and direction and
# moves the centre to radius + GAP).  "BC" and "AB" are chosen where the triangle is obtuse: the centre lies beyond B along AB
# (d3 > 0) and beyond C along AC (d6 > 0) without being in B's or C's region.
# A vertex of the mesh is shared by several wall triangles under different names: the "A" centre is nearest to a point that is A of one
# triangle and B or C of its neighbours, the "B" centre to one that is B and C.  The face region is env 5 of the scene (the centre ON a face).
REGION_ENVS = (("A", (3.2856, 3.5844, 0.813)), ("B", (1.4617, 2.0236, 1.1924)), ("AB", (1.5503, 2.9387, 1.0452)),
               ("AC", (2.4723, 1.3018, 1.0089)), ("BC", (1.3622, 1.4639, 1.0998)))
REGION_TESTS = ((287, "d3<=0", False), (289, "d6<=0", False))


def _upright(E, seed):
    root, dof, tgt = scene_state(E, seed + 1, perturbed_from=E)
    return varied_models(E, seed), root, dof, tgt


def _mesh_scene():
    """envs 0-4: the pelvis sphere nearest to a vertex / an edge of a wall triangle, one region each; env 5: its centre ON a vertical
    face (three units in the last place in front of it); env 6 / 7: over a triangle the vertex moves have turned over, outside it past
    its first edge / inside it"""
    E = len(REGION_ENVS) + 3
    models, root, dof, tgt = _upright(E, 141)
    hf = region_field()
    M = Mesh64(hf)
    for e, (_, p0) in enumerate(REGION_ENVS):
        p0 = np.array(p0)
        _, _, q = M.nearest_wall(p0)
        root[e, :3] = q + (p0 - q) / np.linalg.norm(p0 - q) * (float(np.float32(models[e].geom_r[0])) + GAP)
    x = np.float32(np.float32(15.0) * np.float32(MESH_HS))       # the face's x as the kernel forms it: fmaf(15, 0.1f, 0)
    for _ in range(3):
        x = np.nextafter(x, np.float32(0))
    root[5, :3] = [x, 1.7475, 0.45]
    root[6, :3] = [2.535, 2.961, 1.2]
    root[7, :3] = [2.455, 2.965, 1.2]
    return dict(models=models, root=root, dof=dof, tgt=tgt, hf=hf)


def _mesh_regime(sc):
    M = Mesh64(sc["hf"])
    tests, seen_regions = set(), set()
    for e, (label, _) in enumerate(REGION_ENVS):
        P = sc["root"][e, :3].astype(np.float64)
        rad = float(np.float32(sc["models"][e].geom_r[0]))
        found = [M.nearest_wall(p) for p in _band(P)]
        assert all(f is not None and label in f[0] and f[0] == found[0][0] for f in found), (e, label, found[0])
        assert BAND < found[0][1] - rad < 0.02 - BAND, (e, found[0][1] - rad)      # a contact, and not a penetration
        seen_regions |= found[0][0]
        per_point = [set().union(*[w[3] for w in M.walls(p)]) for p in _band(P)]
        tests |= set.intersection(*per_point)
    assert set(REGION_TESTS) <= tests, tests                    # the obtuse-triangle sides of the edge tests, at every point of a band
    labs, dist, _ = M.nearest_wall(sc["root"][5, :3].astype(np.float64))
    assert labs == {"face"} and 0.0 < dist < 5e-7, (labs, dist)   # 1e-6 is where the kernel falls back to the face normal
    assert seen_regions | labs == set(REGIONS)                   # each vertex region, each edge region and the face in turn
    for e, want in ((6, "eb"), (7, "in")):
        for p in _band(sc["root"][e, :3].astype(np.float64)):
            seen = M.plane(p[0], p[1])[2]
            assert any(sg < 0 and what == want and mar > 1e-3 for sg, what, mar in seen), (e, seen)


def new_cases():
    return [
        Case("joint_angles_at_and_beyond_pi", _angle_scene, 2, regime=_angle_regime, new=True,
             closes=("const float sgn = (((long)kf) & 1) ? -1.0f : 1.0f;",)),
        Case("root_spin_clamped", _spin_scene(100.0), 2, regime=_spin_regime(100.0), new=True,
             closes=("if (n > prm.max_ang_vel) { const float sc = prm.max_ang_vel / n; V0[0] *= sc; V0[1] *= sc; V0[2] *= sc; clamped = true; }",)),
        Case("root_spin_rotation_cap_alone", _spin_scene(400.0), 2, regime=_spin_regime(400.0), new=True,
             closes=("if (prm.max_ang_vel < wlim) wlim = prm.max_ang_vel;",)),
        Case("limbs_overlap_at_rest", _limb_rest_scene, 1, regime=_limb_rest_regime, new=True, closes=("if (vt2 > 1e-12f) {",)),
        Case("limbs_without_friction", _limb_mu0_scene, 2, regime=_limb_mu0_regime, new=True,
             closes=("if (d.sc_mu > 0.0f) {      // Coulomb friction capped by the contact's damper: - min(mu F / |v_t|, c) v_t",)),
        Case("limbs_crossing_exactly", _limb_cross_scene, 1, regime=_limb_cross_regime, new=True,
             closes=("if (dist2 < rsum * rsum && dist2 > 1e-12f) {",)),
        Case("limbs_more_hits_than_slots", _limb_cap_scene, 2, regime=_limb_cap_regime, new=True,
             closes=("if (hit && slot < EMLOCO_SC_MAXHITS) {", "if (nh > EMLOCO_SC_MAXHITS) nh = EMLOCO_SC_MAXHITS;")),
        Case("mesh_regions_face_normal_and_turned_triangles", _mesh_scene, 1, regime=_mesh_regime, new=True,
             closes=("else if (vcc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { const float w = d1 / (d1 - d3); for (int k = 0; k < 3; ++k) q[k] = fmaf(w, ab[k], va[k]); }",
                     "else for (int k = 0; k < 3; ++k) nsel[k] = fn[k] * ifn;",
                     "const bool in = ar > 0.0f ? (eb >= 0.0f && ec >= 0.0f && eb + ec <= ar) : (eb <= 0.0f && ec <= 0.0f && eb + ec >= ar);")),
        Case("ties_at_the_20th_contact", _tie_scene, 1, n_sub=1, n_calls=1, regime=_tie_regime, after=tie_bodies_with_force, new=True,
             closes=("if (act[s] && (cdist[s] > best || (cdist[s] == best && lane + 64 * s > bid))) { best = cdist[s]; bid = lane + 64 * s; }",
                     "if (ob > best || (ob == best && oi > bid)) { best = ob; bid = oi; }")),
    ]


# ==================================================================================================== launch level
def run_launch_extras(emu):
    """What the launchers of csrc/sim_capi.hip do besides the plain step, each against the oracle: forward kinematics of every env /
    of an id list that ends at its first -1 / with fewer workgroups than entries; the row copy of the indexed setters with -1 padding,
    an id past the end and a grid rounded up; a step whose grid is rounded up; a lost hand-over."""
    E = 5
    models, root, dof, tgt = S.split_scene(E)
    ref = oracle_sim(models, root, dof, tgt)
    ref.fk()
    for ids, grid in ((None, 0), (np.array([3, 1, -1, -1], np.int32), 0), (np.array([4, 0, 2, 1, -1], np.int32), 2)):
        b = oracle_sim(models, root, dof, tgt)
        b.rb_state[:] = -7.0
        emu.sim_fk(b, ids=ids, grid=grid)
        listed = np.ones(E, bool)
        if ids is not None:
            listed[:] = False
            listed[ids[:list(ids).index(-1)]] = True
        assert np.array_equal(b.rb_state[listed], ref.rb_state[listed]) and (b.rb_state[~listed] == -7.0).all(), ids
    rng = np.random.default_rng(3)
    src = rng.normal(size=(E, 13)).astype(np.float32)
    dst = np.zeros((E, 13), np.float32)
    emu.sim_copy_rows(src, dst, np.array([2, -1, 7, 4], np.int32), 13, E, grid_pad=3)
    want = np.zeros_like(dst)
    want[[2, 4]] = src[[2, 4]]
    assert np.array_equal(dst, want)
    a = oracle_sim(models, root, dof, tgt, self_collision=True, n_sub=4)
    b = oracle_sim(models, root, dof, tgt, self_collision=True, n_sub=4)
    keys = np.zeros(E, np.uint32)
    a.step(1)
    emu.sim_step(b, 1, parts=2, grid_pad=7, cost_ticks=keys)
    same(a, b, "grid rounded up")
    assert keys.max() > 0
    before = b.rb_state.copy()
    a.step(1)
    import os
    os.environ["EMLOCO_EMU_POISON"] = "1"
    try:
        assert emu.sim_step(b, 1, parts=4, expect_error=True) == 1          # EMLOCO_ERR_PART_TIMEOUT
    finally:
        del os.environ["EMLOCO_EMU_POISON"]
    keep = np.arange(E) != 1
    assert np.array_equal(a.rb_state[keep], b.rb_state[keep]) and np.array_equal(b.rb_state[1], before[1])


def main(argv):
    """Runs the whole table (and the launch-level checks) in this process: what tests/test_sim_branches_cpu.py starts as a child
    with EMLOCO_EMU_EXTRA=--coverage.  `--skip NAME` leaves a scene out (to see which line it alone takes)."""
    import time
    import emu
    skip = {argv[i + 1] for i, a in enumerate(argv) if a == "--skip"}
    t0, total = time.time(), 0
    emu.lib()
    print(f"emulator built or found in {time.time() - t0:.0f} s", flush=True)
    for case in existing_cases() + new_cases():
        if case.name in skip:
            print(f"{case.name}: skipped")
            continue
        t1 = time.time()
        run_emulated(case, emu)
        n = case.cost(case.scene())
        total += n
        print(f"{case.name}: {n} env-substeps, {time.time() - t1:.1f} s, bit-exact", flush=True)
    run_launch_extras(emu)
    print(f"{total} env-substeps, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1:])

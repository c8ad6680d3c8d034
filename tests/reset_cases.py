"""Case tables and judges of the reset conformance matrix (include/emloco_task.h: "Fused reset of finished envs"), shared by the emulator
run on the CPU (tests/test_reset_matrix_cpu.py) and the device run (tests/test_gpu_reset_matrix.py): the two differ in the executor only.

Scope: reset_sample_kernel (frame blend, slerp, rotation vectors, the random-heading turn, placement, centre-height mean), the
kinematics of the reset envs, reset_fix_height, reset_capture_pose, reset_amp_history_kernel and reset_fill_rnd_kernel.  Trajectory
generation is pinned to the reference goldens elsewhere; here only the real-path row pick is observed through traj_verts -- unless a
case says traj=True (the cases of tests/chain_cases.py do): then judge_traj holds traj_verts, waypoint_traj and the inversion flag to
kernel_refs.reset_trajectory in float64.  Such a case may also carry its own scalars of EmlocoResetBufs ("scalars"), tables
("const": see const_of) and explicit real-path rows ("real_pick").

An executor takes a case (make_case) and returns every buffer a reset may write as CPU numpy arrays (OUT_KEYS), having started from
initial(): garbage in the simulator state, NaN / sentinels in the outputs.  judge() compares the listed envs with the float64
references of tests/kernel_refs.py (float outputs through a kernel_refs.Table: bar = MARGIN x the float32 evaluation's own error of
the same function), with the fp32 oracle (ground height) and bit for bit (copies, ids, flags, zeros, envs that are not listed).

The motion cache is synthetic (world()): two random clips (37 frames at 1/30 s, 61 frames at 1/24 s, random unit quaternions), a
single-frame clip (its length is one frame time: a length of 0 makes the phase 0 / 0 in the reference as well), an edge clip of exactly
representable quaternions (EDGE_Q: identical, antipodal and orthogonal neighbours, joints at identity and at exactly 180 degrees) and a
static clip of near-identity joints (1e-4 .. 1e-2 rad).

Classes of joint elements (by the float64 blended quaternion's w): |w| < 1e-5 "180": the rotation vector is +-pi axis and both signs are
the same rotation, compared up to that sign (the root rotation is compared up to the sign of the quaternion in the rows whose time lies
within rounding of a frame, where the frame pair the time falls into decides it, and strictly everywhere else); |w| > 1 - 1e-3 "near-identity": sqrt(1 - w^2) cancels in float32 (relative error
6e-8 / angle^2), a Table name of its own so that it does not loosen the generic bar; every other joint: generic.

Near-branch elements (left out of the float comparison, their share per family capped at 1 %, asserted on the references alone by
near_shares()): u n_motions / u n_valid within 1e-5 n of an integer; a pair of frames whose cosine is within 1e-5 of 0 (the flip) or of
[sqrt(1 - 1e-6), 1] (midpoint / q0) unless the two frames are equal or antipodal (every branch returns q0) or the cosine is exactly 0
(sums of exact products: both precisions compute 0); |sin theta - 1e-5| < 1e-10; in the history rows a rotation vector within 1e-10 of
the 1e-5 threshold of exp_map_to_quat.  One helper (joint_near) builds the joint mask for the judges and for near_shares().
"""
import functools

import numpy as np
import torch

import kernel_refs as R

F32, F64 = torch.float32, torch.float64
RANDOM_HEADING, INIT_HEADING, HEADING_INVERSION, ADJUST_ROOT_VEL, REAL_PATH, FIXED_LOCATION, NO_AMP_HISTORY = 1, 2, 4, 8, 16, 32, 64
RND = 512
RND_MOTION, RND_TIME, RND_YAW, RND_SPEED, RND_LOC, RND_REAL = 0, 1, 2, 3, 4, 5
E, NB, NDOF, MAXCAND = 300, 24, 69, 96
AMP_STEPS, AMP_ROW, NV, NS = 15, 206, 101, 15
DT, HEIGHT_TOL, HSCALE, VSCALE = 1.0 / 30.0, 0.02, 0.1, 0.005
FIXED_XY = (4.1, 3.0)
N_VALID, N_REAL = 97, 261
CLIP_A, CLIP_B, CLIP_SINGLE, CLIP_EDGE, CLIP_NEAR = range(5)
TOP = 1.0 - 2.0 ** -24                       # the largest uniform of the device generator
REL = 1e-5                                    # band of the near-branch elements (relative to the operand scale)
CAP = 0.01                                    # largest share of near-branch elements per family

h = 0.5                                       # (1/2, 1/2, 1/2, 1/2) and its kin: unit quaternions of exact halves
EDGE_Q = [(0, 0, 0, 1), (0, 0, 0, 1), (0, 0, 0, -1), (1, 0, 0, 0), (1, 0, 0, 0), (-1, 0, 0, 0), (h, h, h, h), (-h, -h, -h, -h),
          (h, -h, h, -h), (0, 1, 0, 0)]
CLIP_FRAMES = (37, 61, 1, len(EDGE_Q) + 1, 9)
CLIP_DT = (1.0 / 30.0, 1.0 / 24.0, 1.0 / 30.0, 1.0 / 30.0, 1.0 / 20.0)

# (valid entries, flags, list order, -1 entries behind them, amp_ring)
CASES = [
    dict(n=1, flags=0, order="ascending"),
    dict(n=2, flags=RANDOM_HEADING, order="ascending"),
    dict(n=65, flags=0, order="scattered"),
    dict(n=65, flags=RANDOM_HEADING, order="scattered"),
    dict(n=65, flags=FIXED_LOCATION, order="ascending", pad=15),
    dict(n=65, flags=RANDOM_HEADING | FIXED_LOCATION, order="scattered", amp_ring=6),
    dict(n=257, flags=RANDOM_HEADING, order="scattered"),
    dict(n=257, flags=REAL_PATH | FIXED_LOCATION, order="ascending"),
]
OUT_KEYS = ("root_state", "dof_state", "rb_state", "contact_force", "warm_start", "traj_verts", "inverted", "progress", "reset", "terminate",
            "waypoint_traj", "init_pose", "init_vel", "amp", "motion_ids", "motion_times", "ground_h")


class World:
    """what every case shares: the models of the E envs, the motion cache, the map, the walkable samples, the real paths"""


@functools.lru_cache(maxsize=None)
def world():
    from emloco_amd.model import pack_models
    from helpers import varied_models
    w = World()
    w.models = pack_models(varied_models(E, seed=4))
    g = R._gen(7)
    nrm = lambda *s: torch.randn(*s, generator=g)
    F = sum(CLIP_FRAMES)
    unit = lambda q: q / q.norm(dim=-1, keepdim=True)
    start = np.concatenate([[0], np.cumsum(CLIP_FRAMES)[:-1]]).astype(np.int64)
    gts = nrm(F, NB, 3) * 0.5
    gts[:, :, 2] += 0.9
    grs, lrs = unit(nrm(F, NB, 4)), unit(nrm(F, NB, 4))
    s = int(start[CLIP_EDGE])
    eq = torch.tensor(EDGE_Q, dtype=F32)
    for f in range(CLIP_FRAMES[CLIP_EDGE]):
        for b in range(NB):
            lrs[s + f, b] = eq[(f + b) % len(EDGE_Q)]
            grs[s + f, b] = eq[(f + b) % len(EDGE_Q)]
    s = int(start[CLIP_NEAR])
    ang = 10.0 ** (-4.0 + 2.0 * torch.arange(NB - 1, dtype=F64) / (NB - 2))
    axis = unit(nrm(NB - 1, 3)).double()
    near = torch.cat([axis * torch.sin(ang / 2.0)[:, None], torch.cos(ang / 2.0)[:, None]], dim=1).float()
    lrs[s:s + CLIP_FRAMES[CLIP_NEAR], 1:] = near[None]
    dt = torch.tensor(CLIP_DT, dtype=F32)
    length = dt * torch.tensor([max(n - 1, 1) for n in CLIP_FRAMES], dtype=F32)
    w.cache = dict(gts=gts, grs=grs, lrs=lrs, gvs=nrm(F, NB, 3) * 1.5, gavs=nrm(F, NB, 3) * 3.0, dvs=nrm(F, NDOF) * 3.0, motion_len=length,
                   motion_dt=dt, motion_nframes=torch.tensor(CLIP_FRAMES, dtype=torch.int64), motion_start=torch.from_numpy(start))
    # a non-square map with a slope (83 x 61 cells of 0.1 m); walkable samples over it, the first ones within one probe of its border
    i, j = torch.arange(83)[:, None], torch.arange(61)[None, :]
    w.hf = (100 + 2 * i - j + torch.randint(-15, 16, (83, 61), generator=g)).to(torch.int16)
    vx, vy = 0.3 + torch.rand(N_VALID, generator=g) * 7.6, 0.3 + torch.rand(N_VALID, generator=g) * 5.4
    edge = torch.tensor([(0.05, 3.0), (8.15, 3.0), (4.0, 0.12), (4.0, 5.95), (0.08, 0.1), (8.12, 5.9), (0.02, 5.98), (8.19, 0.05)])
    vx[:8], vy[:8] = edge[:, 0], edge[:, 1]
    w.valid_x, w.valid_y = vx.float(), vy.float()
    w.betas = nrm(E, 17)
    # distinguishable real paths: row r is a straight walk whose z column is r
    k = torch.arange(NV, dtype=F32)
    w.real = torch.stack([0.01 * k[None, :].expand(N_REAL, NV), torch.zeros(N_REAL, NV), torch.arange(N_REAL, dtype=F32)[:, None].expand(N_REAL, NV)],
                         dim=-1).contiguous()
    return w


def cache_np():
    c = world().cache
    return {k: np.ascontiguousarray(v.numpy()) for k, v in c.items()}


def scalars(case):
    """the scalar fields of EmlocoResetBufs of a case"""
    vert_dt = 168 * DT / 100.0
    s = dict(flags=case["flags"], n_motions=len(CLIP_FRAMES), n_real=N_REAL if case["flags"] & REAL_PATH else 0, n_valid=N_VALID, n_dof_subset=57,
             hf_rows=83, hf_cols=61, fixed_x=FIXED_XY[0], fixed_y=FIXED_XY[1], dt=DT, height_tolerance=HEIGHT_TOL, vert_dt=vert_dt,
             dtheta_max=2.0, speed_min=0.0005, speed_max=3.0, accel_max=2.0, sharp_prob=0.02, hybrid_prob=0.0 if case["flags"] & REAL_PATH else 0.5,
             traj_dur=101 * vert_dt, sample_dt=0.4, hscale=HSCALE, vscale=VSCALE, real_pick_key=case["real_key"], amp_ring=case["amp_ring"])
    s.update(case.get("scalars", {}))                            # a case's own values (tests/chain_cases.py: hybrid_prob in the middle)
    return s


def const_of(case):
    """what a reset of `case` reads: the world's motion cache and real paths, with the arrays a case replaces (case["const"]: e.g. a clip
    whose root does not move, real paths with a short or an empty first segment) -> (cache dict, real [R][101][3])"""
    W = world()
    over = case.get("const", {})
    return {k: over.get(k, v) for k, v in W.cache.items()}, over.get("real_traj", W.real)


def initial(seed=11):
    """the state before a reset: garbage in the simulator's tensors, NaN / sentinels in what the reset writes, random AMP rows"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    nan = lambda *s: np.full(s, np.nan, np.float32)
    return dict(root_state=f(E, 13), dof_state=f(E, NDOF, 2), rb_state=f(E, NB, 13), contact_force=f(E, NB, 3), warm_start=f(E, MAXCAND * 3),
                traj_verts=nan(E, NV * 3), inverted=np.full(E, 7, np.uint8), progress=np.full(E, 55, np.int64), reset=np.ones(E, np.int64),
                terminate=np.ones(E, np.int64), waypoint_traj=nan(E, NS * 3), init_pose=nan(E, NB * 3), init_vel=nan(E, 2),
                amp=f(E, AMP_STEPS, AMP_ROW), motion_ids=np.full(E, -9, np.int64), motion_times=nan(E), ground_h=nan(E))


def make_case(spec, index):
    """ids [n + pad] (the valid entries first, -1 behind them) and the random rows [n + pad][512]: uniform draws with the entries that
    steer into the edges set by position in the list"""
    n, pad = spec["n"], spec.get("pad", 0)
    g = R._gen(100 + index)
    perm = torch.randperm(E, generator=g)[:n]
    if spec["order"] == "ascending":
        perm = perm.sort().values
    ids = np.concatenate([perm.numpy(), np.full(pad, -1)]).astype(np.int32)
    rnd = torch.rand(n + pad, RND, generator=g)
    c = world().cache
    M = len(CLIP_FRAMES)
    for bi in range(n):
        pm, pt, pl, py = (bi // 5) % 6, bi % 5, (bi // 3) % 7, (bi // 2) % 6
        if pm == 0:
            rnd[bi, RND_MOTION] = 0.0
        elif pm == 1:
            rnd[bi, RND_MOTION] = TOP
        elif pm == 2:                                            # just below a clip boundary: 1e-3 of an index below it
            rnd[bi, RND_MOTION] = (1 + bi % (M - 1) - 1e-3) / M
        mid = int(R.reset_pick(rnd[bi, RND_MOTION], M))
        nf, ln, dt = CLIP_FRAMES[mid], float(c["motion_len"][mid]), float(c["motion_dt"][mid])
        if pt == 0 and nf > 1:                                   # exactly on a frame
            rnd[bi, RND_TIME] = (bi % (nf - 1)) / (nf - 1)
        elif pt == 1:                                            # on the last frame
            rnd[bi, RND_TIME] = TOP
        elif pt == 2:                                            # within one control step of the clip's start: history rows at negative time
            rnd[bi, RND_TIME] = min(0.7 * DT / ln, 0.9) * (0.1 + 0.9 * float(rnd[bi, RND_TIME]))
        if pl == 0:
            rnd[bi, RND_LOC] = 0.0
        elif pl == 1:
            rnd[bi, RND_LOC] = TOP
        elif pl == 2:
            rnd[bi, RND_LOC] = (1 + bi % (N_VALID - 1) - 1e-3) / N_VALID
        elif pl == 3:                                            # a placement within one probe of the map border
            rnd[bi, RND_LOC] = (bi % 8 + 0.5) / N_VALID
        if py < 3:
            rnd[bi, RND_YAW] = (0.0, 0.5, TOP)[py]
    rnd[:, RND_REAL] = 0.5
    rnd[n:] = float("nan")                                       # rows behind the valid entries are not read
    return dict(spec=spec, name=f"n={n} flags={spec['flags']} {spec['order']}" + (f" pad={pad}" if pad else ""), n=n, ids=ids,
                rnd=np.ascontiguousarray(rnd.numpy()), flags=spec["flags"], amp_ring=spec.get("amp_ring", 0), real_key=0x1234ABCD + index)


def cases():
    return [make_case(s, i) for i, s in enumerate(CASES)]


def phys_row(ring, k):
    return (ring - 1 + k) % AMP_STEPS if ring else k             # EMLOCO_AMP_PHYS_ROW


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def pick_near(u, n):
    """u n within REL n of an integer 1 .. n - 1 (n itself is no branch: the pick is clamped to n - 1)"""
    x = torch.as_tensor(u).double() * n
    k = torch.round(x)
    return ((x - k).abs() < REL * n) & (k >= 1) & (k <= n - 1)


def slerp_near(q0, q1):
    c0, c1 = R.slerp_branch_distances(q0, q1)
    return ((c0 < REL) & (c0 != 0)) | (c1 < REL)


def sin_near(w):
    s = torch.sqrt(1.0 - w.double() ** 2)
    return (s - 1e-5).abs() < REL * 1e-5


def joint_near(c, st, history=False):
    """[rows][23] joints left out of a float comparison: the frame pair within the band of a slerp branch, or sin theta within the band
    of 1e-5; in a history row (whose joints go through exp_map_to_quat) also a rotation vector within the band of that function's 1e-5
    threshold.  judge(), judge_history() and near_shares() all take the mask from here."""
    near = slerp_near(c["lrs"][st["f0"]], c["lrs"][st["f1"]])[:, 1:] | sin_near(st["local_rot"][:, 1:, 3])
    if history:
        a = st["dof_pos"].reshape(-1, NB - 1, 3).norm(dim=-1)
        near = near | ((a - 1e-5).abs() < REL * 1e-5)
    return near


def on_frame(st):
    """rows whose time lies within rounding of a frame (blend weight within 1e-4 of an integer: float32 time carries about 1e-5 of a
    frame): there float32 and float64 may blend different frame pairs"""
    b = st["blend"].double()
    return (b - torch.round(b)).abs() < 1e-4


class Shares:
    """near-branch elements per family: (left out, all)"""

    def __init__(self):
        self.n = {}

    def add(self, family, mask):
        a, b = self.n.get(family, (0, 0))
        self.n[family] = (a + int(mask.sum()), b + mask.numel())

    def check(self):
        print()
        for k, (a, b) in sorted(self.n.items()):
            print(f"  [reset] near-branch share {k:<22} {a} of {b} = {a / max(b, 1):.4%}")
        bad = {k: v for k, v in self.n.items() if v[0] > CAP * v[1]}
        assert not bad, ("more than 1 % of a family's elements lie within the band of a branch: choose other seeds", bad)


def _masked(x, r, keep):
    """x where keep, the reference elsewhere (elements left out of a comparison)"""
    return torch.where(keep, torch.as_tensor(x).double(), r)


def _add(tab, case, name, got, f32, ref, keep=None):
    if keep is not None:
        if not keep.any():
            return
        got, f32 = _masked(got, ref, keep), _masked(f32, ref, keep)
        ref = torch.where(keep, ref, torch.zeros_like(ref))
        got, f32 = torch.where(keep, got, torch.zeros_like(ref)), torch.where(keep, f32, torch.zeros_like(ref))
    tab.add(case, name, R.err_max(got, ref), R.err_max(f32, ref))


def height_fix_error(pos, rot, m, gh, dtype):
    """the height fix applied to a state (dz = lowest point - ground - tolerance, every body lowered by dz) in `dtype`, then the float64
    distance of the result's lowest point above the ground to the tolerance, in metres"""
    pos = torch.as_tensor(pos).double()
    geo = (m["geom_type"], m["geom_a"], m["geom_b"], m["geom_r"])
    low = R.lowest_collision_point(pos, rot, *geo, dtype=dtype)
    tol, ghd = torch.tensor(HEIGHT_TOL, dtype=F32).to(dtype), torch.as_tensor(gh).to(dtype)
    dz = low - ghd - tol
    shifted = pos.clone()
    shifted[:, :, 2] = (pos[:, :, 2].to(dtype) - dz[:, None]).double()
    return R.lowest_collision_point(shifted, rot, *geo) - torch.as_tensor(gh).double() - float(np.float32(HEIGHT_TOL))


def judge(case, init, out, tab, fails, shares=None, history=True, check_unlisted=True, amp_row0=True):
    """every buffer of `out` after the reset of case against the references; figures into `tab`, exact mismatches into `fails`"""
    import oracle
    W = world()
    name, n, flags, ring = case["name"], case["n"], case["flags"], case["amp_ring"]
    shares = shares or Shares()
    env = torch.as_tensor(case["ids"][:n]).long()
    u = torch.as_tensor(case["rnd"][:n])
    T = lambda k: torch.as_tensor(np.ascontiguousarray(out[k]))
    fail = lambda *a: fails.append((name,) + a)
    M = len(CLIP_FRAMES)
    for k in OUT_KEYS:
        if out[k].shape != init[k].shape:
            fail(k, "shape", out[k].shape)
            return
    # ---- envs that are not listed: bit-identical in every buffer
    listed = np.zeros(E, bool)
    listed[env.numpy()] = True
    if check_unlisted:
        for k in OUT_KEYS:
            if not same_bits(out[k][~listed], init[k][~listed]):
                fail(k, "an env that is not listed changed")
    # ---- clip and start time
    mid = R.reset_pick(u[:, RND_MOTION], M)
    near_m = pick_near(u[:, RND_MOTION], M)
    shares.add("motion pick", near_m)
    ok = ~near_m
    got_mid = T("motion_ids")[env]
    if not torch.equal(got_mid[ok], mid[ok]):
        fail("motion_ids", (got_mid != mid).nonzero().reshape(-1)[:8].tolist())
    c, real_tab = const_of(case)
    t64 = u[:, RND_TIME].double() * c["motion_len"][mid].double()
    t32 = u[:, RND_TIME] * c["motion_len"][mid]
    got_t = T("motion_times")[env].double()
    if not bool(((got_t - t64).abs() <= 2.0 ** -24 * t64)[ok].all()):
        fail("motion_times beyond one rounding of u len", float(((got_t - t64).abs() / t64.clamp_min(1e-30))[ok].max()))
    # ---- placement
    if flags & FIXED_LOCATION:
        place = torch.tensor(FIXED_XY, dtype=F32)[None, :].expand(n, 2)
    else:
        li = R.reset_pick(u[:, RND_LOC], N_VALID)
        near_l = pick_near(u[:, RND_LOC], N_VALID)
        shares.add("location pick", near_l)
        ok = ok & ~near_l
        place = torch.stack([W.valid_x[li], W.valid_y[li]], dim=1)
    root = T("root_state")[env]
    if not same_bits(root[ok][:, :2].numpy(), place[ok].contiguous().numpy()):
        fail("root xy is not the placement")
    # ---- joints: motion_state in float64 and float32
    st, s32 = R.motion_state(c, mid, t64), R.motion_state(c, mid, t32, dtype=F32)
    okj = ok[:, None].expand(n, NB - 1)
    w = st["local_rot"][:, 1:, 3]
    near_j = joint_near(c, st)
    shares.add("joint slerp / sin", near_j)
    keep = okj & ~near_j
    half_turn, near_id = w.abs() < 1e-5, w.abs() > 1.0 - 1e-3
    dof = T("dof_state")[env]
    gp, fp, rp = dof[:, :, 0].reshape(n, NB - 1, 3).double(), s32["dof_pos"].reshape(n, NB - 1, 3).double(), st["dof_pos"].reshape(n, NB - 1, 3)
    # a joint at 180 degrees (|w| < 1e-5, the only elements of the "180" name): +pi axis and -pi axis are one rotation, and the float32
    # evaluation itself lands on either (2 acosf(0) wraps to -pi, 2 acos(0) to +pi), so these elements are compared up to that sign;
    # compared strictly the float32 column is 2.0 and its bar means nothing
    sign = lambda x: torch.where((x * rp).sum(-1, keepdim=True) < 0, -x, x)
    x3 = lambda m: m[:, :, None].expand(n, NB - 1, 3)
    _add(tab, name, "dof_pos", gp, fp, rp, x3(keep & ~half_turn & ~near_id))
    _add(tab, name, "dof_pos near-identity", gp, fp, rp, x3(keep & near_id))
    _add(tab, name, "dof_pos 180", sign(gp), sign(fp), rp, x3(keep & half_turn))
    _add(tab, name, "dof_vel", dof[:, :, 1], s32["dof_vel"], st["dof_vel"], ok[:, None].expand(n, NDOF))
    # ---- root: turn, forward speed
    rh = bool(flags & RANDOM_HEADING)
    _, rot, vel, ang = R.reset_root(st, u[:, RND_YAW], u[:, RND_SPEED], rh, place)
    _, rot32, vel32, ang32 = R.reset_root(s32, u[:, RND_YAW], u[:, RND_SPEED], rh, place, dtype=F32)
    near_r = slerp_near(c["grs"][st["f0"], 0], c["grs"][st["f1"], 0])
    shares.add("root slerp", near_r)
    okr = ok & ~near_r
    # q and -q are one rotation, and which of them a blend returns follows the frame pair: at a time within rounding of a frame, float32
    # may blend (f, f + 1) at 0 where float64 blends (f - 1, f) at 1 - eps -- the same rotation, with the sign of another neighbour (compared
    # strictly the float32 column itself is 1.7 there).  Only those rows are compared up to the sign; everywhere else the sign is pinned.
    frame = on_frame(st)[:, None]
    qsign = lambda x: torch.where(frame & ((x.double() * rot).sum(-1, keepdim=True) < 0), -x.double(), x.double())
    _add(tab, name, "root rot", qsign(root[:, 3:7]), qsign(rot32), rot, okr[:, None].expand(n, 4))
    _add(tab, name, "root vel", root[:, 7:10], vel32, vel, (okr if rh else ok)[:, None].expand(n, 3))
    _add(tab, name, "root ang_vel", root[:, 10:13], ang32, ang, ok[:, None].expand(n, 3))
    # ---- ground height: the fp32 oracle's centre probes of the pose the kernel wrote, averaged in torch's order
    c9 = oracle.get_center_heights(np.ascontiguousarray(root.numpy()), W.hf.numpy(), HSCALE, VSCALE)
    s9 = c9[:, 0] + c9[:, 8]
    for k in range(1, 8):
        s9 = s9 + c9[:, k]
    gh = (s9 / np.float32(9.0)).astype(np.float32)
    if not same_bits(out["ground_h"][env.numpy()], gh):
        fail("ground_h differs from the oracle's centre height", int((_bits(out["ground_h"][env.numpy()]) != _bits(gh)).sum()))
    # ---- kinematics of the written root and joints; the lowest collision point sits height_tolerance above the ground
    m = {k: (torch.as_tensor(v[env.numpy()]) if v.ndim > 1 else v) for k, v in W.models.items()}
    rb = T("rb_state")[env]
    if not same_bits(rb[:, 0, :3].contiguous().numpy(), root[:, :3].contiguous().numpy()):
        fail("the root body is not at the root position")
    pos, qw = R.forward_kinematics(root, dof[:, :, 0], m["parent"], m["joint_off"])
    pos32, qw32 = R.forward_kinematics(root, dof[:, :, 0], m["parent"], m["joint_off"], dtype=F32)
    rel = lambda p: p.double() - root[:, None, :3].double()
    _add(tab, name, "fk position", rel(rb[:, :, :3]), rel(pos32), rel(pos))
    _add(tab, name, "fk rotation", rb[:, :, 3:7], qw32, qw)
    zerr = lambda dtype: height_fix_error(rb[:, :, :3], rb[:, :, 3:7], m, gh, dtype).abs().max().item()
    low = R.lowest_collision_point(rb[:, :, :3], rb[:, :, 3:7], m["geom_type"], m["geom_a"], m["geom_b"], m["geom_r"])
    tab.add(name, "height fix [m]", (low - torch.as_tensor(gh).double() - float(np.float32(HEIGHT_TOL))).abs().max().item(), zerr(F32))
    # ---- copies, flags, zeros
    if not same_bits(out["init_pose"][env.numpy()], rb[:, :, :3].reshape(n, -1).contiguous().numpy()):
        fail("init_pose is not the body positions")
    if not same_bits(out["init_vel"][env.numpy()], root[:, 7:9].contiguous().numpy()):
        fail("init_vel is not the root velocity")
    for k in ("progress", "reset", "terminate"):
        if (out[k][env.numpy()] != 0).any():
            fail(k, "not 0")
    for k in ("contact_force", "warm_start"):
        if (_bits(out[k][env.numpy()]) != 0).any():
            fail(k, "not exactly +0")
    # ---- trajectory: out of scope, but written; a real path is the row the permutation picks
    for k in ("traj_verts", "waypoint_traj"):
        if not np.isfinite(out[k][env.numpy()]).all():
            fail(k, "not written")
    sc = scalars(case)
    rows = np.array([R.real_pick_perm(bi % N_REAL, N_REAL, case["real_key"]) for bi in range(n)], np.int64)
    if case.get("real_pick") is not None:                        # explicit rows (supplied random rows only), clamped into the table
        rows = np.clip(np.asarray(case["real_pick"][:n], np.int64), 0, N_REAL - 1)
    if flags & REAL_PATH:
        z = out["traj_verts"][env.numpy()].reshape(n, NV, 3)[:, :, 2]
        is_real = (u[:, RND_REAL] > torch.tensor(sc["hybrid_prob"], dtype=F32)).numpy() & (sc["n_real"] > 0)
        want = np.where(is_real, rows, 0).astype(np.float32)    # a generated path lies in the plane z = 0
        if not np.array_equal(z, np.repeat(want[:, None], NV, 1)):
            fail("real-path rows are not the permutation's", int((z[:, 0] != want).sum()))
        if case.get("real_pick") is None and n <= N_REAL and len(set(z[is_real, 0].tolist())) != int(is_real.sum()):
            fail("real-path rows are not distinct")
    if case.get("traj"):
        judge_traj(case, init, out, tab, fails, env, u, root, rows, real_tab, sc)
    # ---- AMP history rows 1..14; row 0 untouched
    amp, amp0 = out["amp"][env.numpy()], init["amp"][env.numpy()]
    if amp_row0 and not same_bits(amp[:, phys_row(ring, 0)], amp0[:, phys_row(ring, 0)]):
        fail("AMP row 0 changed")
    if history:
        judge_history(case, out, tab, fails, shares)
    elif amp_row0 and not same_bits(amp, amp0):
        fail("AMP rows changed without the history back-fill")
    elif not amp_row0:
        hist = [phys_row(ring, k) for k in range(1, AMP_STEPS)]
        if not same_bits(amp[:, hist], amp0[:, hist]):
            fail("AMP history rows changed without the history back-fill")
    return shares


def judge_traj(case, init, out, tab, fails, env, u, root, rows, real_tab, sc):
    """traj_verts, waypoint_traj and inverted of the listed envs against R.reset_trajectory in float64 (from the root position and
    velocity the reset wrote, as the kinematics are judged from the written joints); vertices relative to the start"""
    name, n, flags = case["name"], case["n"], case["flags"]
    fail = lambda *a: fails.append((name,) + a)
    ip, rv = root[:, :2], root[:, 7:10]
    use_real = real_tab if sc["n_real"] > 0 else None
    ref, inv, _ = R.reset_trajectory(u, ip, rv, sc, flags, use_real, rows)
    r32, _, _ = R.reset_trajectory(u, ip, rv, sc, flags, use_real, rows, dtype=F32)
    got = torch.as_tensor(out["traj_verts"][env.numpy()]).reshape(n, NV, 3)
    rel = lambda v: torch.cat([v[:, :, :2].double() - ip[:, None, :].double(), v[:, :, 2:].double()], dim=-1)
    _add(tab, name, "trajectory", rel(got), rel(r32), rel(ref))
    t = torch.arange(NS, dtype=F32)[None, :].expand(n, NS) * torch.tensor(sc["sample_dt"], dtype=F32)
    dur = float(np.float32(sc["traj_dur"]))
    w64, w32 = R.traj_calc_pos(got, t, dur), R.traj_calc_pos(got, t, dur, dtype=F32)
    relw = lambda v: v.double().reshape(n, NS, 3) - torch.cat([ip.double(), torch.zeros(n, 1, dtype=F64)], dim=1)[:, None, :]
    _add(tab, name, "waypoints", relw(torch.as_tensor(out["waypoint_traj"][env.numpy()])), relw(w32), relw(w64))
    if (flags & INIT_HEADING) and (flags & HEADING_INVERSION):
        if not np.array_equal(out["inverted"][env.numpy()], inv.numpy().astype(np.uint8)):
            fail("inverted is not (u > 0.5)")
    elif not np.array_equal(out["inverted"][env.numpy()], init["inverted"][env.numpy()]):
        fail("inverted written without INIT_HEADING | HEADING_INVERSION")


def judge_history(case, out, tab, fails, shares):
    """rows 1..14 of the listed envs: R.amp_row of motion_state at (the time the reset wrote) - k dt, block by block"""
    W = world()
    name, n, ring = case["name"], case["n"], case["amp_ring"]
    env = torch.as_tensor(case["ids"][:n]).long()
    c, _ = const_of(case)
    K = AMP_STEPS - 1
    mid = torch.as_tensor(out["motion_ids"])[env].repeat_interleave(K)
    mt = torch.as_tensor(out["motion_times"])[env].repeat_interleave(K)
    k = torch.arange(1, K + 1).repeat(n)
    dt32 = torch.tensor(DT, dtype=F32)
    t64, t32 = mt.double() - dt32.double() * k.double(), mt - dt32 * k.float()
    st, s32 = R.motion_state(c, mid, t64), R.motion_state(c, mid, t32, dtype=F32)
    betas = W.betas[env].repeat_interleave(K, dim=0)
    args = lambda s: {a: s[a] for a in ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "key_pos")}
    ref, r32 = R.amp_row(**args(st), betas=betas), R.amp_row(**args(s32), betas=betas, dtype=F32)
    rows = np.stack([out["amp"][env.numpy()][:, phys_row(ring, kk)] for kk in range(1, K + 1)], axis=1).reshape(n * K, AMP_ROW)
    got = torch.as_tensor(rows)
    near_r = slerp_near(c["grs"][st["f0"], 0], c["grs"][st["f1"], 0])
    shares.add("history root slerp", near_r)
    sub_j = sorted({d // 3 for d in R.DOF_SUBSET})
    near_j = joint_near(c, st, history=True)
    shares.add("history joint slerp / sin", near_j)
    near_j = near_j[:, sub_j]                 # (joints at 180 degrees are judged: tangent | normal does not see the +-pi wrap)
    for bname, lo, hi in R.amp_blocks(57):
        wd = hi - lo
        if bname == "dof_pos":
            keep = ~near_j.repeat_interleave(6, dim=1)
        elif bname == "dof_vel":
            keep = torch.ones(n * K, wd, dtype=torch.bool)
        else:
            keep = ~near_r[:, None].expand(n * K, wd)
        _add(tab, name, "history " + bname, got[:, lo:hi], r32[:, lo:hi], ref[:, lo:hi], keep)
    if not torch.equal(got[:, AMP_ROW - 11:].double(), ref[:, AMP_ROW - 11:]):
        fails.append((name, "history betas are not copies"))


def judge_rnd(ids, n, seed, ws, ws0, fails):
    """the random workspace after a seeded call: rows of present entries are reset_rnd_row bit for bit and lie in [0, 1); rows behind the
    first -1 (and behind n) are as they were"""
    present = 0
    while present < n and ids[present] >= 0:
        present += 1
    for bi in range(present):
        if not same_bits(ws[bi], R.reset_rnd_row(seed, bi).numpy()):
            fails.append(("random row", bi, "differs from the hash of (seed, row, entry)"))
            break
    if present and not ((ws[:present] >= 0).all() and (ws[:present] < 1).all()):
        fails.append(("random rows outside [0, 1)",))
    if not same_bits(ws[present:], ws0[present:]):
        fails.append(("a random row behind the last present entry was written",))


def near_shares():
    """the near-branch shares of every case from the references alone (no kernel output): what judge() would leave out"""
    W = world()
    c = W.cache
    sh = Shares()
    M = len(CLIP_FRAMES)
    for case in cases():
        n = case["n"]
        u = torch.as_tensor(case["rnd"][:n])
        sh.add("motion pick", pick_near(u[:, RND_MOTION], M))
        if not case["flags"] & FIXED_LOCATION:
            sh.add("location pick", pick_near(u[:, RND_LOC], N_VALID))
        mid = R.reset_pick(u[:, RND_MOTION], M)
        t0 = u[:, RND_TIME].double() * c["motion_len"][mid].double()
        K = AMP_STEPS - 1
        for fam, mids, ts in (("", mid, t0), ("history ", mid.repeat_interleave(K),
                                               t0.repeat_interleave(K) - float(np.float32(DT)) * torch.arange(1, K + 1).repeat(n).double())):
            st = R.motion_state(c, mids, ts)
            sh.add(fam + "root slerp", slerp_near(c["grs"][st["f0"], 0], c["grs"][st["f1"], 0]))
            sh.add(fam + "joint slerp / sin", joint_near(c, st, history=bool(fam)))
    return sh

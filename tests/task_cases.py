"""Case tables and judges of the task-kernel conformance matrix (include/emloco_task.h), shared by the emulator run on the CPU
(tests/test_kernel_refs_cpu.py) and the device run (tests/test_gpu_task_matrix.py): the two differ in the executor only.

An executor is an object with
    pd_targets(actions, offset, scale, zero_mask) -> [n][69]
    amp_rows(state dict of amp_inputs, subset) -> [n][206]
    post_physics(case, heightfield, mode, amp0) -> dict(obs, flip_obs, rew, reward_raw, amp, progress, reset, terminate)
    heights(heightfield, pose7, grid) -> heights, px, py
    compact(flags) -> ids [n + 1]
taking and returning CPU arrays.  The judges compare what it returns with the float64 references of tests/kernel_refs.py (float
outputs, through a kernel_refs.Table: bar = MARGIN x the float32 evaluation's own error) and with the fp32 oracle (oracle.*: height
observations, map indices, flags and progress, bit for bit).
"""
import numpy as np
import torch

import kernel_refs as R

F32, F64 = torch.float32, torch.float64
ULP4 = 2.0 ** -22                                  # single-rounding element-wise results

POST_ADVANCE, POST_OBS, POST_REWARD, POST_RESET, POST_AMP_SHIFT, POST_AMP_ROW, POST_STEP = 1, 2, 4, 8, 16, 32, 63
POST_SKIP_DONE, POST_AMP_DONE_ONLY = 64, 128

PD_SIZES = [1, 3, 4, 371, 4097]                     # 256 threads = 3.7 envs: the block edge lies between 3 and 4 envs
AMP_CASES = [(1, 11), (2, 12), (65, 13), (300, 14)]          # (rows, seed of case_task)
POST_CASES = [(1, 21), (63, 26), (65, 23), (257, 24)]        # (envs, seed of case_task)
ALGEBRA_CASE = (65, 23)                                      # the state of the mode-algebra, ring and indexed-launch tests
COMPACT_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 4096, 16897]
COMPACT_PATTERNS = ["none", "all", "first", "last", "3%", "50%"]
FLAG_VALUES = (1, -1, 2, 1 << 40)                            # a set flag is any non-zero int64: the low word of 1 << 40 is 0


def case_pd(n, seed):
    g = R._gen(seed)
    mask = torch.zeros(69, dtype=torch.uint8)
    for j in (3, 7, 17, 22):                                 # toes and hands, as shipped; plus one lone entry
        mask[3 * j:3 * j + 3] = 1
    mask[40] = 1
    scale = torch.full((69,), float(np.pi))
    scale[[4, 16]] = 5.0
    return dict(actions=torch.randn(n, 69, generator=g) * 1.5, offset=torch.randn(69, generator=g) * 0.3,
                scale=scale * (1.0 + 0.1 * torch.randn(69, generator=g)), zero_mask=mask)


def judge_pd(c, got):
    """masked targets exactly 0; the others within one fused or unfused rounding of float64: 2^-22 of |offset| + |scale a|"""
    got = torch.as_tensor(got).double()
    ref = R.pd_targets(c["actions"], c["offset"], c["scale"], c["zero_mask"])
    m = c["zero_mask"] != 0
    assert torch.isfinite(got).all(), "a target was not written"
    assert (got[:, m] == 0).all() and not torch.signbit(got[:, m]).any(), "a masked target is not exactly +0"
    err = ((got - ref).abs() / R.pd_targets_mag(c["actions"], c["offset"], c["scale"]).clamp_min(1e-300))[:, ~m].max().item()
    assert err <= ULP4, ("pd_targets beyond 2^-22 of |offset| + |scale a|", err)
    return err


def amp_inputs(c):
    """the explicit-state arguments of emloco_task_amp_rows taken from a case_task state"""
    rb = c["rb_state"]
    return dict(root_pos=rb[:, 0, 0:3].contiguous(), root_rot=rb[:, 0, 3:7].contiguous(), root_vel=rb[:, 0, 7:10].contiguous(),
                root_ang_vel=rb[:, 0, 10:13].contiguous(), dof_pos=c["dof_state"][:, :, 0].contiguous(),
                dof_vel=c["dof_state"][:, :, 1].contiguous(), key_pos=rb[:, list(R.KEY_BODIES), 0:3].contiguous(), betas=c["betas"])


def joint_band(c, subset):
    """[n][n_sub / 3] bool: joints whose rotation vector sits within 1e-5 (relative) of a branch of exp_map_to_quat"""
    sub = torch.as_tensor(subset).long()
    a = c["dof_state"][:, :, 0].double()[:, sub].reshape(c["dof_state"].shape[0], -1, 3).norm(dim=-1)
    return ((a - 1e-5).abs() < 1e-5 * 1e-5) | ((a - np.pi).abs() < 1e-5 * np.pi)


def judge_amp_row(case, c, subset, got, tab, fails):
    """one AMP row per env against float64, block by block; dof velocities and betas are copies (exact)"""
    a = amp_inputs(c)
    n_sub = len(subset)
    ref = R.amp_row(**a, dof_subset=subset)
    r32 = R.amp_row(**a, dof_subset=subset, dtype=F32)
    got = torch.as_tensor(got)
    width = 35 + 3 * n_sub
    band = joint_band(c, subset).repeat_interleave(6, dim=1)
    for name, lo, hi in R.amp_blocks(n_sub):
        g, f, r = got[:, lo:hi].double(), r32[:, lo:hi].double(), ref[:, lo:hi]
        if name == "dof_vel":
            if not torch.equal(g, r):
                fails.append((case, "AMP dof velocities are not copies"))
            continue
        if name == "dof_pos":                                # joints inside the branch band are left out
            g, f = torch.where(band, r, g), torch.where(band, r, f)
        tab.add(case, "amp " + name, R.err_max(g, r), R.err_max(f, r))
    if not torch.equal(got[:, width - 11:width].double(), ref[:, width - 11:width]):
        fails.append((case, "AMP betas are not copies"))


def post_reference(c, advance, dtype=F64):
    """every float output of one post-physics launch on a case_task state, in the dtype given"""
    rb = c["rb_state"]
    prog = c["progress"] + (1 if advance else 0)
    dur = float(np.float32(c["traj_dur"]))
    samples = R.traj_calc_pos(c["traj_verts"], R.traj_sample_times(prog, c["dt"], c["sample_dt"], dtype=dtype), dur, dtype=dtype)
    body = (rb[:, :, 0:3], rb[:, :, 3:7], rb[:, :, 7:10], rb[:, :, 10:13])
    rew, loc, power, terms = R.reward(rb[:, 0, 0:3], samples[:, 0], c["dof_force"], c["dof_state"][:, :, 1], c["power_coef"], dtype=dtype)
    return dict(self_obs=R.self_obs(*body, c["betas"], dtype=dtype), flip_self_obs=R.flip_self_obs(*body, c["betas"], dtype=dtype),
                loc_obs=R.location_obs(rb[:, 0], samples, dtype=dtype), rew=rew, loc_reward=loc, power_reward=power, power_terms=terms,
                amp_row=R.amp_row(**amp_inputs(c), dtype=dtype), target=samples[:, 0], progress=prog)


def oracle_post(c, hf, advance):
    """what the fp32 oracle defines bit for bit: height observations (and their mirror), flags, progress"""
    import oracle
    rb = c["rb_state"].numpy()
    prog = c["progress"].numpy() + (1 if advance else 0)
    hf = np.ascontiguousarray(hf.numpy() if isinstance(hf, torch.Tensor) else hf)
    root = np.ascontiguousarray(rb[:, 0])
    head = np.ascontiguousarray(rb[:, R.HEAD_BODY, :7])
    center = oracle.get_center_heights(root, hf)
    heights = oracle.get_heights(head, hf)
    tar = oracle.traj_calc_pos(c["traj_verts"].numpy(), prog, c["dt"], c["traj_dur"])
    rs, tm = oracle.reset(prog, c["contact_force"].numpy(), rb[:, :, :3], tar, R.CONTACT_BODIES, c["max_episode_length"], c["fail_dist"])
    return dict(height_obs=oracle.height_obs(center, heights), center=center, heights=heights, reset=rs, terminate=tm, progress=prog)


def judge_post(case, c, hf, mode, amp0, out, tab, fails):
    """a launch with every compute bit set (POST_STEP, with or without ADVANCE) against float64 and the oracle"""
    import oracle
    advance = bool(mode & POST_ADVANCE)
    ref, r32, orc = post_reference(c, advance), post_reference(c, advance, dtype=F32), oracle_post(c, hf, advance)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    obs, fobs = T(out["obs"]), T(out["flip_obs"])
    for name, got in (("self_obs", obs[:, :368]), ("flip_self_obs", fobs[:, :368]), ("loc_obs", obs[:, 368:398]), ("rew", T(out["rew"])),
                      ("loc_reward", T(out["reward_raw"])[:, 0])):
        tab.add(case, name, R.err_max(got, ref[name]), R.err_max(r32[name], ref[name]))
    tab.add(case, "power_reward", R.err_terms(T(out["reward_raw"])[:, 1], ref["power_reward"], ref["power_terms"]),
            R.err_terms(r32["power_reward"], ref["power_reward"], ref["power_terms"]))
    amp = T(out["amp"])
    fa = []
    judge_amp_row(case, c, R.DOF_SUBSET, amp[:, 0], tab, fa)
    fails += fa
    if not torch.equal(amp[:, 1:], T(amp0)[:, :-1]):
        fails.append((case, "the AMP history shift is not a pure copy of rows 0..13 to 1..14"))
    # index and threshold arithmetic: the fp32 oracle, bit for bit
    if not np.array_equal(out["obs"][:, 398:], orc["height_obs"]):
        fails.append((case, "height observations differ from the oracle", int((out["obs"][:, 398:] != orc["height_obs"]).sum())))
    if not np.array_equal(out["flip_obs"][:, 368:], oracle.flip_task_obs(np.ascontiguousarray(out["obs"][:, 368:]))):
        fails.append((case, "the mirrored task observations are not the flip of the task observations"))
    for name in ("reset", "terminate", "progress"):
        if not np.array_equal(out[name], orc[name]):
            fails.append((case, name + " differs from the oracle", np.nonzero(out[name] != orc[name])[0][:8].tolist()))
    # ... and float64 agrees wherever an env is not within 1e-5 of a threshold
    rs, tm, dist = R.reset_flags(ref["progress"], c["contact_force"], c["contact_body_mask"], c["rb_state"][:, 0, :3], ref["target"],
                                 c["fail_dist"], c["max_episode_length"])
    far = ~R.reset_near(dist, c["fail_dist"])
    if not (torch.equal(T(out["reset"])[far], rs[far]) and torch.equal(T(out["terminate"])[far], tm[far])):
        fails.append((case, "reset / terminate differ from float64 away from every threshold"))


def judge_heights(case, hf, pose7, grid, got, fails):
    """emloco_task_get_heights: heights and int64 map indices against the oracle, bit for bit"""
    import oracle
    hf = np.ascontiguousarray(hf)
    pose7 = np.ascontiguousarray(pose7, np.float32)
    if grid:
        h, px, py = oracle.get_heights(pose7, hf, return_index=True)
    else:
        root = np.zeros((pose7.shape[0], 13), np.float32)
        root[:, :7] = pose7
        h, px, py = oracle.get_center_heights(root, hf, return_index=True)
    for name, a, b in (("heights", got[0], h), ("px", got[1], px), ("py", got[2], py)):
        if not np.array_equal(a, b):
            fails.append((case, f"get_heights(grid={grid}) {name} differs from the oracle", int((a != b).sum())))
    return px, py


def compact_flags_case(n, pattern, seed=0):
    g = R._gen(1000 * n + seed)
    vals = torch.tensor(FLAG_VALUES)[torch.randint(0, len(FLAG_VALUES), (n,), generator=g)]
    if pattern == "none":
        on = torch.zeros(n, dtype=torch.bool)
    elif pattern == "all":
        on = torch.ones(n, dtype=torch.bool)
    elif pattern in ("first", "last"):
        on = torch.zeros(n, dtype=torch.bool)
        on[0 if pattern == "first" else n - 1] = True
    else:
        on = torch.rand(n, generator=g) < (0.03 if pattern == "3%" else 0.5)
    return torch.where(on, vals, torch.zeros_like(vals))


def judge_compact(flags, ids):
    """ids[0..count) ascending = flags.nonzero(), ids[count..n) = -1, ids[n] = count"""
    n = flags.numel()
    ids = torch.as_tensor(ids).long()
    nz = torch.nonzero(flags).reshape(-1)
    assert ids[n].item() == nz.numel(), ("count", ids[n].item(), nz.numel())
    assert torch.equal(ids[:nz.numel()], nz), "ids are not flags.nonzero()"
    assert (ids[nz.numel():n] == -1).all(), "padding is not -1"

"""GPU: the motion library's device build -- emloco_motion_build against the reference's loader fixture and the float64 host build,
`MotionLib.load_motions(build="device")` against the host build, and `resample_motions()` inside the task with the resets that follow."""
import faulthandler

import numpy as np
import pytest

import motion_build_cases as cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEY_BODIES = [7, 3, 22, 17]
POSE_TOL = dict(rtol=1e-4, atol=2e-5)                    # tests/test_gpu_env.py, test_fused_reset_matches_host_mirror


@pytest.fixture(autouse=True)
def _own_time_limit():
    """every test here runs under a time limit of its own: a launch that never returns ends the process instead of holding the device"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _device_build(case, grid=0):
    from emloco_amd import _lib as L
    lib = L.require_device()
    dev = torch.device("cuda:0")
    up = lambda k: torch.from_numpy(case[k]).to(dev)
    d = {k: up(k) for k in ("quat_global", "root_trans", "frame_start", "n_frames", "fps", "skel_id", "local_translation")}
    out = {k: torch.full(v.shape, float("nan"), device=dev) for k, v in cases.empty_outputs(case).items()}
    rc = lib.emloco_motion_build(case["n_clips"], case["n_skel"], case["F"], d["quat_global"].data_ptr(), d["root_trans"].data_ptr(),
                                 d["frame_start"].data_ptr(), d["n_frames"].data_ptr(), d["fps"].data_ptr(), d["skel_id"].data_ptr(),
                                 case["frame_start"].ctypes.data, case["n_frames"].ctypes.data, case["skel_id"].ctypes.data,
                                 d["local_translation"].data_ptr(), case["parent"].ctypes.data, case["taps"].ctypes.data,
                                 *[out[k].data_ptr() for k in cases.KEYS], grid, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def edge_out():
    rc, out = _device_build(cases.edge_case())
    assert rc == 0
    return out


def test_fixture_clips_match_the_reference_loader():
    rc, out = _device_build(cases.fixture_case())
    assert rc == 0
    cases.assert_fixture(out, "device")
    cases.assert_bar(cases.fixture_case(), out, "device, fixture clips")


def test_edge_matrix_against_the_float64_host_build(edge_out):
    case = cases.edge_case()
    cases.assert_bar(case, edge_out, "device, edge matrix")
    c = list(case["n_frames"]).index(33)
    s = int(case["frame_start"][c])
    assert np.all(edge_out["dvs"][s + 10:s + 15] == 0.0)             # identical frames: exactly zero, no NaN


def test_result_does_not_depend_on_the_grid(edge_out):
    case = cases.edge_case()
    for grid in (1, 7):
        rc, out = _device_build(case, grid=grid)
        assert rc == 0
        for k in cases.KEYS:
            assert np.array_equal(out[k].view(np.uint32), edge_out[k].view(np.uint32)), (grid, k)


def test_bad_arguments_launch_nothing():
    case = dict(cases.fixture_case())
    case["n_frames"] = np.asarray([45, 1], np.int32)
    rc, out = _device_build(case)
    assert rc == -1 and all(np.isnan(v).all() for v in out.values())
    case = dict(cases.fixture_case())
    case["skel_id"] = np.asarray([0, 3], np.int32)
    rc, out = _device_build(case)
    assert rc == -1 and all(np.isnan(v).all() for v in out.values())


# ------------------------------------------------------------------ MotionLib
LENGTHS = (40, 64, 200)                                 # the generated clips; the fixture's have 45 and 38 frames


@pytest.fixture(scope="module")
def pickle5(tmp_path_factory):
    """a 5-clip pickle in the reference's format: the two fixture clips and three generated ones"""
    import joblib
    clips = {f"clip{i}": c for i, c in enumerate(cases.fixture_clips())}
    for i, T in enumerate(LENGTHS):
        clips[f"walk{i}"] = cases.random_clip(T, (60, 30, 30)[i], 500 + i)
    path = str(tmp_path_factory.mktemp("motion") / "amass_isaac_five.pkl")
    joblib.dump(clips, path)
    return path, clips


def _skeletons(n=8):
    lt = cases.golden()["local_translation"].astype(np.float64)
    return [(lt * (0.9, 1.0, 1.1)[j % 3], cases.PARENT) for j in range(n)]


def _case_of(lib, clips, skeletons):
    """the library's current draw as a kernel case: the bars and the float64 reference of exactly these (clip, skeleton) pairs"""
    drawn = [list(clips.values())[i] for i in lib._curr_motion_ids.tolist()]
    table, ids = [], []
    for lt, _ in skeletons:
        key = [t.tobytes() for t in table]
        if lt.tobytes() not in key:
            table.append(lt)
        ids.append([t.tobytes() for t in table].index(lt.tobytes()))
    return cases.pack(drawn, table, ids)


def _arrays(lib):
    return {k: getattr(lib, k).cpu().numpy() for k in cases.KEYS}


def test_load_motions_device_against_host(pickle5):
    from emloco_amd.utils.motion_lib_smpl import MotionLib
    path, clips = pickle5
    skels, betas = _skeletons(), torch.arange(8 * 17, dtype=torch.float32).reshape(8, 17) / 100
    libs = {}
    for mode in ("host", "device"):
        lib = libs[mode] = MotionLib(path, key_body_ids=KEY_BODIES, device="cuda:0", build=mode)
        torch.manual_seed(21)
        assert lib.load_motions(skels, gender_betas=betas, limb_weights=None, random_sample=True) is lib
    h, d = libs["host"], libs["device"]
    torch.cuda.synchronize()
    assert len(set(d._curr_motion_ids.tolist())) >= 3
    for k in ("_curr_motion_ids", "length_starts", "_motion_num_frames", "_motion_lengths", "_motion_dt", "_motion_aa", "_motion_fps",
              "_motion_bodies", "_motion_limb_weights", "_motion_weights", "motion_ids"):
        a, b = getattr(h, k), getattr(d, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(a, b), k
    assert d.num_motions() == 8 and d.num_reallocations == 0
    for k in cases.KEYS:
        assert getattr(h, k).shape == getattr(d, k).shape and getattr(d, k).is_contiguous(), k
    case = _case_of(d, clips, skels)
    ref = cases.reference(case)
    for k in cases.KEYS:                                             # the host build is the float64 reference, cast
        assert np.array_equal(_arrays(h)[k], ref[k].astype(np.float32).reshape(_arrays(h)[k].shape)), k
    cases.assert_bar(case, _arrays(d), "load_motions(device)")
    ids = torch.tensor([0, 3, 5, 7], device="cuda:0")
    times = torch.tensor([0.0, 0.21, 0.5, 0.35], device="cuda:0")
    assert bool((times < d._motion_lengths[ids]).all())
    rh, rd = h.get_motion_state_smpl(ids, times), d.get_motion_state_smpl(ids, times)
    for k in ("root_pos", "rg_pos", "key_pos"):                      # the tolerances of tests/test_motion_lib_cpu.py:55-60
        np.testing.assert_allclose(rd[k].cpu().numpy(), rh[k].cpu().numpy(), rtol=0, atol=2e-4, err_msg=k)
    np.testing.assert_allclose(rd["dof_vel"].cpu().numpy(), rh["dof_vel"].cpu().numpy(), rtol=0, atol=2e-2)
    q, qr = rd["root_rot"].cpu().numpy(), rh["root_rot"].cpu().numpy()
    assert np.minimum(np.abs(q - qr).max(-1), np.abs(q + qr).max(-1)).max() < 1e-4
    assert torch.equal(rd["motion_aa"], rh["motion_aa"]) and torch.equal(rd["motion_bodies"], rh["motion_bodies"])


# ------------------------------------------------------------------ the task
def _make_env(num_envs, extra):
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    args = get_args(["--num_envs", str(num_envs), "--seed", "3", *extra])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    return create_rlgpu_env(args, cfg, cfg_train)


def _check_cache_is_a_host_build_of_the_draw(task, path, clips, seed, prob):
    """a fresh host build under the same seed and sampling weights draws the same ids; the task's cache holds them within the bars"""
    from emloco_amd.utils.motion_lib_smpl import MotionLib
    lib = task._motion_lib
    skels = [a.model for a in task.humanoid_assets]
    host = MotionLib(path, key_body_ids=KEY_BODIES, device=task.device, build="host")
    host._sampling_prob = prob.clone()
    torch.manual_seed(seed)
    host.load_motions(skels, gender_betas=task.humanoid_betas.cpu(), limb_weights=None, random_sample=True)
    assert torch.equal(host._curr_motion_ids, lib._curr_motion_ids)
    for k in ("length_starts", "_motion_num_frames", "_motion_lengths", "_motion_dt", "_motion_aa", "_motion_bodies"):
        assert torch.equal(getattr(host, k), getattr(lib, k)), k
    case = _case_of(lib, clips, [(np.asarray(m.joint_off, np.float64), None) for m in skels])
    ref = cases.reference(case)
    assert np.array_equal(host.gts.cpu().numpy(), ref["gts"].astype(np.float32))
    cases.assert_bar(case, _arrays(lib), "task cache after resample_motions")


def _check_reset_of_every_env(task):
    """reset_done() with every env flagged: each env starts from its clip of the NEW library at the id / time the reset wrote.  No
    heading flags are set, so the reset applies no heading; its height shift is the one that puts the lowest collision point 0.02 m
    above the ground (what tests/test_gpu_env.py checks), its placement moves x and y."""
    E = task.num_envs
    task.reset_buf[:] = 1
    task.reset_done()
    torch.cuda.synchronize()
    assert (task.reset_buf == 0).all() and (task.progress_buf == 0).all()
    mid, mt = task._sampled_motion_ids, task._motion_start_times
    lib = task._motion_lib
    assert int(mid.min()) >= 0 and int(mid.max()) < E and bool((mt >= 0).all()) and bool((mt <= lib._motion_lengths[mid]).all())
    ref = lib.get_motion_state_smpl(mid, mt)
    root = task._humanoid_root_states
    np.testing.assert_allclose(root[:, 3:7].cpu().numpy(), ref["root_rot"].cpu().numpy(), **POSE_TOL)
    np.testing.assert_allclose(root[:, 7:10].cpu().numpy(), ref["root_vel"].cpu().numpy(), **POSE_TOL)
    np.testing.assert_allclose(root[:, 10:13].cpu().numpy(), ref["root_ang_vel"].cpu().numpy(), **POSE_TOL)
    np.testing.assert_allclose(task._dof_pos.cpu().numpy(), ref["dof_pos"].cpu().numpy(), **POSE_TOL)
    np.testing.assert_allclose(task._dof_vel.cpu().numpy(), ref["dof_vel"].cpu().numpy(), **POSE_TOL)
    # root position: x and y are the sampled place; the height is the clip's plus the shift that grounds the pose
    np.testing.assert_allclose(task._rigid_body_pos[:, 0].cpu().numpy(), root[:, 0:3].cpu().numpy(), rtol=0, atol=0)
    low = task._lowest_point(torch.arange(E, device=task.device)).cpu().numpy()
    np.testing.assert_allclose(low, 0.02, atol=2e-4)
    assert torch.isfinite(task.obs_buf).all() and torch.isfinite(task._amp_obs_buf).all()


@pytest.mark.parametrize("chain", ["plain", "fused_chain"])
def test_task_resamples_in_place_then_reallocates(pickle5, chain):
    from emloco_amd.utils.motion_lib_smpl import MotionLib
    path, clips = pickle5
    E = 8
    env = _make_env(E, ["--motion_file", path, "--motion_build", "device"])
    task = env.task
    lib = task._motion_lib
    assert isinstance(lib, MotionLib) and lib.build == "device" and lib.num_motions() == E and task.shape_resampling_interval == 250
    env.reset(torch.arange(E, device=task.device))                   # the reset structures now hold the first draw's addresses
    if chain == "fused_chain":
        task.fused_chain = True
        for _ in range(2):                                           # the pool of pre-drawn episodes fills from the first draw
            task.reset_buf[:] = 1
            task.reset_done()
    torch.cuda.synchronize()
    ptrs = {k: getattr(lib, k).data_ptr() for k in cases.KEYS}
    per_motion = {k: getattr(lib, k).data_ptr() for k in ("length_starts", "_motion_num_frames", "_motion_lengths", "_motion_dt")}
    n_clips = len(clips)
    lengths = torch.tensor([len(c["pose_quat_global"]) for c in clips.values()])
    # a draw that fits whatever the first one was: weight on the three shortest clips (at most 45 frames each, the first draw had
    # at least 38 per env and left 1.5x its rows)
    short = torch.zeros(n_clips)
    short[lengths.argsort()[:3]] = 1.0 / 3
    lib._sampling_prob = short.clone()
    torch.manual_seed(77)
    info = task.resample_motions()
    assert info["build"] == "device" and not info["reallocated"] and info["num_motions"] == E and lib.num_reallocations == 0
    assert info["distinct_clips"] == len(set(lib._curr_motion_ids.tolist())) >= 2
    assert {k: getattr(lib, k).data_ptr() for k in cases.KEYS} == ptrs
    assert {k: getattr(lib, k).data_ptr() for k in per_motion} == per_motion
    _check_cache_is_a_host_build_of_the_draw(task, path, clips, 77, short)
    _check_reset_of_every_env(task)
    # a draw that cannot fit: every env takes the longest clip
    longest = torch.zeros(n_clips)
    longest[lengths.argmax()] = 1.0
    lib._sampling_prob = longest.clone()
    torch.manual_seed(78)
    info = task.resample_motions()
    assert info["reallocated"] and lib.num_reallocations == 1 and info["distinct_clips"] == 1
    assert lib.gts.shape[0] == E * int(lengths.max()) and lib.gts.data_ptr() != ptrs["gts"]
    assert {k: getattr(lib, k).data_ptr() for k in per_motion} == per_motion           # the per-motion arrays never move
    assert int(lib.length_starts[-1]) + int(lib._motion_num_frames[-1]) == lib.gts.shape[0]
    _check_cache_is_a_host_build_of_the_draw(task, path, clips, 78, longest)
    _check_reset_of_every_env(task)
    for _ in range(3):                                               # and the rollout goes on
        env.step(torch.randn(E, 69, device=task.device) * 0.1)
        task.reset_done()
    torch.cuda.synchronize()
    assert torch.isfinite(task.obs_buf).all()

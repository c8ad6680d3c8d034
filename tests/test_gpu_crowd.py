"""GPU: the crowd-aware terrain sensor on the device -- every scenario of tests/test_crowd_cpu.py through emloco_task_crowd_sensor,
bit-equal to the emulator's output; the task in crowd mode beside a twin in the default configuration; the pacer_group.yaml shape."""
import ctypes as C
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import crowd_ref  # noqa: E402
import emu_crowd  # noqa: E402
import test_crowd_cpu as T  # noqa: E402


class DeviceBackend(emu_crowd.CrowdHost):
    """CrowdHost with every array on the device: the guarded arrays travel whole, so a write outside the rows or the map shows in
    the guard words read back."""

    def launch(self, ids, n):
        from emloco_amd import _lib as L
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if not hasattr(self, "_dev"):
            self._dev = {k: up(getattr(self, k).view(np.int32) if k.endswith("whole") else getattr(self, k))
                         for k in ("hf", "probe_xy", "root_x", "root_y", "_obs_whole", "_flip_whole")}
        d = self._dev
        d["rb"], d["src"], d["src_flip"] = up(self.rb), up(self.src), up(self.src_flip)
        d["_owner_whole"] = up(self._owner_whole.view(np.int32))
        b = type(self.bufs).from_buffer_copy(self.bufs)
        g = 4 * emu_crowd.GUARD
        b.rb_state, b.heightfield, b.probe_xy = d["rb"].data_ptr(), d["hf"].data_ptr(), d["probe_xy"].data_ptr()
        b.root_x, b.root_y, b.owner = d["root_x"].data_ptr(), d["root_y"].data_ptr(), d["_owner_whole"].data_ptr() + g
        b.obs, b.flip_obs = d["_obs_whole"].data_ptr() + g, d["_flip_whole"].data_ptr() + g
        if self.n_copy:
            b.src_obs, b.src_flip_obs = d["src"].data_ptr(), d["src_flip"].data_ptr()
        ids_d = None if ids is None else up(ids)
        lib = L.require_device()
        rc = lib.emloco_task_crowd_sensor(C.byref(b), None if ids_d is None else ids_d.data_ptr(), n,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "emloco_task_crowd_sensor")
        torch.cuda.synchronize()
        for k in ("_obs_whole", "_flip_whole", "_owner_whole"):
            np.copyto(getattr(self, k), d[k].cpu().numpy().view(np.uint32))


SCENARIOS = ([("fixture_" + n, T.fixture_case, (n,)) for n in emu_crowd.fixtures()[1]] +
             [("padded_ids", T.padded_ids_case, ()), ("default", T.default_case, ()), ("dup_12", T.duplicate_case, ((1, 2),)),
              ("dup_21", T.duplicate_case, ((2, 1),)), ("three_calls", T.three_calls_case, ()), ("wrap", T.wrap_case, ())] +
             [("blown_up_%s" % b, T.blown_up_case, (b,)) for b in T.BAD])


@pytest.mark.parametrize("name,body,args", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_scenario_on_device_equals_emulator(name, body, args):
    dev = body(DeviceBackend, *args)                 # (the scenario's own checks against fixtures / restatement run on the device's output)
    emu = body(emu_crowd.EmuBackend, *args)
    assert len(dev) == len(emu) and all(np.array_equal(a, b) for a, b in zip(dev, emu))


# ------------------------------------------------------------------ the task
def _seed(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


def _make_env(num_envs, env_cfg, cfg_env=None, small=True):
    from emloco_amd.run import create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    argv = ["--num_envs", str(num_envs), "--seed", "3"] + (["--small_terrain"] if small else []) + ([] if cfg_env is None else ["--cfg_env", cfg_env])
    args = get_args(argv)
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    cfg["env"].update(env_cfg)
    return create_rlgpu_env(args, cfg, cfg_train)


def _sensor_block_checks(task, C_, res, extent, stamps, gs):
    """The task's sensor block on the task's own state tensors: bit-equal to the emulator's, and equal to the float64 restatement on
    every probe that does not hang on float32 rounding.  Spawn points lie on cell corners (the valid locations are cell indices times
    the cell size, the fixed location is (50, 55)), so a member that walks along an axis keeps a coordinate ON a cell boundary, where
    float32 and float64 may legitimately pick different cells: crowd_ref.unsure names those probes (for such an env all of them,
    through the centre mean), and at least half of the probes must remain."""
    from emloco_amd import _lib as L
    E = task.num_envs
    n_copy = L.SELF_OBS + 2 * L.TRAJ_SAMPLES
    rb = task._rigid_body_state.view(E, 24, 13).cpu().numpy()
    hf = task.height_samples.cpu().numpy()
    hs, vs = task.terrain.horizontal_scale, task.terrain.vertical_scale
    got = task.obs_buf[:, n_copy:].cpu().numpy()
    gotf = task._flip_obs_buf[:, n_copy:].cpu().numpy()
    emu = emu_crowd.EmuBackend(E, hf, hs, vs, res, extent, C_, stamps, gs)
    rows, flip = emu.run(rb)
    assert np.array_equal(got, rows) and np.array_equal(gotf, flip) and emu.guards()
    rr, rf = crowd_ref.sensor(rb, hf, hs, vs, 13, res, extent, C_, stamps, gs)
    sure = ~crowd_ref.unsure(rb, hf.shape, hs, 13, res, extent, stamps, gs)
    print("probes clear of cell boundaries:", sure.mean())
    assert sure.mean() >= 0.5
    got = got.reshape(E, res * res, C_)
    gotf = gotf.reshape(E, res, res, C_)
    assert np.abs(got - rr.reshape(got.shape))[sure].max() <= T.TOL
    assert np.abs(gotf[:, :, ::-1].reshape(got.shape) - rr.reshape(got.shape))[sure].max() <= T.TOL
    return got


def test_task_in_crowd_mode_beside_a_default_twin():
    from emloco_amd import _lib as L
    E, res, gs = 8, 8, 4
    n_copy = L.SELF_OBS + 2 * L.TRAJ_SAMPLES
    crowd_cfg = dict(divide_group=True, num_env_group=gs, velocity_map=True, sensor_res=res, sensor_extent=2)
    tasks = []
    for env_cfg in (crowd_cfg, dict(fused_reset=False)):
        _seed(3)
        env = _make_env(E, env_cfg)
        t = env.task
        tasks.append(t)
        _seed(100)
        env.reset(torch.arange(E, device=t.device))
        t._snap = [{k: getattr(t, k).clone() for k in ("_rigid_body_state", "rew_buf", "reset_buf", "obs_buf", "_flip_obs_buf")}]
        for k in range(3):
            _seed(200 + k)
            env.step(torch.zeros(E, 69, device=t.device))
            t._snap.append({k: getattr(t, k).clone() for k in ("_rigid_body_state", "rew_buf", "reset_buf", "obs_buf", "_flip_obs_buf")})
            if t is tasks[0]:
                seen = _sensor_block_checks(t, 3, res, 2.0, True, gs)
    torch.cuda.synchronize()
    a, b = tasks
    assert a._crowd_mode and not b._crowd_mode and not a._fused_reset and not b._fused_reset
    assert a.num_obs == n_copy + 3 * res * res and a.obs_buf.shape == a._flip_obs_buf.shape == (E, a.num_obs)
    assert a.get_task_obs_size() == 30 + 3 * res * res and list(a.get_task_obs_size_detail().items()) == [("traj", 30), ("heightmap_velocity", 3 * res * res)]
    assert b.num_obs == L.OBS
    for sa, sb in zip(a._snap, b._snap):
        for k in ("_rigid_body_state", "rew_buf", "reset_buf"):
            assert torch.equal(sa[k], sb[k]), k
        for k in ("obs_buf", "_flip_obs_buf"):
            assert torch.equal(sa[k][:, :n_copy], sb[k][:, :n_copy]), k
    assert (np.abs(seen[..., 0]) > 1.0).any()                    # somebody stands in view: 1.7 m x 5, clipped at 15
    # a reset of two envs rewrites those two rows only
    before, before_f = a.obs_buf.clone(), a._flip_obs_buf.clone()
    _seed(300)
    a.reset(torch.tensor([1, 6], device=a.device))
    torch.cuda.synchronize()
    rest = [0, 2, 3, 4, 5, 7]
    assert torch.equal(a.obs_buf[rest], before[rest]) and torch.equal(a._flip_obs_buf[rest], before_f[rest])
    assert not torch.equal(a.obs_buf[[1, 6]], before[[1, 6]])
    # the switches of the other launch arrangements
    for name in ("fused_chain", "overlap_obs", "overlap_reset"):
        assert getattr(a, name) is False
        with pytest.raises(RuntimeError, match=name):
            setattr(a, name, True)
        setattr(b, name, True)
        assert getattr(b, name) is True
        setattr(b, name, False)


def test_task_refuses_what_is_not_built():
    with pytest.raises(NotImplementedError, match="group_obs"):
        _make_env(8, dict(divide_group=True, num_env_group=4, group_obs=True))
    with pytest.raises(Exception, match="multiple"):
        _make_env(10, dict(divide_group=True, num_env_group=4))
    with pytest.raises(ValueError, match="sensor_res"):
        _make_env(8, dict(sensor_res=65))


def test_pacer_group_shape_at_reduced_size():
    import emloco_amd
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    E = 64
    _seed(3)
    env = _make_env(E, dict(num_env_group=16), cfg_env=cfg_env)
    t = env.task
    assert t._crowd_mode and t.sensor_res == 64 and t.sensor_extent == 4 and t.velocity_map and t._crowd is None
    env.reset(torch.arange(E, device=t.device))
    assert t._crowd.group_size == 16 and t._crowd.n_groups == 4 and t._crowd.owner_bytes == 4 * 4 * t.height_samples.numel()
    for k in range(4):
        obs, rew, done, info = env.step(torch.zeros(E, 69, device=t.device))
    torch.cuda.synchronize()
    assert obs.shape == (E, 368 + 2 * 15 + 3 * 64 * 64) and info["flip_obs"].shape == obs.shape
    assert torch.isfinite(obs).all() and torch.isfinite(info["flip_obs"]).all()
    assert (obs[:, 398::3].abs() > 1.0).any() and (obs[:, 399::3] != 0).any()

"""GPU: waypoint tracks -> dense paths on the MI355X (emloco_traj_densify, csrc/traj_kernels.hip), TrajGenerator.reset_on_device under
--pred_path, and `run.py --test --pred_path` end to end.

Kernel against scipy float64 (cases and bar: tests/traj_densify_cases.py).  Measured maxima of |kernel - scipy| on origin-shifted
output over all cases: emulated on the CPU 4.24e-6 m, on the MI355X 4.24e-6 m (the same maximum in the same case: the same
IEEE operations in the same order, no contraction); bar 4 x the larger = 1.70e-5 m, plus one float32 ulp of the largest
coordinate when the origin is added back."""
import ctypes as C
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import traj_densify_cases as TC  # noqa: E402
from emloco_amd.env.util.traj_densify import TRAJ_PHASE, densify, densify_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ the kernel against scipy
@pytest.mark.parametrize("origin", [True, False])
@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_kernel_matches_scipy(shape, origin):
    knot_t, query_t = TC.SHAPES[shape]
    for n in (TC.N_TRAJ if shape == "shipped" else (65,)):
        for offset in (0.0, 100.0):
            way = TC.tracks(n, knot_t, seed=n + len(shape), offset=offset)
            out, valid = densify(torch.from_numpy(way).to(_dev()), knot_t, query_t, origin=origin)
            assert out.dtype == torch.float32 and out.shape == (n, len(query_t), 3) and valid.dtype == torch.bool
            ref = TC.reference(way, knot_t, query_t, origin)
            err = np.abs(out.cpu().numpy() - ref).max()
            print(f"{shape} n={n} offset={offset} origin={origin}: max |kernel - scipy| = {err:.3e} m, extent {np.abs(ref).max():.1f} m")
            assert valid.all()
            assert err <= TC.bar(ref, origin), (shape, n, offset, err)


def test_kernel_extrapolates_the_shipped_tail_and_follows_the_stream():
    way = TC.tracks(257, TRAJ_PHASE, seed=3)
    ref = TC.reference(way, TRAJ_PHASE, TC.QUERY_101, True)
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):                                   # the launch goes to the current stream
        w = torch.from_numpy(way).to(_dev())
        out, _ = densify(w, origin=True)
    side.synchronize()
    assert TRAJ_PHASE[-1] < 85 and np.abs(out.cpu().numpy()[:, 85:] - ref[:, 85:]).max() <= TC.BAR_M      # vertices 85..100: the last piece


def _raw(lib, way, knot_t, query_t, out, valid, flags=0):
    k, q = np.ascontiguousarray(knot_t, np.float32), np.ascontiguousarray(query_t, np.float32)
    return lib.emloco_traj_densify(k.ctypes.data, int(k.size), way.data_ptr(), int(way.shape[0]), q.ctypes.data, int(q.size), out.data_ptr(),
                                   None if valid is None else valid.data_ptr(), flags, C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))


def test_kernel_flags_non_finite_tracks_and_leaves_their_neighbours_alone():
    from emloco_amd import _lib as L
    lib = L.require_device()
    way = TC.tracks(130, TRAJ_PHASE, seed=9, offset=100.0)
    clean, _ = densify(torch.from_numpy(way).to(_dev()))
    way[0, 0, 0], way[64, 6, 2], way[129, 12, 1] = np.nan, np.inf, np.nan          # first, a middle and the last waypoint
    out, valid = densify(torch.from_numpy(way).to(_dev()))
    bad = np.zeros(130, bool)
    bad[[0, 64, 129]] = True
    assert (valid.cpu().numpy() == ~bad).all()
    out, clean = out.cpu().numpy(), clean.cpu().numpy()
    assert (out[bad] == 0).all() and np.array_equal(out[~bad], clean[~bad])
    # valid = NULL: the same output, nothing else written
    w = torch.from_numpy(way).to(_dev())
    out2 = torch.full((130, 101, 3), 7.0, device=_dev())
    assert _raw(lib, w, TRAJ_PHASE, TC.QUERY_101, out2, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), out)


def test_entry_refuses_bad_arguments_without_launching():
    from emloco_amd import _lib as L
    lib = L.require_device()
    even = np.arange(17.0)
    for knots, query in ((even[:3], TC.QUERY_101), (even, TC.QUERY_101), (even[:13], np.zeros(0)), (even[:13], np.arange(129.0)),
                         (np.array([0, 1, 2, 2, 3.0]), TC.QUERY_101)):
        w = torch.ones((2, len(knots), 3), device=_dev())
        out = torch.full((2, max(len(query), 1), 3), 7.0, device=_dev())
        valid = torch.full((2,), 9, dtype=torch.uint8, device=_dev())
        assert _raw(lib, w, knots, query, out, valid) == -1
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (valid == 9).all()            # nothing was launched
        with pytest.raises(ValueError):
            densify(w, knots, query)
    assert _raw(lib, torch.ones((0, 13, 3), device=_dev()), TRAJ_PHASE, TC.QUERY_101, torch.ones(1, device=_dev()), None) == 0      # an empty batch


def test_exporter_batch_on_the_device_agrees_with_the_host_path():
    way = TC.tracks(300, TRAJ_PHASE, seed=12, offset=100.0)
    dev_out, _ = densify(torch.from_numpy(way).to(_dev()))
    host_out, _ = densify_host(way, TRAJ_PHASE, TC.QUERY_101)
    assert np.abs(dev_out.cpu().numpy() - host_out).max() <= TC.bar(host_out, False)


# ------------------------------------------------------------------------------------------------ reset_on_device under --pred_path
@pytest.mark.parametrize("tag", ["plain", "heading"])
def test_reset_on_device_pred_path_matches_host_reset_and_golden(golden, tag):
    """The predicted paths through the real-path table of emloco_task_traj_reset: every env a row, no speed rescaling.  The reference
    places a row as row - (first - root) (traj_generator.py:174), the kernel a table row as (row - first) + root; reset_on_device
    places the call's rows in the reference's order before the launch, so what reaches the heading block is the host's, bit for bit.
    Against the host reset and the reference's golden, within the 1e-4 m of the real-path test (tests/test_gpu_env.py); `plain` has
    no arithmetic left that differs and is bit-exact.  Measured on the MI355X: `plain` 0 against both, `heading` 7.6e-6 m against both
    (the heading block's cosf / sinf / atan2f against torch's)."""
    from helpers import traj_rnd_rows
    from emloco_amd.env.util.traj_generator import TrajGenerator
    from test_traj_densify_cpu import _pred_flags, pred_draws, pred_table
    g = golden("traj_reset_pred")
    heading = tag == "heading"
    mk = lambda dev: TrajGenerator(16, 168 * (2 / 60.0), 101, dev, 2.0, 0.0005, 3.0, 2.0, 0.02, None, hybridInitProb=0.5, flags=_pred_flags(heading),
                                   pred_traj_data=pred_table(g))
    host, tg = mk("cpu"), mk(_dev())
    host.inverted[:] = True
    tg.inverted[:] = True
    init_pos, root_vel = torch.from_numpy(g["init_pos"]), torch.from_numpy(g["root_vel"])
    host.reset(torch.arange(16), init_pos, root_vel, draws=pred_draws(g, tag))
    rows = {k: g[f"{tag}_{k}"] for k in ("r_dtheta", "r_dtheta_sharp", "bern_sharp", "r_heading", "r_dspeed", "r_speed0", "r_inversion")}
    tg.reset_on_device(torch.arange(16, device=_dev()), init_pos.to(_dev()), root_vel.to(_dev()), rnd=torch.from_numpy(traj_rnd_rows(rows)).to(_dev()),
                       real_pick=torch.from_numpy(g[f"{tag}_pred_rids"].astype(np.int32)))
    torch.cuda.synchronize()
    got = tg._verts.cpu().numpy()
    err_host, err_golden = np.abs(got - host._verts.numpy()).max(), np.abs(got - g[f"{tag}_verts"]).max()
    print(f"reset_on_device pred_path {tag}: max |device - host reset| = {err_host:.3e} m, |device - golden| = {err_golden:.3e} m")
    assert np.abs(got[:, 0, :2] - g["init_pos"][:, :2]).max() < 1e-5              # the first vertex sits on the root
    assert err_host < 1e-4 and err_golden < 1e-4, (err_host, err_golden)
    if not heading:
        assert np.array_equal(got, host._verts.numpy())
    assert tg.last_pred_rows.tolist() == g[f"{tag}_pred_rids"].tolist()
    if heading:
        np.testing.assert_array_equal(tg.show_inverted().long().cpu().numpy(), g[f"{tag}_inverted"])
    for flag in ("fixed_path", "slow", "add_noise"):                # these stay on the host path
        f = _pred_flags(heading)
        setattr(f, flag, True)
        tg._flags = f
        with pytest.raises(NotImplementedError):
            tg.reset_on_device(torch.arange(16, device=_dev()), init_pos.to(_dev()), root_vel.to(_dev()))


# ------------------------------------------------------------------------------------------------ --test --pred_path end to end
def _write_pred_table(path, rows=96):
    way = TC.tracks(rows, TRAJ_PHASE, seed=21, offset=100.0)
    dense, _ = densify_host(way, TRAJ_PHASE, TC.QUERY_101)
    table = {i * 20 + 3: {"coord_dense": dense[i], "sample": i, "mode": 3, "ade": 0.0, "locoval": None} for i in range(rows)}
    with open(path, "wb") as f:
        pickle.dump(table, f)
    return table


def test_run_test_pred_path_end_to_end(tmp_path):
    """64 envs on a 96-row table, one game per env: the run finishes and every game's record names the row it walked."""
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    table = str(tmp_path / "preds.pkl")
    _write_pred_table(table)
    torch.manual_seed(11)
    net = str(tmp_path / "locoval.pth")
    torch.save({k: v.cpu() for k, v in ValuePoseNet(True, True).state_dict().items()}, net)
    out, recs = str(tmp_path / "eval.json"), str(tmp_path / "games.npz")
    p = subprocess.run([sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "64", "--seed", "1", *ENV_ARGS, "--policy_random_init",
                        "--valuenet_path", net, "--games_num", "1", "--pred_path", "--pred_traj_file", table, "--eval_out", out,
                        "--eval_records", recs], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    rep = json.load(open(out))
    assert rep["games"] == 64 and rep["shortfall"] == 0
    g = np.load(recs)
    assert len(g["pred_row"]) == 64 and ((g["pred_row"] >= 0) & (g["pred_row"] < 96)).all()
    assert len(set(g["pred_row"].tolist())) == 64                   # the first reset samples without replacement


def test_pred_path_env_walks_its_table_row_from_the_root_position(tmp_path):
    from emloco_amd.run import RLGPUEnv, create_rlgpu_env, fill_flags
    from emloco_amd.utils.config import get_args, load_cfg
    from emloco_amd.utils.flags import flags
    table = _write_pred_table(str(tmp_path / "preds.pkl"))
    args = get_args(["--num_envs", "64", "--seed", "2", "--random_heading", "--pred_path", "--pred_traj_file", str(tmp_path / "preds.pkl")])
    cfg, cfg_train, _ = load_cfg(args)
    fill_flags(args)
    try:
        env = RLGPUEnv(create_rlgpu_env(args, cfg, cfg_train))
        task = env.env.task
        assert not task._fused_reset                                # the host reset places predicted paths
        env.reset(torch.arange(64, device=task.device))
        torch.cuda.synchronize()
        tg = task._traj_gen
        verts, rows = tg._verts.cpu().numpy(), tg.last_pred_rows.numpy()
        root = task._humanoid_root_states[:, :2].cpu().numpy()
        assert ((rows >= 0) & (rows < 96)).all() and len(set(rows.tolist())) == 64
        np.testing.assert_allclose(verts[:, 0, :2], root, atol=1e-5)               # the first vertex is the reset root position
        dense = np.stack([v["coord_dense"] for v in table.values()])[rows]
        np.testing.assert_allclose(verts[:, :, :2] - verts[:, :1, :2], (dense - dense[:, :1])[:, :, :2], atol=1e-4)      # ... and the row's shape
        obs, _, _, _ = env.step(torch.zeros(64, 69, device=task.device))
        assert torch.isfinite(obs).all()
    finally:
        flags.pred_path = False

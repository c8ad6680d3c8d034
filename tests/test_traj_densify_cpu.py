"""CPU-only: waypoint tracks -> dense paths (emloco_traj_densify) and what is built on it -- the kernel emulated on the CPU and the
float64 host path against scipy, the dataset exporter, TrajGenerator.reset under --pred_path against the reference's golden, and the
plumbing of --pred_path / --save_pred_trajs.

Kernel error against scipy float64 (tests/traj_densify_cases.py holds the cases and the bar): emulated kernel at most 4.24e-6 m on
origin-shifted output over all cases, the MI355X the same 4.24e-6 m; bar 4 x the larger = 1.70e-5 m."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.interpolate import CubicSpline

import emu
import traj_densify_cases as TC
from emloco_amd.env.util.traj_densify import TRAJ_PHASE, densify, densify_host
from emloco_amd.utils.flags import Flags


# ------------------------------------------------------------------------------------------------------------ the kernel, emulated
def run_emu(way, knot_t, query_t, origin=False, want_valid=True, fill=7.0):
    way = np.ascontiguousarray(way, np.float32)
    k, q = np.ascontiguousarray(knot_t, np.float32), np.ascontiguousarray(query_t, np.float32)
    out = np.full((way.shape[0], q.size, 3), fill, np.float32)
    valid = np.full(way.shape[0], 9, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = emu.lib().emu_traj_densify(P(k), int(k.size), P(way), C.c_int64(way.shape[0]), P(q), int(q.size), P(out), P(valid) if want_valid else None,
                                    1 if origin else 0)
    return rc, out, valid


@pytest.mark.parametrize("origin", [True, False])
@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_emulated_kernel_matches_scipy(shape, origin):
    knot_t, query_t = TC.SHAPES[shape]
    for n in (TC.N_TRAJ if shape == "shipped" else (65,)):
        for offset in (0.0, 100.0):
            way = TC.tracks(n, knot_t, seed=n + len(shape), offset=offset)
            rc, out, valid = run_emu(way, knot_t, query_t, origin)
            ref = TC.reference(way, knot_t, query_t, origin)
            err = np.abs(out - ref).max()
            print(f"{shape} n={n} offset={offset} origin={origin}: max |kernel - scipy| = {err:.3e} m, extent {np.abs(ref).max():.1f} m")
            assert rc == 0 and valid.tolist() == [1] * n
            assert err <= TC.bar(ref, origin), (shape, n, offset, err)


def test_emulated_kernel_extrapolates_the_shipped_tail():
    """vertices 85..100 of the 101 lie behind the last waypoint (phase 84.87): the last piece, as scipy extrapolates"""
    way = TC.tracks(64, TRAJ_PHASE, seed=3)
    _, out, _ = run_emu(way, TRAJ_PHASE, TC.QUERY_101, origin=True)
    ref = TC.reference(way, TRAJ_PHASE, TC.QUERY_101, True)
    assert TRAJ_PHASE[-1] < 85 and np.abs(out[:, 85:] - ref[:, 85:]).max() <= TC.BAR_M
    # ... and the spline passes through its waypoints
    k = np.round(TRAJ_PHASE).astype(int)
    shifted = way.astype(np.float64).copy()
    shifted[..., :2] -= shifted[:, :1, :2]
    slope = np.abs(np.diff(ref, axis=1)).max()                        # a vertex is at most 0.5 phase units from its waypoint
    assert np.abs(out[:, k] - shifted).max() <= 0.5 * slope + TC.BAR_M


def test_emulated_kernel_flags_non_finite_tracks():
    way = TC.tracks(130, TRAJ_PHASE, seed=9, offset=100.0)
    clean = way.copy()
    way[0, 0, 0], way[64, 6, 2], way[129, 12, 1] = np.nan, np.inf, np.nan          # first, a middle and the last waypoint
    rc, out, valid = run_emu(way, TRAJ_PHASE, TC.QUERY_101)
    _, out_clean, _ = run_emu(clean, TRAJ_PHASE, TC.QUERY_101)
    bad = np.zeros(130, bool)
    bad[[0, 64, 129]] = True
    assert rc == 0 and (valid == ~bad).all()
    assert (out[bad] == 0).all() and np.array_equal(out[~bad], out_clean[~bad])      # the neighbouring rows are untouched
    rc, out2, untouched = run_emu(way, TRAJ_PHASE, TC.QUERY_101, want_valid=False)     # valid = NULL
    assert rc == 0 and np.array_equal(out2, out) and (untouched == 9).all()


def test_emulated_entry_refuses_bad_arguments():
    even = np.arange(17.0)
    for knots, query, word in ((even[:3], TC.QUERY_101, "n_knots"), (even, TC.QUERY_101, "n_knots"), (even[:13], np.zeros(0), "n_query"),
                               (even[:13], np.arange(129.0), "n_query"), (np.array([0, 1, 2, 2, 3.0]), TC.QUERY_101, "increasing"),
                               (np.array([0, 1, np.nan, 3, 4.0]), TC.QUERY_101, "finite")):
        rc, out, _ = run_emu(np.ones((2, len(knots), 3)), knots, query)
        assert rc == -1 and word in emu.lib().emu_traj_densify_error().decode(), (word, emu.lib().emu_traj_densify_error())
        assert (out == 7.0).all()                                     # nothing was launched


def test_emulated_entry_refuses_null_tables_a_bad_count_an_unknown_flag_and_non_finite_queries():
    """the refusals of densify_pack that the table above does not reach"""
    P = lambda a: C.c_void_p(a.ctypes.data)
    k, q = np.arange(13, dtype=np.float32), np.ascontiguousarray(TC.QUERY_101, np.float32)
    bad_q = q.copy()
    bad_q[50] = np.inf
    way, out = np.ones((2, 13, 3), np.float32), np.full((2, q.size, 3), 7.0, np.float32)
    fn = emu.lib().emu_traj_densify
    for args, word in (((None, 13, P(way), C.c_int64(2), P(q), q.size, P(out), None, 0), "null"),
                       ((P(k), 13, P(way), C.c_int64(2), None, q.size, P(out), None, 0), "null"),
                       ((P(k), 13, P(way), C.c_int64(-1), P(q), q.size, P(out), None, 0), "n_traj"),
                       ((P(k), 13, P(way), C.c_int64(2), P(q), q.size, P(out), None, 2), "flag"),
                       ((P(k), 13, P(way), C.c_int64(2), P(bad_q), q.size, P(out), None, 0), "finite")):
        assert fn(*args) == -1 and word in emu.lib().emu_traj_densify_error().decode(), (word, emu.lib().emu_traj_densify_error())
        assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------------------ the float64 host path
@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_host_path_matches_scipy(shape):
    knot_t, query_t = TC.SHAPES[shape]
    way = TC.tracks(65, knot_t, seed=2, offset=100.0).astype(np.float64)
    for origin in (False, True):
        out, valid = densify(way, knot_t, query_t, origin=origin)
        ref = CubicSpline(knot_t, way, axis=1, bc_type="natural")(query_t)
        if origin:
            ref[..., :2] -= way[:, :1, :2]
        assert out.dtype == np.float64 and valid.all() and np.abs(out - ref).max() <= 1e-12
    t_out, t_valid = densify(torch.from_numpy(way), knot_t, query_t)       # a CPU tensor comes back as a tensor
    assert torch.is_tensor(t_out) and t_out.dtype == torch.float64 and np.array_equal(t_out.numpy(), densify_host(way, knot_t, query_t)[0])


def test_host_path_defaults_flags_and_errors():
    way = TC.tracks(5, TRAJ_PHASE, seed=4).astype(np.float64)
    way[3, 5, 1] = np.nan
    out, valid = densify(way)
    assert out.shape == (5, 101, 3) and valid.tolist() == [True, True, True, False, True] and (out[3] == 0).all()
    assert len(TRAJ_PHASE) == 13 and TRAJ_PHASE[1] == pytest.approx(7.07) and TRAJ_PHASE[-1] == pytest.approx(84.87)
    for bad in (dict(knot_t=np.arange(3.0)), dict(knot_t=np.arange(17.0)), dict(query_t=np.arange(129.0)), dict(query_t=np.zeros(0)),
                dict(knot_t=np.array([0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11.0]))):
        kn = bad.get("knot_t", TRAJ_PHASE)
        with pytest.raises(ValueError):
            densify(np.zeros((2, len(kn), 3)), **bad)


# ------------------------------------------------------------------------------------------------------------ the exporter
@pytest.mark.parametrize("dataset", ["jta", "jrdb"])
def test_export_trajs_writes_the_tables_traj_generator_loads(tmp_path, dataset):
    from emloco_amd.env.util.traj_generator import TrajGenerator
    from emloco_amd.predictor import export_trajs
    if dataset == "jta":
        from emloco_amd.predictor.dataset_jta import write_synthetic_split
    else:
        from emloco_amd.predictor.dataset_jrdb import write_synthetic_split
    data = str(tmp_path / "data")
    for split, n in (("train", 9), ("val", 4), ("test", 5)):
        d = write_synthetic_split(data, split, n, max_people=3, seed=len(split))
    train_dir = os.path.join(os.path.dirname(d), "train")
    part = os.path.join(train_dir, sorted(os.listdir(train_dir))[0])
    scenes = pickle.load(open(part, "rb"))
    scenes[1][0][0][14, 0, 1] = float("nan")                           # scene 1: a NaN on the primary's future track -> left out
    scenes[2][0][0][8, 5, 0] = float("nan")                            # scene 2: a NaN in the initial pose -> pose None
    scenes[3][0][0][2, 0, 0] = float("nan")                            # scene 3: a NaN before the last observed frame -> kept
    pickle.dump(scenes, open(part, "wb"))
    written = export_trajs.main(["--cfg", f"configs/{dataset}_all_visual_cues.yaml", "--data_root", data, "--out", str(tmp_path / "out"),
                                 "--device", "cpu"], say=lambda *a: None)
    name = f"{dataset}_all_visual_cues"
    suffix = "_trajs.pkl" if dataset == "jta" else "_trajs_filterv2.pkl"
    assert {k: os.path.basename(v) for k, v in written.items()} == {s: f"{name}_{s}{suffix}" for s in ("train", "val", "test")}
    table = pickle.load(open(written["train"], "rb"))
    assert sorted(table) == [0, 2, 3, 4, 5, 6, 7, 8] and len(pickle.load(open(written["val"], "rb"))) == 4
    assert table[2]["pose"] is None and all(table[i]["pose"].shape == (24, 3) for i in table if i != 2)
    assert all(v["traj"].shape == (101, 3) and v["traj"].dtype == np.float64 for v in table.values())
    # the track: the primary person from the last observed frame (8) on, through scipy's spline
    j = scenes[4][0][0].numpy().astype(np.float64)
    ref = CubicSpline(TRAJ_PHASE, j[8:21, 0, :3], axis=0, bc_type="natural")(np.arange(101))
    assert np.abs(table[4]["traj"] - ref).max() <= 1e-12
    pose_tokens = slice(3, 27) if dataset == "jta" else slice(2, 26)
    np.testing.assert_array_equal(table[4]["pose"], scenes[4][0][0][8, pose_tokens, :3].numpy())
    # TrajGenerator consumes the file as it consumes the reference's
    flags = Flags(dict(real_path=True, jta_path=True, jrdb_path=False, pred_path=False, fixed_path=False, slow=False, adjust_root_vel=False,
                       init_heading=False, heading_inversion=False, add_noise=False, vru=False))
    tg = TrajGenerator(4, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, hybridInitProb=-1.0, flags=flags, traj_data=[written["train"]])
    assert tg.real_rows().shape == (8, 101, 3)
    init = torch.tensor([[50.0, 55.0, 0.9]]).repeat(4, 1)
    tg.reset(torch.arange(4), init, torch.zeros(4, 3), draws=dict(tg._draw(4, 101), real_rids=[0, 2, 3, 7]))
    want = torch.from_numpy(table[7]["traj"]).float()
    want[:, :2] = want[:, :2] - want[0, :2] + init[0, :2]
    np.testing.assert_allclose(tg._verts[3].numpy(), want.numpy(), atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ reset under --pred_path
def _pred_flags(heading):
    return Flags(dict(real_path=False, jta_path=False, jrdb_path=False, pred_path=True, fixed_path=False, slow=False, adjust_root_vel=heading,
                      init_heading=heading, heading_inversion=heading, add_noise=False, vru=False))


def pred_table(g):
    return {int(k): {"coord_dense": row} for k, row in zip(g["pred_keys"], g["pred_table"])}


def pred_draws(g, tag):
    d = {k: torch.from_numpy(g[f"{tag}_{k}"]) for k in ("r_dtheta", "r_dtheta_sharp", "bern_sharp", "r_heading", "r_dspeed", "r_speed0", "r_inversion")}
    d["pred_rids"] = g[f"{tag}_pred_rids"].tolist()
    return d


@pytest.mark.parametrize("tag", ["plain", "heading"])
def test_reset_pred_path_matches_reference(golden, tag):
    """traj_generator.py:163-175 on the reference's own sample: 16 envs, a table of 24 rows at +-100 m; `heading` = init_heading +
    heading_inversion + adjust_root_vel (no speed rescaling in this branch)."""
    from emloco_amd.env.util.traj_generator import TrajGenerator
    g = golden("traj_reset_pred")
    tg = TrajGenerator(16, 168 * (2 / 60.0), 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, hybridInitProb=0.5, flags=_pred_flags(tag == "heading"),
                       pred_traj_data=pred_table(g))
    tg.inverted[:] = True
    tg.pred_row_log = []
    init_pos = torch.from_numpy(g["init_pos"])
    tg.reset(torch.arange(16), init_pos, torch.from_numpy(g["root_vel"]), draws=pred_draws(g, tag))
    assert len(set(g[f"{tag}_pred_rids"].tolist())) == 16 and g["pred_table"].shape == (24, 101, 3)
    np.testing.assert_allclose(tg._verts.numpy(), g[f"{tag}_verts"], rtol=1e-5, atol=2e-5)
    np.testing.assert_array_equal(tg.show_inverted().long().numpy(), g[f"{tag}_inverted"])
    np.testing.assert_allclose(tg._verts[:, 0, :2].numpy(), g["init_pos"][:, :2], atol=1e-5)       # the first vertex sits on the root
    assert tg.last_pred_rows.tolist() == g[f"{tag}_pred_rids"].tolist() and tg.pred_row_log[0][1].tolist() == tg.last_pred_rows.tolist()
    if tag == "heading":                                                # speeds are the table's, whatever the root's speed
        seg = np.linalg.norm(np.diff(tg._verts.numpy()[..., :2], axis=1), axis=-1)
        want = np.linalg.norm(np.diff(g["pred_table"][g[f"{tag}_pred_rids"]][..., :2], axis=1), axis=-1)
        np.testing.assert_allclose(seg, want, atol=2e-5)


def test_reset_pred_path_samples_without_replacement(golden):
    import random
    from emloco_amd.env.util.traj_generator import TrajGenerator
    g = golden("traj_reset_pred")
    tg = TrajGenerator(24, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, flags=_pred_flags(False), pred_traj_data=pred_table(g))
    random.seed(1)
    tg.reset(torch.arange(24), torch.zeros(24, 3), torch.zeros(24, 3))
    assert sorted(tg.last_pred_rows.tolist()) == list(range(24))
    big = TrajGenerator(25, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, flags=_pred_flags(False), pred_traj_data=pred_table(g))
    with pytest.raises(ValueError, match="25 envs.*24 rows"):
        big.reset(torch.arange(25), torch.zeros(25, 3), torch.zeros(25, 3))


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_pred_path_with_a_missing_file_stops_the_run_and_names_it(tmp_path, monkeypatch):
    from emloco_amd import run
    from emloco_amd.env.util.traj_generator import TrajGenerator
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    missing = str(tmp_path / "no_such_preds.pkl")
    with pytest.raises(SystemExit, match="no_such_preds.pkl"):
        run.main(["--pred_path", "--pred_traj_file", missing, "--num_envs", "4"])
    monkeypatch.chdir(tmp_path)                                         # the default is the reference's relative path
    with pytest.raises(SystemExit, match="data/traj/traj_pred_data.pkl"):
        run.main(["--pred_path", "--num_envs", "4"])
    with pytest.raises(FileNotFoundError, match="no_such_preds.pkl"):
        TrajGenerator(4, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, flags=_pred_flags(False), pred_traj_data=missing)


class _StubPredictor(torch.nn.Module):
    """M modes per sample: the primary's last observed step continued, turned a little more per mode -> (B, 12, M * 2)."""

    def __init__(self, modes):
        super().__init__()
        self.modes, self.seen = modes, []

    def forward(self, in_joints, padding_mask, limit_obs=False):
        step = in_joints[:, 8, 0, :2] - in_joints[:, 7, 0, :2]                                   # (B, 2)
        t = torch.arange(1, 13, dtype=step.dtype)[None, :, None]                                  # (1, 12, 1)
        ang = torch.arange(self.modes, dtype=step.dtype)[None, None, :] * 0.05 * t                # (1, 12, M)
        x, y = step[:, None, None, 0], step[:, None, None, 1]
        pred = torch.stack([(x * torch.cos(ang) - y * torch.sin(ang)) * t, (x * torch.sin(ang) + y * torch.cos(ang)) * t], -1)
        self.seen.append(pred)
        return pred.reshape(pred.shape[0], 12, self.modes * 2)


@pytest.mark.parametrize("dataset", ["jta", "jrdb"])
def test_save_pred_trajs_writes_a_table_pred_path_walks(tmp_path, dataset):
    from torch.utils.data import DataLoader
    from emloco_amd.env.util.traj_generator import TrajGenerator
    from emloco_amd.predictor import evaluate_jta as EV
    if dataset == "jta":
        from emloco_amd.predictor.dataset_jta import collate_batch, create_dataset, write_synthetic_split
    else:
        from emloco_amd.predictor.dataset_jrdb import collate_batch, create_dataset, write_synthetic_split
    M, N = 5, 7
    write_synthetic_split(str(tmp_path), "test", N, max_people=3, seed=3)
    ds = create_dataset(f"{dataset}_all_visual_cues", None, split="test", track_size=21, track_cutoff=9, preprocessed=True, root=str(tmp_path))
    config = {"DEVICE": "cpu", "TRAIN": {"input_track_size": 9, "output_track_size": 12}, "MODEL": {"value_threshold": 0.7},
              "DATA": {"train_datasets": [f"{dataset}_all_visual_cues"]}}
    tables = {}
    for modes in ("best", "all"):
        col = EV.PredTrajCollector(modes)
        loader = DataLoader(ds, batch_size=3, num_workers=0, shuffle=False, collate_fn=collate_batch)
        model = _StubPredictor(M)
        res = EV.evaluate_ade_fde(model, None, "test", "traj+all", loader, 3, config, dataset=dataset, pred_trajs=col)
        tables[modes] = pickle.load(open(col.save(str(tmp_path / f"pred_{modes}.pkl")), "rb"))
        assert res["samples"] == N
    best, every = tables["best"], tables["all"]
    assert sorted(best) == list(range(N)) and sorted(every) == list(range(N * M))          # one entry per sample | modes x that
    for i in range(N):
        e = best[i]
        assert set(e) == {"coord_dense", "sample", "mode", "ade", "locoval"} and e["sample"] == i and e["locoval"] is None
        assert e["coord_dense"].shape == (101, 3) and e["coord_dense"].dtype == np.float64
        ades = [every[i * M + m]["ade"] for m in range(M)]
        assert e["mode"] == int(np.argmin(ades)) and e["ade"] == min(ades)                  # no LocoVal network: the min-ADE mode
        np.testing.assert_array_equal(e["coord_dense"], every[i * M + e["mode"]]["coord_dense"])
        last_obs = ds[i][0][0, 8, 0, :3].double().numpy()
        np.testing.assert_allclose(e["coord_dense"][0], last_obs, atol=1e-12)               # vertex 0 is the last observed point
    # vertex round(TRAJ_PHASE[k]) lies within the spline's reach of waypoint k: at most half a phase unit of path away
    scene = ds[2][0]
    pred = torch.cat(model.seen)[2]                                      # (12, M, 2), relative to the last observed point
    for m in range(M):
        dense = every[2 * M + m]["coord_dense"]
        way = np.concatenate([np.zeros((1, 2)), pred[:, m].double().numpy()]) + scene[0, 8, 0, :2].double().numpy()
        slope = np.abs(np.diff(dense[:, :2], axis=0)).max()
        assert np.abs(dense[np.round(TRAJ_PHASE).astype(int), :2] - way).max() <= 0.5 * slope + 1e-5
    # the rollout's generator walks the file
    tg = TrajGenerator(N, 5.6, 101, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, flags=_pred_flags(False), pred_traj_data=str(tmp_path / "pred_best.pkl"))
    init = torch.zeros(N, 3)
    tg.reset(torch.arange(N), init, torch.zeros(N, 3), draws=dict(tg._draw(N, 101), pred_rids=list(range(N))))
    np.testing.assert_allclose(tg._verts[4].numpy()[:, :2], (best[4]["coord_dense"] - best[4]["coord_dense"][0])[:, :2], atol=2e-5)

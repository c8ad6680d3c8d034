"""Dataset tracks to the dense real-path tables `--real_path` walks.

    python -m emloco_amd.predictor.export_trajs --cfg configs/jta_all_visual_cues.yaml [--dataset jta|jrdb] [--data_root data] [--out DIR]

Mirror of social-transmotion/load_jta_traj.py:41-121 and load_jrdb_traj.py:24-123: for train, val and test of the preprocessed
split, the primary person's track from the last observed frame on (13 points at 0.4 s) goes through the natural cubic spline to 101
vertices (`env/util/traj_densify.py`: batched, on the device when there is one, else the float64 host path), and
`{id: {'pose': (24, 3) or None, 'traj': (101, 3) float64}}` is pickled as `<out>/<name>_<split>_trajs.pkl` (JRDB:
`..._trajs_filterv2.pkl`), id = the scene's index in the split.  A track with a NaN is left out (load_jta_traj.py:87-89), an initial
pose with a NaN is stored as None (:111-114).  `TrajGenerator(traj_data=[file])` and `run.py --real_path JTA --real_traj_file file`
load the result.  No plots.
"""
import argparse
import os
import pickle

import numpy as np
import torch

from ..env.util.traj_densify import NUM_VERTS, TRAJ_PHASE, densify

OUT_DIR = os.path.join("data", "saved_trajs")                    # load_jta_traj.py:31
SUFFIX = {"jta": "_trajs.pkl", "jrdb": "_trajs_filterv2.pkl"}    # load_jta_traj.py:34, load_jrdb_traj.py:39
BATCH = 65536


def primary_init_pose(joints, dataset):
    """The 24 joints of the primary person at frame 8: tokens 3:27 of a JTA scene (load_jta_traj.py:38-39), tokens 2: of a JRDB scene
    (load_jrdb_traj.py:24-25).  joints: (people, frames, tokens, 4)."""
    return joints[0, 8, 3:27, :3] if dataset == "jta" else joints[0, 8, 2:, :3]


def export_split(ds, in_F, dataset="jta", device=None, n_knots=len(TRAJ_PHASE)):
    """{id: {'pose', 'traj'}} of one split: `ds[i][0]` is scene i's (people, frames, tokens, 4) tensor."""
    ids, ways, poses = [], [], []
    for i in range(len(ds)):
        joints = torch.as_tensor(ds[i][0])
        traj = joints[0, in_F - 1:, 0, :3]
        if torch.isnan(traj).any() or traj.shape[0] < n_knots:
            continue
        pose = primary_init_pose(joints, dataset)
        ids.append(i)
        ways.append(traj[:n_knots])
        poses.append(None if torch.isnan(pose).any() else pose.numpy().copy())
    out = {}
    for a in range(0, len(ids), BATCH):
        way = torch.stack(ways[a:a + BATCH])
        if device is not None and torch.device(device).type == "cuda":
            dense, ok = densify(way.to(device), origin=False)
            dense = dense.double().cpu()
        else:
            dense, ok = densify(way.double(), origin=False)
        dense, ok = dense.numpy(), ok.cpu().numpy()
        for k in range(len(way)):
            if ok[k]:
                out[ids[a + k]] = {"pose": poses[a + k], "traj": dense[k].copy()}
    assert all(v["traj"].shape == (NUM_VERTS, 3) and v["traj"].dtype == np.float64 for v in out.values())
    return out


def load_yaml(path):
    import yaml
    if not os.path.exists(path):                                  # a shipped config by its relative name, as train_jta.load_config
        shipped = os.path.join(os.path.dirname(os.path.abspath(__file__)), path)
        path = shipped if os.path.exists(shipped) else path
    with open(path, "rt") as f:
        return yaml.safe_load(f)


def main(argv=None, say=print):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", type=str, default="", help="config (default: configs/<dataset>_all_visual_cues.yaml)")
    p.add_argument("--dataset", type=str, default="", choices=["", "jta", "jrdb"], help="default: read off the config's train_datasets")
    p.add_argument("--data_root", type=str, default="data", help="root of <name>/preprocess_smpl*/<split>/*.pkl")
    p.add_argument("--out", type=str, default=OUT_DIR, help="directory of the written tables")
    p.add_argument("--device", type=str, default="auto", help="auto | cpu | cuda[:i]")
    a = p.parse_args(argv)
    cfg = load_yaml(a.cfg or f"configs/{a.dataset or 'jta'}_all_visual_cues.yaml")
    names = cfg["DATA"]["train_datasets"]
    dataset = a.dataset or ("jrdb" if names[0].startswith("jrdb") else "jta")
    if dataset == "jta":
        from .dataset_jta import create_dataset
    else:
        from .dataset_jrdb import create_dataset
    device = a.device
    if device == "auto":
        device = "cuda" if torch.cuda.is_available() else "cpu"
    in_F, out_F = cfg["TRAIN"]["input_track_size"], cfg["TRAIN"]["output_track_size"]
    kw = dict(track_size=in_F + out_F, track_cutoff=in_F, preprocessed=cfg["DATA"]["preprocessed"], root=a.data_root)
    os.makedirs(a.out, exist_ok=True)
    written = {}
    for split in ("train", "val", "test"):
        # train: every dataset of the list, concatenated (load_jta_traj.py:45); val / test: the first one (:52, :58)
        parts = [create_dataset(n, None, split=split, **kw) for n in (names if split == "train" else names[:1])]
        table, base = {}, 0
        for ds in parts:
            table.update({base + i: v for i, v in export_split(ds, in_F, dataset, device).items()})
            base += len(ds)
        path = os.path.join(a.out, f"{names[0]}_{split}{SUFFIX[dataset]}")
        with open(path, "wb") as f:
            pickle.dump(table, f)
        written[split] = path
        say(f"{split}: saved {len(table)} of {base} trajectories to {path}")
    return written


if __name__ == "__main__":
    main()

"""Multi-modal evaluation with the LocoVal filter, vectorised on the device.

Mirror of /root/reference/social-transmotion/evaluate_jta.py:22-35 (`inference`) and :140-500 (`evaluate_ade_fde`), and
of the JRDB variant evaluate_jrdb.py:60-330 (pose tokens `2:` with x negated, threshold 0.8 hard-coded at :206).
The reference walks samples and modes in Python and calls LocoVal with batch 1, 2 x modes times per sample; here one
batch is: one model forward, one batched distance computation, ONE LocoVal launch over B x 2M trajectories, masked
reductions for the filter -- no per-sample host work.

Two arithmetic quirks of the reference loop are reproduced by default so that its logged numbers are matched on the
same inputs (each can be switched off):
  * `reference_gt_shift`: inside the mode loop `gt_xy` gets the origin prepended after mode 0 (:291), so modes 1..M-1
    are scored against the ground truth shifted by one frame (ADE / DES; FDE uses `[-1]` and is unaffected);
  * `reference_inplace_pose`: `ValuePoseNet._rotate_normalization` rotates the caller's pose in place
    (value_pose_net.py:98), so within one sample the pose handed to call c is already rotated by the heading angles
    of all earlier calls (order: pred mode 0, gt, pred mode 1, gt, ...).
Plots of the reference are out of scope.

`--save_pred_trajs FILE` keeps the predictions in the form the rollout walks (`run.py --pred_path --pred_traj_file FILE`,
traj_generator.py:163-175): per stored (sample, mode) the last observed point and the 12 predicted points of the primary person, in
world coordinates, through the natural cubic spline of load_jta_traj.py:93-95 to 101 vertices (`env/util/traj_densify.py`; on the
device when the predictions are there).  `--save_pred_modes best` (default) stores per sample the mode the run keeps -- the LocoVal
arg-max with `--valueloss`, the min-ADE mode without -- and `all` every mode.

`--refine_steps N` (with `--valueloss`) nudges every predicted path along the LocoVal value's gradient before it is scored: N Adam steps
per (sample, mode) on the 12 predicted points (`ValuePoseNet.refine`, one launch per batch; plausibl/test_value_mlp.py:239-274 is the
reference's loop: 750 steps, lr 1e-4).  Everything downstream -- ADE / FDE, the chi distances, the value statistics, the filter, the
saved paths -- sees the refined paths; the summary keeps `ade_unrefined`, `fde_unrefined`, `value_mean_unrefined` of the paths as
predicted and `refine_shift_mean` / `refine_shift_max`, the mean and the largest |change| of a refined coordinate in metres.
`--refine_modes best` refines per sample only the mode with the highest value.  The refinement reads the pose as given
(side-effect-free), while the scoring reproduces `reference_inplace_pose` by default: with a pose-reading network the value statistics
are then those of another pose than the one refined against; `reference_inplace_pose=False` scores what was refined.
"""
import math

import numpy as np
import torch

from .dataset_jrdb import batch_process_coords as batch_process_coords_jrdb
from .train_jta import batch_process_coords

DELTA_T = 0.4      # 2.5 fps (utils/metrics.py:69)


def inference(model, config, input_joints, padding_mask, out_len=14, limit_obs=False):
    """evaluate_jta.py:22-35."""
    model.eval()
    with torch.no_grad():
        if torch.isnan(input_joints).any():
            input_joints = torch.where(torch.isnan(input_joints), torch.zeros_like(input_joints), input_joints)
        if config.get("NOISY_TRAJ", 0):
            input_joints[:, :, 0, :2] = input_joints[:, :, 0, :2] + torch.randn_like(input_joints[:, :, 0, :2]) * config["NOISY_TRAJ"]
        pred_joints = model(input_joints, padding_mask, limit_obs=limit_obs)
    return pred_joints[:, -out_len:]


def calculate_initial_yaw_error(group_A, group_B):
    """utils/metrics.py:49-67."""
    norm_A = torch.norm(group_A, dim=1, keepdim=True)
    norm_B = torch.norm(group_B, dim=1, keepdim=True)
    nA = torch.where(norm_A > 0, group_A / norm_A, group_A)
    nB = torch.where(norm_B > 0, group_B / norm_B, group_B)
    return torch.acos((nA * nB).sum(1).clamp(-1, 1))


def motion_primitives(xy):
    """utils/metrics.py:69-110 for a stack of trajectories xy (..., T, 2): speed, |accel|, |heading rate|, |heading accel|."""
    d = xy[..., 1:, :] - xy[..., :-1, :]
    vel = torch.linalg.norm(d / DELTA_T, dim=-1)
    acc = ((vel[..., 1:] - vel[..., :-1]) / DELTA_T).abs()
    ang = (torch.atan2(d[..., 1], d[..., 0]) / DELTA_T).abs()
    ang_acc = ((ang[..., 1:] - ang[..., :-1]) / DELTA_T).abs()
    return {"velocity": vel, "acceleration": acc, "ang_velocity": ang, "ang_acceleration": ang_acc}


def _chi_from_counts(gt_counts, pred_counts):
    gt_dens, pred_dens = gt_counts / max(gt_counts.sum(), 1), pred_counts / max(pred_counts.sum(), 1)
    s = gt_dens + pred_dens
    nz = s != 0
    return float((((gt_dens - pred_dens) ** 2)[nz] / s[nz]).sum())


def calculate_chi_distance(gt_primitive, pred_primitive, num_bins=20, reduce=None):
    """utils/metrics.py:112-145: chi-square distance of the 20-bin histograms over the joint value range.
    `density=True` histograms times the bin width are count fractions, so ranks only need to agree on the range
    (`reduce("min"/"max", x)`) and add their counts (`reduce("sum", x)`) to get the single-process result."""
    out = {}
    for key in gt_primitive:
        gt_values, pred_values = np.asarray(gt_primitive[key], np.float64), np.asarray(pred_primitive[key], np.float64)
        lo, hi = min(gt_values.min(), pred_values.min()), max(gt_values.max(), pred_values.max())
        if reduce is not None:
            lo, hi = float(reduce("min", np.array([lo]))[0]), float(reduce("max", np.array([hi]))[0])
        bins = np.linspace(lo, hi, num_bins + 1)
        gt_counts = np.histogram(gt_values, bins=bins)[0].astype(np.float64)
        pred_counts = np.histogram(pred_values, bins=bins)[0].astype(np.float64)
        if reduce is not None:
            gt_counts, pred_counts = reduce("sum", gt_counts), reduce("sum", pred_counts)
        out[key] = _chi_from_counts(gt_counts, pred_counts)
    return out


def _dist_reduce(op, arr):
    """all-reduce a float64 numpy array over the default process group (RCCL on GPUs, gloo in the CPU tests)."""
    import torch.distributed as dist
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).clone()
    if dist.get_backend() == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op={"sum": dist.ReduceOp.SUM, "min": dist.ReduceOp.MIN, "max": dist.ReduceOp.MAX}[op])
    return t.cpu().numpy()


def _heading(traj):
    """angle of _rotate_normalization (value_pose_net.py:76-85) for traj (..., 13, 2)."""
    x, y = traj[..., 1, 0], traj[..., 1, 1]
    x = torch.where(x.abs() < 1e-10, torch.full_like(x, 1e-10), x)
    return torch.atan2(y, x)


def _rotate_xy(v, ang):
    """bmm(v, R(ang)) with R = [[c, -s], [s, c]]: (x, y) -> (x c + y s, -x s + y c)."""
    c, s = torch.cos(ang), torch.sin(ang)        # ang has the shape of v[..., 0]
    x, y = v[..., 0], v[..., 1]
    return torch.stack([x * c + y * s, -x * s + y * c], dim=-1)


class EvalAccumulator:
    """Running sums of evaluate_ade_fde; `update` consumes one batch on the device, `summary` gives the logged numbers."""

    def __init__(self, filter_threshold=0.7, reference_gt_shift=True, reference_inplace_pose=True):
        self.thr = float(filter_threshold)
        self.gt_shift, self.inplace_pose = reference_gt_shift, reference_inplace_pose
        self.s = {k: 0.0 for k in ("ade", "fde", "ade_min", "fde_min", "ade_max", "fde_max", "iye", "ade_value", "fde_value",
                                   "ade_random", "fde_random", "minade_value", "minfde_value", "ade_filtered", "fde_filtered",
                                   "value", "value_gt", "value_loss", "value_loss_gt")}
        self.des = np.zeros(12)
        self.n = {"sample": 0, "value_sampling": 0, "filtered": 0, "random": 0, "values": 0}
        self.gt_prim = {k: [] for k in ("velocity", "acceleration", "ang_velocity", "ang_acceleration")}
        self.pred_prim = {k: [] for k in self.gt_prim}
        self.num_mode = 1
        self.values, self.ades, self.fdes = [], [], []

    @torch.no_grad()
    def update(self, in_joints, out_joints, pred_joints, primary_init_pose, valuenet=None, random_ids=None, dataset="jta"):
        dev = pred_joints.device
        B = out_joints.shape[0]
        pred = pred_joints.reshape(B, 12, -1, 2).float()
        M = pred.shape[2]
        self.num_mode = M
        gt = out_joints[:, :, 0, :2].float()                                      # (B,12,2)
        self.s["iye"] += float(calculate_initial_yaw_error(gt[:, 0], pred[:, 0, 0]).sum())
        gt_m = gt[:, :, None, :].expand(B, 12, M, 2)
        if self.gt_shift and M > 1:
            shifted = torch.cat([torch.zeros(B, 1, 2, device=dev), gt[:, :11]], 1)
            gt_m = torch.cat([gt[:, :, None, :], shifted[:, :, None, :].expand(B, 12, M - 1, 2)], 2)
        des = torch.linalg.norm(gt_m - pred, dim=-1).double()                     # (B,12,M)
        ade = des.mean(1)                                                         # (B,M)
        fde = torch.linalg.norm(gt[:, -1, None, :] - pred[:, -1], dim=-1).double()
        self.s["ade"] += float(ade.mean(1).sum())
        self.s["fde"] += float(fde.mean(1).sum())
        self.s["ade_min"] += float(ade.min(1)[0].sum())
        self.s["fde_min"] += float(fde.min(1)[0].sum())
        self.s["ade_max"] += float(ade.max(1)[0].sum())
        self.s["fde_max"] += float(fde.max(1)[0].sum())
        self.des += des.mean(2).sum(0).cpu().numpy()
        self.n["sample"] += B
        self.last = {"pred": pred, "ade": ade, "value": None, "valid": None}      # this batch, for PredTrajCollector
        for k, v in motion_primitives(gt).items():
            self.gt_prim[k].append(v.reshape(-1))
        for k, v in motion_primitives(pred.permute(0, 2, 1, 3)).items():
            self.pred_prim[k].append(v.reshape(-1))
        if valuenet is None:
            return
        # ---- LocoVal over every (sample, mode) prediction and the ground truth, one launch
        init_pose = primary_init_pose.to(dev).float().clone()
        if dataset == "jta":
            init_pose[..., 2] = -init_pose[..., 2]                                # evaluate_jta.py:221
        else:
            init_pose[..., 0] = -init_pose[..., 0]                                # evaluate_jrdb.py:108
        init_vel = ((in_joints[:, 8, 0, :2] - in_joints[:, 7, 0, :2]) * 2.5).to(dev).float()
        zero = torch.zeros(B, 1, 2, device=dev)
        gt_traj = torch.cat([zero, gt], 1)                                        # (B,13,2)
        pred_traj = torch.cat([zero[:, :, None, :].expand(B, 1, M, 2), pred], 1).permute(0, 2, 1, 3)   # (B,M,13,2)
        # call order of the reference loop: pred 0, gt, pred 1, gt, ...
        calls = torch.stack([pred_traj, gt_traj[:, None].expand(B, M, 13, 2)], 2).reshape(B, 2 * M, 13, 2)
        valid = ~(torch.isnan(init_pose).reshape(B, -1).any(1)[:, None] | torch.isnan(pred_traj).reshape(B, M, -1).any(2))   # (B,M)
        pose_c = init_pose[:, None].expand(B, 2 * M, 24, 3).clone()
        reads_pose, reads_vel = getattr(valuenet, "use_pose", True), getattr(valuenet, "use_vel", True)
        if self.inplace_pose and reads_pose:                                      # (a network that does not read the pose: nothing to reproduce)
            theta = _heading(calls) * valid.repeat_interleave(2, 1)               # skipped calls do not rotate the pose
            before = torch.cumsum(theta, 1) - theta                               # rotation already applied when call c starts
            pose_c[..., :2] = _rotate_xy(pose_c[..., :2], before[:, :, None].expand(B, 2 * M, 24))
            hidden = before.new_zeros(B, 2 * M, dtype=torch.bool)
            hidden[:, 1:] = (torch.cumsum(valid.repeat_interleave(2, 1).int(), 1)[:, :-1] > 0)
            for j in (4, 8, 9, 10, 11):                                           # joints zeroed by the first executed call
                pose_c[:, :, j] = torch.where(hidden[:, :, None], torch.zeros_like(pose_c[:, :, j]), pose_c[:, :, j])
        flat = lambda t: t.reshape(B * 2 * M, *t.shape[2:]).contiguous()
        safe_calls = torch.nan_to_num(flat(calls))
        safe_pose = torch.nan_to_num(flat(pose_c))
        vel_c = torch.nan_to_num(flat(init_vel[:, None].expand(B, 2 * M, 2)))
        was_inplace = getattr(valuenet, "inplace_pose", False)
        valuenet.inplace_pose = False
        values = valuenet(safe_calls, safe_pose if reads_pose else None, vel_c if reads_vel else None).reshape(B, M, 2).double()
        valuenet.inplace_pose = was_inplace
        v_pred, v_gt = values[..., 0], values[..., 1]
        self.last.update(value=v_pred, valid=valid)
        nv = int(valid.sum())
        self.n["values"] += nv
        self.s["value"] += float((v_pred * valid).sum())
        self.s["value_gt"] += float((v_gt * valid).sum())
        self.s["value_loss"] += float((((v_pred - 1) ** 2) * valid).sum())
        self.s["value_loss_gt"] += float((((v_gt - 1) ** 2) * valid).sum())
        if M <= 1:
            return
        self.values.append(v_pred[valid].cpu()); self.ades.append(ade[valid].cpu()); self.fdes.append(fde[valid].cpu())
        has = valid.any(1)                                                        # samples with at least one scored mode
        big = 1e30
        if random_ids is None:
            random_ids = torch.randint(0, M, (B,), device=dev)
        random_ids = torch.as_tensor(random_ids, device=dev).long()
        self.s["ade_random"] += float((ade.gather(1, random_ids[:, None])[:, 0] * has).sum())
        self.s["fde_random"] += float((fde.gather(1, random_ids[:, None])[:, 0] * has).sum())
        self.n["random"] += int(has.sum())
        kept = valid & (v_pred >= self.thr)
        rejected = valid & (v_pred < self.thr)
        any_kept = kept.any(1)
        best = torch.where(valid, v_pred, torch.full_like(v_pred, -big)).argmax(1)
        ade_best, fde_best = ade.gather(1, best[:, None])[:, 0], fde.gather(1, best[:, None])[:, 0]
        fallback = has & ~any_kept                                                # nothing passes: the arg-max value mode stands in
        self.s["ade_value"] += float((ade * kept).sum() + (ade_best * fallback).sum())
        self.s["fde_value"] += float((fde * kept).sum() + (fde_best * fallback).sum())
        self.n["value_sampling"] += int(kept.sum()) + int(fallback.sum())
        min_ade_kept = torch.where(kept, ade, torch.full_like(ade, big)).min(1)[0]
        min_fde_kept = torch.where(kept, fde, torch.full_like(fde, big)).min(1)[0]
        self.s["minade_value"] += float(torch.where(any_kept, min_ade_kept, ade_best * fallback).sum())
        self.s["minfde_value"] += float(torch.where(any_kept, min_fde_kept, fde_best * fallback).sum())
        self.s["ade_filtered"] += float((ade * rejected).sum() + (ade_best * fallback).sum())      # evaluate_jta.py:339-340,356-359
        self.s["fde_filtered"] += float((fde * rejected).sum() + (fde_best * fallback).sum())
        self.n["filtered"] += int(rejected.sum())

    def summary(self, distributed=None):
        """The numbers evaluate_ade_fde logs.  With `distributed` (default: a process group with world_size > 1 exists) the
        running sums, histogram counts and per-bin statistics are all-reduced first, so every rank returns the result of
        the whole data-parallel evaluation (eval shards by batch, only scalars are exchanged)."""
        import torch.distributed as dist
        if distributed is None:
            distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        red = _dist_reduce if distributed else None
        s, cnt, des, num_mode = dict(self.s), dict(self.n), self.des.copy(), self.num_mode
        if distributed:
            keys_s, keys_n = sorted(s), sorted(cnt)
            flat = _dist_reduce("sum", np.array([s[k] for k in keys_s] + [cnt[k] for k in keys_n] + list(des)))
            s = dict(zip(keys_s, flat[:len(keys_s)]))
            cnt = {k: int(round(v)) for k, v in zip(keys_n, flat[len(keys_s):len(keys_s) + len(keys_n)])}
            des = flat[len(keys_s) + len(keys_n):]
            num_mode = int(_dist_reduce("max", np.array([float(num_mode)]))[0])
        n = max(cnt["sample"], 1)
        out = {"samples": cnt["sample"], "ade": s["ade"] / n, "fde": s["fde"] / n, "min_ade": s["ade_min"] / n,
               "min_fde": s["fde_min"] / n, "worst_ade": s["ade_max"] / n, "worst_fde": s["fde_max"] / n,
               "iye": s["iye"] / n, "des": des / n}
        if self.gt_prim["velocity"]:
            gp = {k: torch.cat(v).cpu().numpy() for k, v in self.gt_prim.items()}
            pp = {k: torch.cat(v).cpu().numpy() for k, v in self.pred_prim.items()}
            out.update({"chi_" + k: v for k, v in calculate_chi_distance(gp, pp, reduce=red).items()})
        if cnt["values"]:
            nv = cnt["values"]
            out.update({"value_mean": s["value"] / nv, "value_gt_mean": s["value_gt"] / nv,
                        "value_loss_mean": s["value_loss"] / nv, "value_loss_gt_mean": s["value_loss_gt"] / nv})
        if num_mode > 1 and cnt["values"]:
            d = lambda a, b: a / b if b > 0 else 0.0
            out.update({"threshold": self.thr, "ade_value": d(s["ade_value"], cnt["value_sampling"]),
                        "fde_value": d(s["fde_value"], cnt["value_sampling"]),
                        "ade_random": d(s["ade_random"], cnt["sample"]), "fde_random": d(s["fde_random"], cnt["sample"]),
                        "minade_value": d(s["minade_value"], cnt["sample"]), "minfde_value": d(s["minfde_value"], cnt["sample"]),
                        "ade_rejected": d(s["ade_filtered"], cnt["filtered"]), "fde_rejected": d(s["fde_filtered"], cnt["filtered"])})
            # plausibility-score bins (evaluate_jta.py:432-449): mean ADE / FDE per 0.1-wide value bin, value histogram
            if self.values:
                v, a, f = torch.cat(self.values).numpy(), torch.cat(self.ades).numpy(), torch.cat(self.fdes).numpy()
            else:
                v = a = f = np.zeros(0)
            idx = np.digitize(v, np.arange(0, 1.05, 0.1))
            per_bin = np.stack([np.array([x[idx == i].sum() for i in range(1, 11)]) for x in (a, f, np.ones_like(v))])
            hist = np.histogram(v, bins=10, range=(0, 1))[0].astype(np.float64)
            if distributed:
                per_bin, hist = _dist_reduce("sum", per_bin), _dist_reduce("sum", hist)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["ade_per_value_bin"] = np.where(per_bin[2] > 0, per_bin[0] / per_bin[2], np.nan)
                out["fde_per_value_bin"] = np.where(per_bin[2] > 0, per_bin[1] / per_bin[2], np.nan)
            out["value_hist"] = hist.astype(np.int64)
        return out


class PredTrajCollector:
    """The predictions of an evaluation as the table `--pred_path` walks: {key: {'coord_dense': (101, 3) float64, 'sample': i, 'mode': m,
    'ade': ..., 'locoval': ... or None}} (with --refine_steps also 'locoval_unrefined' and 'refined': True), `coord_dense` being the key
    traj_generator.py:170 reads.  modes = "best": one entry per sample
    (key i), the mode of the highest LocoVal value among the scored ones, or of the lowest ADE when no LocoVal network scores the run;
    "all": every mode (key i * M + m).  A track with a non-finite point is left out, as load_jta_traj.py:87-89 leaves such tracks out."""

    def __init__(self, modes="best"):
        if modes not in ("best", "all"):
            raise ValueError("--save_pred_modes is best or all")
        self.modes, self.entries = modes, {}

    @torch.no_grad()
    def add(self, first_sample, last_observed, last):
        """One batch: `last_observed` (B, 3) world position of the primary person at the last observed frame, `last` = what
        EvalAccumulator.update kept of the batch (pred (B, 12, M, 2) relative to that position, ade (B, M), value / valid (B, M) or None)."""
        from ..env.util.traj_densify import densify
        pred, ade, value, valid = last["pred"], last["ade"], last["value"], last["valid"]
        B, _, M, _ = pred.shape
        org = last_observed.to(pred.device).to(pred.dtype)
        if self.modes == "best":
            if value is not None:
                pick = torch.where(valid, value, torch.full_like(value, -1e30)).argmax(1)
            else:
                pick = torch.nan_to_num(ade, nan=1e30).argmin(1)
            mode = pick[:, None]                                                  # (B, 1)
        else:
            mode = torch.arange(M, device=pred.device)[None, :].expand(B, M)
        K = mode.shape[1]
        sel = pred.permute(0, 2, 1, 3).gather(1, mode[:, :, None, None].expand(B, K, 12, 2))       # (B, K, 12, 2)
        way = torch.zeros(B, K, 13, 3, device=pred.device, dtype=pred.dtype)
        way[:, :, :, :] = org[:, None, None, :]
        way[:, :, 1:, :2] += sel
        dense, ok = densify(way.reshape(B * K, 13, 3), origin=False)
        dense, ok = dense.double().cpu().numpy().reshape(B, K, -1, 3), ok.cpu().numpy().reshape(B, K)
        ade_k = ade.gather(1, mode).cpu().numpy()
        val_k = None if value is None else value.gather(1, mode).cpu().numpy()
        unrefined = last.get("value_unrefined")                                   # (--refine_steps: the value of the path as predicted)
        unref_k = None if unrefined is None else unrefined.gather(1, mode).cpu().numpy()
        mode = mode.cpu().numpy()
        for b in range(B):
            for k in range(K):
                if not ok[b, k]:
                    continue
                i, m = first_sample + b, int(mode[b, k])
                self.entries[i if self.modes == "best" else i * M + m] = {
                    "coord_dense": dense[b, k].copy(), "sample": i, "mode": m, "ade": float(ade_k[b, k]),
                    "locoval": None if val_k is None else float(val_k[b, k])}
                if unref_k is not None:
                    self.entries[i if self.modes == "best" else i * M + m].update(locoval_unrefined=float(unref_k[b, k]), refined=True)

    def save(self, path):
        import os
        import pickle
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(self.entries, f)
        return path


def refine_predictions(valuenet, in_joints, pred_joints, primary_init_pose, dataset="jta", steps=750, lr=1e-4, anchor_w=0.0, modes="all"):
    """`pred_joints` (B, 12, M [x] 2) of `inference` with every (sample, mode) path refined against `valuenet` (ValuePoseNet.refine on the
    LocoVal inputs `EvalAccumulator.update` builds: origin prepended, pose with the dataset's axis negated, velocity from the last two
    observed frames), in the same shape, and (sum, count, max) of |change| over the coordinates of the refined paths.  modes = "best":
    per sample only the mode of the highest value is refined.  Paths with a non-finite input are left as they are."""
    if modes not in ("all", "best"):
        raise ValueError("--refine_modes is all or best")
    dev = pred_joints.device
    B = pred_joints.shape[0]
    pred = pred_joints.reshape(B, 12, -1, 2).float()
    M = pred.shape[2]
    init_pose = primary_init_pose.to(dev).float().clone()
    if dataset == "jta":
        init_pose[..., 2] = -init_pose[..., 2]
    else:
        init_pose[..., 0] = -init_pose[..., 0]
    init_vel = ((in_joints[:, 8, 0, :2] - in_joints[:, 7, 0, :2]) * 2.5).to(dev).float()
    traj = torch.cat([torch.zeros(B, M, 1, 2, device=dev), pred.permute(0, 2, 1, 3)], 2).reshape(B * M, 13, 2).contiguous()
    pose = init_pose[:, None].expand(B, M, 24, 3).reshape(B * M, 24, 3)
    vel = init_vel[:, None].expand(B, M, 2).reshape(B * M, 2)
    mask = None
    if modes == "best" and M > 1:
        v0 = valuenet.refine(traj, pose, vel, steps=0)[1].reshape(B, M)
        mask = torch.zeros(B, M, dtype=torch.bool, device=dev)
        mask[torch.arange(B, device=dev), torch.nan_to_num(v0, nan=-1e30).argmax(1)] = True
        mask = mask.reshape(B * M)
    out, _before, after = valuenet.refine(traj, pose, vel, steps=steps, lr=lr, anchor_w=anchor_w, row_mask=mask)
    done = torch.isfinite(after)                                                  # the rows that were refined
    shift = (out[done, 1:] - traj[done, 1:]).abs().double()
    stats = (float(shift.sum()), int(shift.numel()), float(shift.max()) if shift.numel() else 0.0)
    refined = out[:, 1:].reshape(B, M, 12, 2).permute(0, 2, 1, 3).reshape(pred_joints.shape).to(pred_joints.dtype)
    return refined, stats


def evaluate_ade_fde(model, valuenet, split, modality_selection, dataloader, bs, config, logger=None, exp_name="", return_all=False,
                     visualize=False, limit_obs=False, dataset="jta", random_ids=None, shard=None, pred_trajs=None,
                     refine_steps=0, refine_lr=1e-4, refine_anchor=0.0, refine_modes="all", **acc_kw):
    """Same arguments as the reference; additionally returns the summary dict (the reference only logs it).
    Data-parallel (configs[4]): with a process group of W ranks, rank r evaluates batches r, r+W, ... (`shard=(r, W)`,
    default from torch.distributed) and the summary is all-reduced -- no tensor data crosses ranks.
    refine_steps > 0 (`--refine_steps`): every prediction goes through `refine_predictions` between `inference` and the accumulator; a
    second accumulator scores the paths as predicted for the `*_unrefined` keys.  With 0 nothing of this runs."""
    import torch.distributed as dist
    if refine_steps > 0 and valuenet is None:
        raise ValueError("--refine_steps needs a LocoVal network to ascend: pass --valueloss")
    if shard is None:
        shard = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    out_F = config["TRAIN"]["output_track_size"]
    thr = 0.8 if dataset == "jrdb" else config["MODEL"]["value_threshold"]
    acc = EvalAccumulator(thr, **acc_kw)
    acc0 = EvalAccumulator(thr, **acc_kw) if refine_steps > 0 else None           # the paths as predicted
    shift_sum, shift_n, shift_max = 0.0, 0, 0.0
    off = 0
    for bi, batch in enumerate(dataloader):
        joints, masks, padding_mask = batch[0], batch[1], batch[2]
        if bi % shard[1] != shard[0]:
            off += joints.shape[0]
            continue
        padding_mask = padding_mask.to(config["DEVICE"])
        primary_init_pose = joints[:, 0, 8, 3:27, :3] if dataset == "jta" else joints[:, 0, 8, 2:, :3]
        bpc = batch_process_coords if dataset == "jta" else batch_process_coords_jrdb
        in_joints, in_masks, out_joints, out_masks, padding_mask = bpc(joints, masks, padding_mask, config, modality_selection)
        pred_joints = inference(model, config, in_joints, padding_mask, out_len=out_F, limit_obs=limit_obs)
        B = out_joints.shape[0]
        ids = None if random_ids is None else random_ids[off:off + B]
        off += B
        if acc0 is not None:
            if ids is None:                                                       # one draw for both accumulators (the one `update` makes)
                ids = torch.randint(0, pred_joints.reshape(B, 12, -1, 2).shape[2], (B,), device=pred_joints.device)
            acc0.update(in_joints, out_joints, pred_joints, primary_init_pose, valuenet, ids, dataset)
            pred_joints, (ds, dn, dm) = refine_predictions(valuenet, in_joints, pred_joints, primary_init_pose, dataset, refine_steps, refine_lr,
                                                           refine_anchor, refine_modes)
            shift_sum, shift_n, shift_max = shift_sum + ds, shift_n + dn, max(shift_max, dm)
        acc.update(in_joints, out_joints, pred_joints, primary_init_pose, valuenet, ids, dataset)
        if acc0 is not None:
            acc.last["value_unrefined"] = acc0.last["value"]
        if pred_trajs is not None:                                                # (a PredTrajCollector)
            pred_trajs.add(off - B, joints[:, 0, config["TRAIN"]["input_track_size"] - 1, 0, :3], acc.last)
    res = acc.summary()
    if acc0 is not None:
        res0 = acc0.summary()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            shift_sum, shift_n = _dist_reduce("sum", np.array([shift_sum, float(shift_n)]))
            shift_max = float(_dist_reduce("max", np.array([shift_max]))[0])
        res.update({"refine_steps": int(refine_steps), "ade_unrefined": res0["ade"], "fde_unrefined": res0["fde"],
                    "value_mean_unrefined": res0.get("value_mean", float("nan")),
                    "refine_shift_mean": float(shift_sum) / max(float(shift_n), 1.0), "refine_shift_max": float(shift_max)})
    if logger is not None:
        logger.info(f"Total samples: {res['samples']}")
        for label, key in (("ADE", "ade"), ("FDE", "fde"), ("Min ADE", "min_ade"), ("Min FDE", "min_fde"), ("Worst ADE", "worst_ade"),
                           ("Worst FDE", "worst_fde"), ("IYE", "iye")):
            logger.info(f"{label}: {res[key]:.5f}")
        logger.info(f"DES: {np.round(res['des'], 5)}")
        if "chi_velocity" in res:
            logger.info(f"Chi-square distance:\\n Velocity: {res['chi_velocity']:.5f},\\n Acceleration: {res['chi_acceleration']:.5f},\\n "
                        f"Angular velocity: {res['chi_ang_velocity']:.5f},\\n Angular acceleration: {res['chi_ang_acceleration']:.5f}")
        if "ade_value" in res:
            logger.info(f"Threadhold: {res['threshold']}")
            for label, key in (("ADE with Value sampling", "ade_value"), ("FDE with Value sampling", "fde_value"),
                               ("ADE with Random sampling", "ade_random"), ("FDE with Random sampling", "fde_random"),
                               ("Min ADE with Value sampling", "minade_value"), ("Min FDE with Value sampling", "minfde_value"),
                               ("ADE of rejected samples", "ade_rejected"), ("FDE of rejected samples", "fde_rejected")):
                logger.info(f"{label}: {res[key]:.5f}")
        if acc0 is not None:
            logger.info(f"Refined with {res['refine_steps']} steps: ADE {res['ade_unrefined']:.5f} -> {res['ade']:.5f}, FDE {res['fde_unrefined']:.5f} -> "
                        f"{res['fde']:.5f}, value {res['value_mean_unrefined']:.5f} -> {res.get('value_mean', float('nan')):.5f}, "
                        f"shift mean {res['refine_shift_mean']:.5f} m, max {res['refine_shift_max']:.5f} m")
    return res


# ---------------------------------------------------------------------------------------------- entry point (evaluate_jta.py:509-625)
def build_arg_parser():
    """The flags of the reference's `python evaluate_jta.py` (evaluate_jta.py:511-527), plus --data_root / --out_root / --dataset."""
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument("--exp_name", type=str, help="checkpoint path")
    p.add_argument("--split", type=str, default="test", help="Split to use. one of [train, test, valid]")
    p.add_argument("--metric", type=str, default="ade_fde", help="Evaluation metric")
    p.add_argument("--modality", type=str, default="traj+all", help="modality combination, e.g. 'traj', 'traj+3dpose', 'traj+all'")
    p.add_argument("--vis", action="store_true", help="Visualize the predictions (out of scope here: ignored)")
    p.add_argument("--limit_obs", type=int, default=0, help="Limit the number of observations")
    p.add_argument("--valueloss", action="store_true", help="Use value loss")
    p.add_argument("--all_frames", action="store_true", help="Evaluate all observation frames")
    p.add_argument("--noisy_traj", type=float, default=0, help="Add noise to the trajectory to mimic real data")
    p.add_argument("--multi_modal", action="store_true", help="Use multi-modal model")
    p.add_argument("--last_epoch", action="store_true", help="Use last epoch checkpoint")
    p.add_argument("--no_pose", action="store_true", help="No pose in valuenet")
    p.add_argument("--no_vel", action="store_true", help="No velocity in valuenet")
    p.add_argument("--epoch", type=str, default=0, help="Epoch to evaluate")
    p.add_argument("--filter_threshold", type=float, default=0.7, help="Threshold for filtering samples")
    p.add_argument("--data_root", type=str, default="data", help="root of <dataset>/preprocess_smpl/<split>/part_*.pkl")
    p.add_argument("--out_root", type=str, default="experiments", help="root of the experiment directories")
    p.add_argument("--dataset", type=str, default="jta", choices=["jta", "jrdb"], help="evaluate_jta.py | evaluate_jrdb.py")
    p.add_argument("--save_pred_trajs", type=str, default="", help="write the predictions as a --pred_path table (101-vertex paths) to this pickle")
    p.add_argument("--save_pred_modes", type=str, default="best", choices=["best", "all"], help="the mode the run keeps per sample | every mode")
    p.add_argument("--refine_steps", type=int, default=0, help="Adam steps that raise the LocoVal value of every predicted path before it is scored (0: off; needs --valueloss)")
    p.add_argument("--refine_lr", type=float, default=1e-4, help="learning rate of the refinement (metres per step, about)")
    p.add_argument("--refine_anchor", type=float, default=0.0, help="weight of the mean squared distance to the predicted path in the refinement's objective")
    p.add_argument("--refine_modes", type=str, default="all", choices=["all", "best"], help="refine every mode | per sample the mode of the highest value")
    return p


def find_checkpoint(args):
    """evaluate_jta.py:537-553: which file of the experiment's checkpoint directory the flags select."""
    import os
    d = os.path.join(args.out_root, args.dataset.upper(), args.exp_name, "checkpoints")
    if args.last_epoch:
        names = ["checkpoint.pth.tar"]
    elif args.epoch != 0:
        names = [f"best_val_checkpoint_{args.epoch}epoch.pth.tar", f"checkpoint_{args.epoch}epoch.pth.tar", f"best_val_{args.epoch}.pth.tar"]
    else:
        names = ["best_val_checkpoint.pth.tar"]
    for n in names:
        if os.path.exists(os.path.join(d, n)):
            return os.path.join(d, n)
    raise FileNotFoundError(f"Checkpoint not found: {names} under {d}")


def run(args, logger=None):
    """evaluate_jta.py:555-625: load the checkpoint and its config, the LocoVal network, the split, and evaluate."""
    import os
    from torch.utils.data import DataLoader
    from ..learning.value_pose_net import ValuePoseNet
    from .train_jta import load_checkpoint, load_config
    if getattr(args, "refine_steps", 0) > 0 and not args.valueloss:
        raise SystemExit("evaluate_jta --refine_steps: the refinement ascends the LocoVal value, which --valueloss loads; pass --valueloss")
    dev = f"cuda:{torch.cuda.current_device()}"
    ckpt_name = find_checkpoint(args)
    if logger is not None:
        logger.info(f"Loading checkpoint from {ckpt_name}")
    config = torch.load(ckpt_name, map_location="cpu")["config"]
    new_cfg = load_config(f"configs/{args.dataset}_all_visual_cues.yaml", exp_name=args.exp_name + "_eval", dataset_name=args.dataset.upper(),
                          out_root=args.out_root)
    config["DEVICE"], config["NOISY_TRAJ"], config["MULTI_MODAL"] = dev, args.noisy_traj, args.multi_modal
    config["MODEL"]["value_threshold"] = args.filter_threshold
    valuenet = None
    if args.valueloss:
        valuenet = ValuePoseNet(use_pose=not args.no_pose, use_vel=not args.no_vel)
        vck = config["MODEL"].get("valuenet_checkpoint") or new_cfg["MODEL"].get("valuenet_checkpoint", "")
        if vck:
            valuenet.load_state_dict(torch.load(vck, map_location="cpu"))
        elif logger is not None:
            logger.info("No checkpoint provided for valuenet. Using random weights.")
        valuenet = valuenet.to(dev).eval()
    if args.dataset == "jta":
        from .dataset_jta import collate_batch, create_dataset
        from .model_jta import create_model
    else:
        from .dataset_jrdb import collate_batch, create_dataset
        from .model_jrdb import create_model
    model = create_model(config, logger)
    load_checkpoint(model, ckpt_name, strict=True)
    in_F, out_F = config["TRAIN"]["input_track_size"], config["TRAIN"]["output_track_size"]
    dataset = create_dataset(config["DATA"]["train_datasets"][0], logger, split=args.split, track_size=in_F + out_F, track_cutoff=in_F,
                             preprocessed=config["DATA"]["preprocessed"], root=args.data_root)
    bs = new_cfg["TRAIN"]["batch_size"] * 10
    loader = DataLoader(dataset, batch_size=bs, num_workers=0, shuffle=False, collate_fn=collate_batch)
    out = {}
    for obs_i in ([1, 2, 3, 4, 5, 6, 7, 8, 0] if args.all_frames else [args.limit_obs]):
        if logger is not None:
            logger.info(f"Evaluating with {9 if obs_i == 0 else obs_i} frames")
        collector = PredTrajCollector(args.save_pred_modes) if getattr(args, "save_pred_trajs", "") else None
        out[obs_i] = evaluate_ade_fde(model, valuenet, args.split, args.modality, loader, bs, config, logger, args.exp_name, return_all=True,
                                      limit_obs=obs_i, dataset=args.dataset, pred_trajs=collector, refine_steps=getattr(args, "refine_steps", 0),
                                      refine_lr=getattr(args, "refine_lr", 1e-4), refine_anchor=getattr(args, "refine_anchor", 0.0),
                                      refine_modes=getattr(args, "refine_modes", "all"))
        if collector is not None:                                                 # (--all_frames: the last pass, all 9 frames, stays)
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 else None
            path = collector.save(args.save_pred_trajs + ("" if rank is None else f".rank{rank}"))      # a rank holds its own batches
            if logger is not None:
                logger.info(f"Saved {len(collector.entries)} predicted paths to {path}")
    return out


if __name__ == "__main__":
    import random
    from .. import _lib, configure_runtime
    from ..dist import init_from_env
    configure_runtime()                                  # entry point: 16 hardware queues, ahead of the first GPU call
    from .train_jta import create_logger
    _lib.require_device()
    a = build_arg_parser().parse_args()
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    _rank, local_rank, _world = init_from_env("nccl")
    torch.cuda.set_device(local_rank)
    import os
    logdir = os.path.join(a.out_root, a.dataset.upper(), a.exp_name, "eval_logs")
    os.makedirs(logdir, exist_ok=True)
    run(a, create_logger(logdir))

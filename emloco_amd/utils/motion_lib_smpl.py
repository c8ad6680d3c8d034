"""MotionLib over AMASS pickles -- the reference's motion data path (pacer/pacer/utils/motion_lib_smpl.py:84-131,176-363).

On-disk format (scripts/data_process/convert_amass_isaac.py:309-317, read with joblib): a dict  clip name -> {
    "pose_quat_global" (T, 24, 4) global body rotations xyzw in the humanoid's body order,
    "root_trans_offset" (T, 3) root translation, "pose_aa" (T, 72) SMPL axis-angle pose, "beta" (16,), "gender", "fps" }.
Per clip the reference builds a poselib SkeletonMotion on the env's skeleton (`load_motion_with_skeleton`): local rotations from the
global ones, global translations by forward kinematics over the skeleton's local translations, global linear velocities as
gaussian-filtered np.gradient of the translations and angular velocities as gaussian-filtered quaternion differences
(poselib skeleton3d.py:1249-1272), joint velocities from successive local rotations (:44-67); the frames of all clips are concatenated into
the cache `get_motion_state_smpl` blends from (:334-363).  The same here, restated on torch / numpy / scipy (host-side data
preparation, as in the reference), pinned by tests/golden/motion_amass.npz = the reference's own loader run on two clips in that format.

What is NOT here: `fix_height` through the SMPL mesh (:70-82: needs the licensed SMPL model).  The reset path places a sampled pose on
the ground by its lowest collision point instead (env/tasks/humanoid_amp.py `_lowest_point`), clip by clip at reset time,
so a clip's stored height is only a starting point.  `masterfoot` skeletons are not part of this path.
"""
import numpy as np
import torch

from .motion_lib_synthetic import MotionLibBase


def _qmul(a, b):
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                        w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def _qinv(q):
    return torch.cat([-q[..., :3], q[..., 3:]], -1)


def _qnormalize(q):                 # poselib quat_normalize: real part made non-negative, unit length
    q = torch.where(q[..., 3:] < 0, -q, q)
    return q / q.norm(dim=-1, keepdim=True).clamp(min=1e-9)


def _qmul_norm(a, b):
    return _qnormalize(_qmul(a, b))


def _qrot(q, v):                    # poselib quat_rotate: q (v, 0) q^-1
    return _qmul(_qmul(q, torch.cat([v, torch.zeros_like(v[..., :1])], -1)), _qinv(q))[..., :3]


def _angle_axis(q):                 # poselib quat_angle_axis: angle in [0, pi] from the real part, axis = normalised imaginary part
    angle = (2 * q[..., 3] ** 2 - 1).clamp(-1, 1).arccos()
    axis = q[..., :3] / q[..., :3].norm(dim=-1, keepdim=True).clamp(min=1e-9)
    return angle, axis


def clip_cache(clip, local_translation, parents):
    """One clip on one skeleton -> the per-frame arrays of the reference's SkeletonMotion (float64): global translation (T,24,3),
    global rotation, local rotation (T,24,4), global velocity, global angular velocity (T,24,3), joint velocities (T,23,3), fps."""
    from scipy.ndimage import gaussian_filter1d
    gq = torch.as_tensor(np.asarray(clip["pose_quat_global"]), dtype=torch.float64)
    trans = torch.as_tensor(np.asarray(clip["root_trans_offset"]), dtype=torch.float64)
    fps = float(clip.get("fps", 30))
    dt = 1.0 / fps
    T, J, _ = gq.shape
    lt = torch.as_tensor(np.asarray(local_translation), dtype=torch.float64)
    lq = torch.zeros_like(gq)
    gp = torch.zeros(T, J, 3, dtype=torch.float64)
    for b in range(J):
        p = int(parents[b])
        if p < 0:
            lq[:, b], gp[:, b] = gq[:, b], trans
        else:
            lq[:, b] = _qmul_norm(_qinv(gq[:, p]), gq[:, b])
            gp[:, b] = gp[:, p] + _qrot(gq[:, p], lt[b].expand(T, 3))
    gv = torch.from_numpy(gaussian_filter1d(np.gradient(gp.numpy(), axis=0), 2, axis=0, mode="nearest") / dt)
    dq = torch.zeros_like(gq)
    dq[..., 3] = 1.0
    dq[:-1] = _qmul_norm(gq[1:], _qinv(gq[:-1]))
    ang, ax = _angle_axis(dq)
    gav = torch.from_numpy(gaussian_filter1d((ax * ang.unsqueeze(-1) / dt).numpy(), 2, axis=0, mode="nearest"))
    dl = _qmul_norm(_qinv(lq[:-1]), lq[1:])
    a2, x2 = _angle_axis(dl)
    dv = (x2 * a2.unsqueeze(-1) / dt)[:, 1:]
    dv = torch.cat([dv, dv[-1:]], 0)
    return dict(gts=gp, grs=gq, lrs=lq, gvs=gv, gavs=gav, dvs=dv, fps=fps)


def gaussian_taps(sigma=2.0, radius=8):
    """The weights scipy's gaussian_filter1d(sigma, truncate=4) applies, computed in float64 and normalised, as float32: what
    emloco_motion_build (include/emloco_task.h) takes as its filter."""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * (x / sigma) ** 2)
    return (w / w.sum()).astype(np.float32)


BUILD_MODES = ("host", "device")
FRAME_KEYS = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")
_FRAME_SHAPES = dict(gts=(24, 3), grs=(24, 4), lrs=(24, 4), gvs=(24, 3), gavs=(24, 3), dvs=(69,), _motion_aa=(72,), _quat_in=(24, 4), _trans_in=(3,))
CAPACITY_FACTOR = 1.5               # spare frame rows of the device build's arrays over its first draw


class MotionLib(MotionLibBase):
    """`MotionLib(motion_file, key_body_ids, device)` + `load_motions(skeleton_trees, gender_betas, limb_weights, random_sample,
    start_idx)` (motion_lib_smpl.py:176-363): one clip per skeleton (= per env), drawn from the pickle with `_sampling_prob`, each
    built on ITS skeleton.  A skeleton is anything with `.joint_off` (24, 3) and `.parent` (24,) -- emloco_amd.model.HumanoidModel --
    or a (local_translation, parent_indices) pair."""

    def __init__(self, motion_file, key_body_ids, device, fix_height=False, masterfoot_conifg=None, min_length=-1, build="host"):
        import joblib
        if build not in BUILD_MODES:
            raise ValueError(f"build must be one of {BUILD_MODES}, not {build!r}")
        self.build = build              # how load_motions builds the clip cache unless told otherwise
        self.num_reallocations = 0      # device builds whose draw did not fit the frame arrays (their addresses changed)
        self._frame_capacity = 0
        self._store = {}
        self._build_events = None
        if masterfoot_conifg is not None:
            raise NotImplementedError("masterfoot skeletons are not part of this path")
        if fix_height:
            raise NotImplementedError("fix_height needs the licensed SMPL mesh; the reset path grounds a sampled pose by its lowest "
                                      "collision point instead (humanoid_amp.py _lowest_point): pass fix_height=False")
        self._device = torch.device(device)
        self._key_body_ids = torch.as_tensor(key_body_ids, dtype=torch.long, device=self._device)
        data = motion_file if isinstance(motion_file, dict) else joblib.load(motion_file)
        if min_length != -1:
            data = {k: v for k, v in data.items() if len(v["pose_quat_global"]) >= min_length}
        self._motion_data_list = list(data.values())
        self._motion_data_keys = np.array(list(data.keys()))
        self._num_unique_motions = len(self._motion_data_list)
        if self._num_unique_motions == 0:
            raise ValueError("the motion file holds no clip (after the min_length filter)")
        self._curr_motion_ids = None
        self._termination_history = torch.zeros(self._num_unique_motions)
        self._success_rate = torch.zeros(self._num_unique_motions)
        self._sampling_history = torch.zeros(self._num_unique_motions)
        self._sampling_prob = torch.ones(self._num_unique_motions) / self._num_unique_motions

    @staticmethod
    def _skeleton(s):
        if hasattr(s, "joint_off"):
            return np.asarray(s.joint_off, np.float64), np.asarray(s.parent)
        lt, par = s
        return np.asarray(lt, np.float64), np.asarray(par)

    def load_motions(self, skeleton_trees, gender_betas=None, limb_weights=None, random_sample=True, start_idx=0, build=None):
        """`build`: "host" -- every (clip, skeleton) pair through `clip_cache` in float64 -- or "device" -- the drawn clips' raw frames
        uploaded as float32 and built by emloco_motion_build; None: the library's mode (`self.build`).  Both leave the same attributes."""
        build = self.build if build is None else build
        if build not in BUILD_MODES:
            raise ValueError(f"build must be one of {BUILD_MODES}, not {build!r}")
        if build == "device":
            return self._load_motions_device(skeleton_trees, gender_betas, limb_weights, random_sample, start_idx)
        n = len(skeleton_trees)
        if random_sample:
            ids = torch.multinomial(self._sampling_prob, num_samples=n, replacement=True)
        else:
            ids = torch.clip(torch.arange(n) + start_idx, 0, self._num_unique_motions - 1)
        self._curr_motion_ids = ids
        self._sampling_batch_prob = self._sampling_prob[ids] / self._sampling_prob[ids].sum()
        keys = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")
        parts = {k: [] for k in keys}
        lens, fpss, nfr, aa, bodies = [], [], [], [], []
        built = {}                      # (clip, skeleton) pairs repeat when envs share a body shape: build each once
        for j, i in enumerate(ids.tolist()):
            clip = self._motion_data_list[i]
            lt, par = self._skeleton(skeleton_trees[j])
            key = (i, lt.tobytes())
            if key not in built:
                built[key] = clip_cache(clip, lt, par)
            c = built[key]
            for k in keys:
                parts[k].append(c[k].reshape(c[k].shape[0], -1, c[k].shape[-1]) if k != "dvs" else c[k].reshape(c[k].shape[0], -1))
            T = c["gts"].shape[0]
            nfr.append(T); fpss.append(c["fps"]); lens.append((T - 1) / c["fps"])
            if "beta" in clip:
                aa.append(np.asarray(clip["pose_aa"], np.float64).reshape(-1, 72))
                bodies.append(torch.as_tensor(np.asarray(gender_betas[j]), dtype=torch.float32) if gender_betas is not None else torch.zeros(17))
            else:
                aa.append(np.zeros((T, 72)))
                bodies.append(torch.zeros(17))
        dev = self._device
        for k in keys:
            setattr(self, k, torch.cat(parts[k]).float().to(dev).contiguous())
        self._motion_lengths = torch.tensor(lens, dtype=torch.float32, device=dev)
        self._motion_fps = torch.tensor(fpss, dtype=torch.float32, device=dev)
        self._motion_dt = 1.0 / self._motion_fps
        self._motion_num_frames = torch.tensor(nfr, dtype=torch.long, device=dev)
        self._motion_aa = torch.tensor(np.concatenate(aa), dtype=torch.float32, device=dev)
        self._motion_bodies = torch.stack(bodies).to(dev).float()
        self._motion_limb_weights = (torch.as_tensor(limb_weights).float().to(dev) if limb_weights is not None else torch.zeros(n, 10, device=dev))
        shifted = self._motion_num_frames.roll(1)
        shifted[0] = 0
        self.length_starts = shifted.cumsum(0)
        self._motion_weights = self._sampling_batch_prob.to(dev).float()
        self._num_motions = n
        self.motion_ids = torch.arange(n, dtype=torch.long, device=dev)
        return self

    # ------------------------------------------------------------------ the device build
    def _clip_frames32(self, i):
        """clip i's raw frames as the kernel takes them: float32, contiguous (no copy where the pickle holds them so)"""
        clip = self._motion_data_list[i]
        quat = np.ascontiguousarray(np.asarray(clip["pose_quat_global"]), dtype=np.float32).reshape(-1, 24, 4)
        trans = np.ascontiguousarray(np.asarray(clip["root_trans_offset"]), dtype=np.float32).reshape(-1, 3)
        aa = (np.ascontiguousarray(np.asarray(clip["pose_aa"]), dtype=np.float32).reshape(-1, 72) if "beta" in clip
              else np.zeros((quat.shape[0], 72), np.float32))
        if quat.shape[0] != trans.shape[0] or quat.shape[0] != aa.shape[0]:
            raise ValueError(f"clip {self._motion_data_keys[i]}: rotations, translations and poses differ in their frame counts")
        return quat, trans, aa, float(clip.get("fps", 30))

    def _frame_rows(self, F):
        """The frame arrays with room for F rows: the ones in use when F fits their capacity -- their addresses stay valid -- and new
        ones with CAPACITY_FACTOR x F rows otherwise.  True when they were (re)allocated."""
        if F <= self._frame_capacity:
            return False
        if self._frame_capacity:
            self.num_reallocations += 1
        self._frame_capacity = int(np.ceil(CAPACITY_FACTOR * F))
        self._store = {k: torch.zeros((self._frame_capacity,) + s, dtype=torch.float32, device=self._device) for k, s in _FRAME_SHAPES.items()}
        return True

    def _set_rows(self, name, value):
        """a per-motion array: rewritten in place when its shape is unchanged (its address stays valid)"""
        old = getattr(self, name, None)
        if isinstance(old, torch.Tensor) and old.shape == value.shape and old.dtype == value.dtype and old.device == value.device:
            old.copy_(value)
        else:
            setattr(self, name, value.contiguous())

    def _load_motions_device(self, skeleton_trees, gender_betas, limb_weights, random_sample, start_idx):
        from .. import _lib
        dev = self._device
        if dev.type != "cuda":
            raise _lib.EmlocoError(f'load_motions(build="device") builds the clip cache with a HIP kernel: it needs a GPU device, not {dev}; '
                                   'use build="host" there')
        lib = _lib.require_device()
        n = len(skeleton_trees)
        if random_sample:
            ids = torch.multinomial(self._sampling_prob, num_samples=n, replacement=True)
        else:
            ids = torch.clip(torch.arange(n) + start_idx, 0, self._num_unique_motions - 1)
        self._curr_motion_ids = ids
        self._sampling_batch_prob = self._sampling_prob[ids] / self._sampling_prob[ids].sum()
        # the skeleton table: one row per distinct set of joint offsets
        skel_rows, skel_of, skel_id, parent = [], {}, np.zeros(n, np.int32), None
        for j, s in enumerate(skeleton_trees):
            lt, par = self._skeleton(s)
            par = np.asarray(par, np.int32)
            if lt.shape != (24, 3) or par.shape != (24,) or (parent is not None and not np.array_equal(par, parent)):
                raise ValueError("the device build takes 24-body skeletons that share one parent list")
            parent = par
            key = lt.tobytes()
            if key not in skel_of:
                skel_of[key] = len(skel_rows)
                skel_rows.append(lt.astype(np.float32))
            skel_id[j] = skel_of[key]
        frames = [self._clip_frames32(i) for i in ids.tolist()]
        nfr = np.asarray([f[0].shape[0] for f in frames], np.int32)
        if int(nfr.min()) < 2:
            raise ValueError("a clip needs at least 2 frames")
        fps = np.asarray([f[3] for f in frames], np.float32)
        start = np.zeros(n, np.int64)
        np.cumsum(nfr[:-1], out=start[1:])
        F = int(nfr.sum())
        self.reallocated = self._frame_rows(F)
        st = self._store
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        # only the drawn clips travel: their frames concatenated, env after env
        st["_quat_in"][:F].copy_(torch.from_numpy(np.concatenate([f[0] for f in frames])))
        st["_trans_in"][:F].copy_(torch.from_numpy(np.concatenate([f[1] for f in frames])))
        st["_motion_aa"][:F].copy_(torch.from_numpy(np.concatenate([f[2] for f in frames])))
        self._set_rows("_motion_num_frames", torch.from_numpy(nfr.astype(np.int64)).to(dev))
        self._set_rows("length_starts", torch.from_numpy(start).to(dev))
        self._set_rows("_motion_fps", torch.from_numpy(fps).to(dev))
        d_nfr32, d_skel = torch.from_numpy(nfr).to(dev), torch.from_numpy(skel_id).to(dev)
        d_lt = torch.from_numpy(np.ascontiguousarray(np.stack(skel_rows))).to(dev)
        ev[1].record()
        taps = gaussian_taps()
        rc = lib.emloco_motion_build(n, len(skel_rows), F, st["_quat_in"].data_ptr(), st["_trans_in"].data_ptr(), self.length_starts.data_ptr(),
                                     d_nfr32.data_ptr(), self._motion_fps.data_ptr(), d_skel.data_ptr(), start.ctypes.data, nfr.ctypes.data,
                                     skel_id.ctypes.data, d_lt.data_ptr(), parent.ctypes.data, taps.ctypes.data,
                                     *[st[k].data_ptr() for k in FRAME_KEYS], 0, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "emloco_motion_build")
        ev[2].record()
        self._build_events = ev
        for k in FRAME_KEYS + ("_motion_aa",):
            setattr(self, k, st[k][:F])                    # the live rows: a view at the storage's address
        self._set_rows("_motion_lengths", torch.from_numpy(((nfr - 1) / fps.astype(np.float64)).astype(np.float32)).to(dev))
        self._set_rows("_motion_dt", 1.0 / self._motion_fps)
        bodies = []
        for j, i in enumerate(ids.tolist()):
            has_beta = "beta" in self._motion_data_list[i] and gender_betas is not None
            bodies.append(torch.as_tensor(np.asarray(gender_betas[j].cpu() if isinstance(gender_betas[j], torch.Tensor) else gender_betas[j]),
                                          dtype=torch.float32) if has_beta else torch.zeros(17))
        self._set_rows("_motion_bodies", torch.stack(bodies).to(dev).float())
        self._set_rows("_motion_limb_weights", torch.as_tensor(limb_weights).float().to(dev) if limb_weights is not None else torch.zeros(n, 10, device=dev))
        self._set_rows("_motion_weights", self._sampling_batch_prob.to(dev).float())
        self._set_rows("motion_ids", torch.arange(n, dtype=torch.long, device=dev))
        self._num_motions = n
        return self

    def build_times(self):
        """(upload ms, kernel ms) of the last device build from its HIP events; waits for the build to finish"""
        if self._build_events is None:
            return None
        e0, e1, e2 = self._build_events
        e2.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    def get_motion_files(self, motion_ids):
        return self._motion_data_keys[self._curr_motion_ids[torch.as_tensor(motion_ids).cpu()]]

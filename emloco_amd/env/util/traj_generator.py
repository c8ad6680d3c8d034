"""TrajGenerator: the per-env target polyline (101 vertices) the humanoid follows.

Host-side mirror of pacer/pacer/env/util/traj_generator.py (class TrajGenerator :19-296): same constructor,
`reset`, `calc_pos`, `show_inverted`, `get_*` methods and the same order of random draws, so a seeded CPU run
reproduces the reference's vertices (pinned by tests/test_host_logic.py against tests/golden/traj_reset_*.npz).
`reset` runs once per episode; the per-step sampling (`calc_pos`, :278-296) is done on the device by the fused
post-physics kernel and is kept here for host callers.

Real-world paths (`flags.real_path`): `traj_data` is a list of dicts {id: {'traj': (>=101,3) array, 'pose': ...}}
in the format load_jta_traj.py:109-114 writes; pass it in (or a pickle path) instead of the hard-coded files
(`python -m emloco_amd.predictor.export_trajs` writes them).

Predicted paths (`flags.pred_path`, :53-54,163-175): `pred_traj_data` is a dict {key: {'coord_dense': (>=101,3) array, ...}} or the path
of its pickle (`evaluate_jta --save_pred_trajs` writes one; default: the reference's data/traj/traj_pred_data.pkl).  Every env walks one
row, sampled without replacement, moved so that its first vertex sits on the env's root position.
"""
import os
import random

import numpy as np
import torch

PRED_TRAJ_FILE = "data/traj/traj_pred_data.pkl"          # traj_generator.py:54


def load_pred_traj_data(src=None):
    """The table of predicted paths: a dict as it is, a pickle path loaded; a missing file is an error that names it."""
    src = PRED_TRAJ_FILE if src is None else src
    if isinstance(src, (str, os.PathLike)):
        if not os.path.isfile(src):
            raise FileNotFoundError(f"--pred_path: the predicted-path table {src} does not exist (--pred_traj_file PATH or "
                                    "cfg['env']['pred_traj_data'] names it; `evaluate_jta --save_pred_trajs` writes one)")
        import joblib
        src = joblib.load(src)
    if not isinstance(src, dict) or not all("coord_dense" in v for v in src.values()):
        raise ValueError("--pred_path: the predicted-path table is a dict {key: {'coord_dense': (>=101, 3) array}}")
    return src


class TrajGenerator():
    def __init__(self, num_envs, episode_dur, num_verts, device, dtheta_max, speed_min, speed_max, accel_max,
                 sharp_turn_prob, motion_lib=None, hybridInitProb=0.5, flags=None, traj_data=None, pred_traj_data=None):
        self._device = device
        self._dt = episode_dur / (num_verts - 1)
        self._dtheta_max = dtheta_max
        self._speed_min = speed_min
        self._speed_max = speed_max
        self._accel_max = accel_max
        self._sharp_turn_prob = sharp_turn_prob
        self._motion_lib = motion_lib
        self._hybrid_init_prob = hybridInitProb
        self._flags = flags
        self.inverted = torch.zeros(num_envs, dtype=torch.bool, device=self._device)
        self._verts_flat = torch.zeros((num_envs * num_verts, 3), dtype=torch.float32, device=self._device)
        self._verts = self._verts_flat.view((num_envs, num_verts, 3))
        self.traj_data = []
        if self._flags is not None and self._flags.real_path:
            if traj_data is None:
                raise ValueError("flags.real_path needs traj_data (list of {id: {'traj': array}} dicts or pickle paths)")
            for d in traj_data:
                if isinstance(d, str):
                    import joblib
                    d = joblib.load(d)
                self.traj_data.append(d)
        self.traj_pred_data = None
        self.last_pred_rows = None              # table row (position in the table's key order) every env walked at its last reset
        if self._flags is not None and getattr(self._flags, "pred_path", False):
            self.traj_pred_data = load_pred_traj_data(pred_traj_data)
            self.last_pred_rows = torch.full((num_envs,), -1, dtype=torch.int64)
        self.pred_row_log = None                # a list: every reset under pred_path appends (env ids, table rows) as int64 arrays
        self.heading = torch.zeros(num_envs, 1)

    # ------------------------------------------------------------------ random draws, in the reference's order (:63-78)
    def _draw(self, n, num_verts):
        dev = self._device
        return dict(
            r_dtheta=torch.rand([n, num_verts - 1], device=dev),
            r_dtheta_sharp=torch.rand([n, num_verts - 1], device=dev),
            bern_sharp=torch.bernoulli(self._sharp_turn_prob * torch.ones([n, num_verts - 1], device=dev)),
            r_heading=torch.rand([n], device=dev),
            r_dspeed=torch.rand([n, num_verts - 1], device=dev),
            r_speed0=torch.rand([n], device=dev),
        )

    def _polyline(self, d, init_pos, root_vel):
        """Random-walk polyline from the draws (:63-118)."""
        dtheta = 2 * d["r_dtheta"] - 1.0
        dtheta *= self._dtheta_max * self._dt
        dtheta_sharp = np.pi * (2 * d["r_dtheta_sharp"] - 1.0)
        sharp_mask = d["bern_sharp"] == 1.0
        dtheta[sharp_mask] = dtheta_sharp[sharp_mask]
        dtheta[:, 0] = np.pi * (2 * d["r_heading"] - 1.0)
        dspeed = 2 * d["r_dspeed"] - 1.0
        dspeed *= self._accel_max * self._dt
        dspeed[:, 0] = (self._speed_max - self._speed_min) * d["r_speed0"] + self._speed_min
        speed = torch.zeros_like(dspeed)
        speed[:, 0] = dspeed[:, 0]
        for i in range(1, dspeed.shape[-1]):
            speed[:, i] = torch.clip(speed[:, i - 1] + dspeed[:, i], self._speed_min, self._speed_max)
        f = self._flags
        if f.fixed_path:
            dtheta[:, :] = 0
            if len(dtheta) > 1:
                dtheta[1, 0] = -np.pi
            speed[:] = (self._speed_min + self._speed_max) / 2
        if f.slow:
            speed[:] = speed / 4
        if f.adjust_root_vel:
            root_speed = torch.norm(root_vel[:, :2], dim=-1)
            speed_ratio = root_speed / speed[:, 0]
            speed = torch.clip(speed_ratio.unsqueeze(-1) * speed, self._speed_min, self._speed_max)
        dtheta = torch.cumsum(dtheta, dim=-1)
        seg_len = speed * self._dt
        dpos = torch.stack([torch.cos(dtheta), -torch.sin(dtheta), torch.zeros_like(dtheta)], dim=-1)
        dpos *= seg_len.unsqueeze(-1)
        dpos[..., 0, 0:2] += init_pos[..., 0:2]
        return torch.cumsum(dpos, dim=-2)

    def reset(self, env_ids, init_pos, root_vel=None, motion_ids=None, motion_times=None, draws=None):
        n = len(env_ids)
        if n == 0:
            return
        f = self._flags
        num_verts = self.get_num_verts()
        d = draws if draws is not None else self._draw(n, num_verts)
        vert_pos = self._polyline(d, init_pos, root_vel)
        self._verts[env_ids, 0, 0:2] = init_pos[..., 0:2]
        self._verts[env_ids, 1:] = vert_pos

        if f.real_path:                                                             # :121-160
            real_prob = d.get("r_real", None)
            if real_prob is None:
                real_prob = torch.rand(n, device=self._device)
            real_mask = real_prob > self._hybrid_init_prob
            real_num = int(torch.sum(real_mask))
            sizes = [len(t) for t in self.traj_data]
            rids = d.get("real_rids", None)                 # explicit sample (tests replay the reference's / the device's)
            if rids is None:
                rids = random.sample(range(sum(sizes)), real_num)
            rids = [int(r) for r in rids]
            assert len(rids) == real_num
            traj = torch.zeros([real_num, num_verts, 3], device=self._device)
            for i, rid in enumerate(rids):
                k = 0
                while rid >= sizes[k]:
                    rid -= sizes[k]
                    k += 1
                src = self.traj_data[k]
                item = src[rid] if not isinstance(src, dict) or rid in src else src[list(src.keys())[rid]]
                traj[i] = torch.as_tensor(np.asarray(item["traj"]), dtype=torch.float32)[:num_verts]
            traj[..., 0:2] = traj[..., 0:2] - traj[..., 0, 0:2].unsqueeze(1)
            if f.adjust_root_vel:
                init_speed = torch.clamp(torch.norm(traj[:, 1] - traj[:, 0], dim=-1), min=self._speed_min * self._dt)
                root_speed = torch.norm(root_vel[real_mask, :2].clone(), dim=-1)
                ratio = root_speed.div(init_speed) * self._dt
                traj[..., 0:2] = ratio.view(-1, 1, 1) * traj[..., 0:2]
            traj[..., 0:2] += init_pos[real_mask, 0:2].unsqueeze(1)
            self._verts[env_ids[real_mask]] = traj

        elif getattr(f, "pred_path", False):                                        # :163-175
            rows = d.get("pred_rids", None)                 # explicit sample: positions in the table's key order
            if rows is None:
                rows = self._sample_pred_rows(n)
            rows = [int(r) for r in rows]
            assert len(rows) == n
            keys = list(self.traj_pred_data.keys())
            traj = torch.stack([torch.from_numpy(np.asarray(self.traj_pred_data[keys[r]]["coord_dense"]))[:num_verts] for r in rows],
                               dim=0).to(self._device).float()
            traj[..., 0:2] = traj[..., 0:2] - (traj[..., 0, 0:2] - init_pos[..., 0:2])[:, None]      # no speed rescaling (:174)
            self._verts[env_ids] = traj
            self._note_pred_rows(env_ids, rows)

        if f.init_heading:                                                          # :176-235
            verts = self._verts[env_ids].clone()
            dinit = verts[:, 1, :2] - verts[:, 0, :2]
            root_mag = torch.sqrt(torch.sum(root_vel ** 2, dim=1))
            dinit_mag = torch.sqrt(torch.sum(dinit ** 2, dim=1))
            root_rot = torch.where(root_mag > 0, torch.atan2(root_vel[..., 1], root_vel[..., 0]), torch.zeros_like(root_vel[..., 0]))
            init_heading = torch.where(dinit_mag > 0, torch.atan2(dinit[..., 1], dinit[..., 0]), torch.zeros_like(dinit[..., 0]))
            rot_diff = init_heading - root_rot
            if f.heading_inversion:
                r_inv = d.get("r_inversion", None)
                if r_inv is None:
                    r_inv = torch.rand(n, device=self._device)
                inv = r_inv > 0.5
                self.inverted[env_ids[inv]] = True
                self.inverted[env_ids[~inv]] = False
                rot_diff[inv] = init_heading[inv] - root_rot[inv] + np.pi
            origin = verts[:, 0, 0:2].clone().unsqueeze(1).expand(-1, num_verts, 2)
            verts[:, :, 0:2] -= origin
            c, s = torch.cos(rot_diff), torch.sin(rot_diff)
            R = torch.stack([c, -s, s, c], dim=-1).view(-1, 2, 2)
            verts[:, :, 0:2] = torch.bmm(verts[:, :, 0:2].clone(), R)
            verts[:, :, 0:2] += origin
            self._verts[env_ids] = verts
        if f.add_noise:
            self._verts[env_ids] += torch.randn_like(self._verts[env_ids]) * 0.5

    def _sample_pred_rows(self, n):
        """n distinct rows of the predicted-path table, as the reference's random.sample(traj_data.keys(), n) (:165)."""
        size = len(self.traj_pred_data)
        if n > size:
            raise ValueError(f"--pred_path: {n} envs reset at once but the predicted-path table holds {size} rows "
                             "(rows are sampled without replacement: the table needs at least as many rows as envs)")
        return random.sample(range(size), n)

    def _note_pred_rows(self, env_ids, rows):
        ids = torch.as_tensor(env_ids).cpu().to(torch.int64)
        rows = torch.as_tensor(rows, dtype=torch.int64)
        self.last_pred_rows[ids] = rows
        if self.pred_row_log is not None:
            self.pred_row_log.append((ids.numpy().copy(), rows.numpy().copy()))

    def pred_rows(self):
        """The predicted paths as one (n_rows, num_verts, 3) float32 table in the table's key order."""
        nv = self.get_num_verts()
        return np.stack([np.asarray(v["coord_dense"], np.float32)[:nv] for v in self.traj_pred_data.values()])

    def real_rows(self):
        """The real paths as one (n_real, num_verts, 3) float32 table, datasets concatenated in order (row = the id
        `random.sample(range(jta_num + jrdb_num), ...)` indexes, traj_generator.py:128-143)."""
        rows = []
        for src in self.traj_data:
            vals = src.values() if isinstance(src, dict) else src
            rows += [np.asarray(v["traj"], np.float32)[:self.get_num_verts()] for v in vals]
        return np.stack(rows) if rows else np.zeros((0, self.get_num_verts(), 3), np.float32)

    def reset_on_device(self, env_ids, init_pos, root_vel, rnd=None, real_pick=None, real_pick_key=0):
        """`reset` as one kernel launch (emloco_task_traj_reset, reset_kernels.hip): random rows `rnd` [n][RESET_RND]
        uniform in [0, 1) laid out as include/emloco_task.h describes (drawn with torch.rand when omitted), real-path rows
        from `real_pick` (int32 [n]) or the keyed permutation.  Needs the gfx950 library and CUDA tensors.
        `flags.pred_path` goes through the same kernel's real-path table: every env takes a row (hybrid_prob -1), the speed rescaling
        is off (:163-175); rows from `real_pick` or, when omitted, sampled on the host as `reset` samples them.  The reference places a
        predicted row as row - (first - root) (:174), the kernel a table row as (row - first) + root: in float32 the two differ by an
        ulp per vertex, which the heading block magnifies by the path's vertex count.  So the rows of the call are placed on the
        device in the reference's order and handed over as the call's table with their own first vertex as the root: the kernel's
        (v - v0) + v0 gives v back, and what reaches the heading block is what `reset` has there, bit for bit."""
        import ctypes as C
        from ... import _lib as L
        from ...sim import current_stream_handle
        lib = L.require_device()
        n = len(env_ids)
        if n == 0:
            return
        f = self._flags
        dev = self._verts.device
        pred = bool(getattr(f, "pred_path", False)) and not f.real_path          # (`reset`: the real-path branch comes first)
        if f.fixed_path or f.slow or f.add_noise:
            raise NotImplementedError("reset_on_device: fixed_path / slow / add_noise stay on the host path (reset)")
        if rnd is None:
            rnd = torch.rand((n, L.RESET_RND), device=dev)
        if getattr(self, "_real_dev", None) is None and (f.real_path or pred):
            self._real_dev = torch.from_numpy(self.pred_rows() if pred else self.real_rows()).to(dev).contiguous()
        if pred and real_pick is None:
            real_pick = torch.as_tensor(self._sample_pred_rows(n), dtype=torch.int32)
        table = getattr(self, "_real_dev", None)
        if pred:
            self._note_pred_rows(env_ids, real_pick.cpu().tolist())
            root = init_pos[:, :3].float().to(dev)
            table = self._real_dev[real_pick.to(dev).long()]                       # (n, num_verts, 3), a copy
            table[..., 0:2] = table[..., 0:2] - (table[..., 0, 0:2] - root[..., 0:2])[:, None]      # :174, the reference's order
            table = table.contiguous()
            real_pick = torch.arange(n, dtype=torch.int32, device=dev)
            init_pos = torch.cat([table[:, 0, 0:2], root[:, 2:3]], dim=1)
        if getattr(self, "_inverted_u8", None) is None:
            self._inverted_u8 = torch.zeros(self.get_num_envs(), dtype=torch.uint8, device=dev)
        self._inverted_u8.copy_(self.inverted.to(torch.uint8))
        b = L.ResetBufs()
        fl = (L.RESET_INIT_HEADING if f.init_heading else 0) | (L.RESET_ADJUST_ROOT_VEL if f.adjust_root_vel else 0)
        fl |= L.RESET_HEADING_INVERSION if (f.init_heading and f.heading_inversion) else 0
        fl |= L.RESET_REAL_PATH if (f.real_path or pred) else 0
        if pred:
            fl &= ~L.RESET_ADJUST_ROOT_VEL
        b.flags, b.n_real = fl, (int(table.shape[0]) if (f.real_path or pred) else 0)
        b.vert_dt, b.dtheta_max, b.speed_min, b.speed_max = self._dt, self._dtheta_max, self._speed_min, self._speed_max
        b.accel_max, b.sharp_prob, b.hybrid_prob = self._accel_max, self._sharp_turn_prob, (-1.0 if pred else self._hybrid_init_prob)
        b.real_traj = table.data_ptr() if (f.real_path or pred) else None
        b.traj_verts, b.inverted = self._verts.data_ptr(), self._inverted_u8.data_ptr()
        keep = [rnd.contiguous(), env_ids.to(dev).to(torch.int32).contiguous(), init_pos[:, :3].float().contiguous(),
                root_vel[:, :3].float().contiguous(), table]
        if real_pick is not None:
            keep.append(real_pick.to(dev).to(torch.int32).contiguous())
            b.real_pick = keep[-1].data_ptr()
        b.real_pick_key = int(real_pick_key) & 0xFFFFFFFF
        L.check(lib.emloco_task_traj_reset(C.byref(b), keep[1].data_ptr(), n, keep[0].data_ptr(), keep[2].data_ptr(),
                                           keep[3].data_ptr(), current_stream_handle(dev)), "emloco_task_traj_reset")
        if f.init_heading and f.heading_inversion:
            self.inverted = self._inverted_u8.bool()

    def show_inverted(self):
        return self.inverted

    def get_num_verts(self):
        return self._verts.shape[1]

    def get_num_segs(self):
        return self.get_num_verts() - 1

    def get_num_envs(self):
        return self._verts.shape[0]

    def get_traj_duration(self):
        return self.get_num_verts() * self._dt      # (sic) the reference uses num_verts, not num_segs (:270-273)

    def get_traj_verts(self, traj_id):
        return self._verts[traj_id]

    def calc_pos(self, traj_ids, times):                                             # :278-296
        traj_dur = self.get_traj_duration()
        num_verts = self.get_num_verts()
        num_segs = self.get_num_segs()
        phase = torch.clip(times / traj_dur, 0.0, 1.0)
        seg_idx = phase * num_segs
        seg_id0 = torch.floor(seg_idx).long()
        seg_id1 = torch.ceil(seg_idx).long()
        lerp = (seg_idx - seg_id0).unsqueeze(-1)
        pos0 = self._verts_flat[traj_ids * num_verts + seg_id0]
        pos1 = self._verts_flat[traj_ids * num_verts + seg_id1]
        return (1.0 - lerp) * pos0 + lerp * pos1

"""float64 restatement of the crowd-aware terrain sensor (include/emloco_task.h: EmlocoCrowdBufs) -- TEST INFRASTRUCTURE ONLY.

The reference's get_heights / sample_height_points / _compute_task_obs / _compute_flip_task_obs (humanoid_pedestrain_terrain.py:400-492,
761-815,1212-1297) with the duplicate-cell rule written out as a serial loop: among the members of a group that stamp one cell the one
with the highest member * 200 + point owns it.  Inputs are float32 arrays (the state as the kernels see it); the arithmetic is float64,
so a probe within float32 rounding of a cell boundary can land in the neighbouring cell: the callers keep their probes away from them
(`margin`).
"""
import numpy as np

NB = 24


def heading(q):
    """calc_heading (torch_utils.py:137-150) of xyzw quaternions [..., 4]"""
    x, y, z, w = (q[..., k].astype(np.float64) for k in range(4))
    # my_quat_rotate(q, e_x): e_x (2 w^2 - 1) + 2 w (q x e_x) + 2 q (q . e_x)
    rx = (2.0 * w * w - 1.0) + 2.0 * x * x
    ry = 2.0 * w * z + 2.0 * y * x
    return np.arctan2(ry, rx)


def rot_z(angle, v):
    """v [..., 2 | 3] rotated about +z by angle [...]"""
    c, s = np.cos(angle), np.sin(angle)
    out = np.array(v, dtype=np.float64, copy=True)
    out[..., 0] = c * v[..., 0] - s * v[..., 1]
    out[..., 1] = s * v[..., 0] + c * v[..., 1]
    return out


def map_index(p, hscale, n):
    """world_points_to_map (:1212-1218): truncation towards zero, clipped to [0, n - 2]; the project's rule for NaN: 0"""
    # (the float32 quotient, as every implementation forms it)
    v = (np.asarray(p, np.float32) / np.float32(hscale)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, np.clip(v, -1.0, float(n)))
    return np.clip(np.trunc(v).astype(np.int64), 0, n - 2)


def world_points(origin, yaw, xs, ys):
    """[E][len(xs) * len(ys)][2]: the grid (meshgrid 'ij') rotated by yaw [E] about origin [E][>= 2]"""
    gx, gy = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64), indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel()], -1)[None].repeat(len(yaw), 0)
    return rot_z(yaw[:, None], pts) + origin[:, None, :2].astype(np.float64)


def center_mean(rb, hf, hscale, vscale):
    """the mean of the nine centre probes (:427-429,732-759): yaw-only rotation of the root, the unstamped field"""
    root = rb[:, 0]
    yaw = 2.0 * np.arctan2(root[:, 5].astype(np.float64), root[:, 6].astype(np.float64))        # quat_apply_yaw: (0, 0, z, w) normalised
    pts = world_points(root[:, :3], yaw, np.linspace(-0.1, 0.1, 3), np.linspace(-0.2, 0.2, 3))
    px, py = map_index(pts[..., 0], hscale, hf.shape[0]), map_index(pts[..., 1], hscale, hf.shape[1])
    h = np.minimum(hf[px, py], hf[px + 1, py + 1]).astype(np.float64) * vscale
    return h.mean(-1)


def _wrap16(v):
    return ((v + 32768) % 65536) - 32768


def stamp_units(vscale):
    return _wrap16(int(np.float32(1.7 / float(vscale))))


def owners(rb, hf_shape, hscale, group_size):
    """{group: {(px, py): env}}: the serial loop over members and points, the later writer wins"""
    E = rb.shape[0]
    root = rb[:, 0]
    pts = world_points(root[:, :3], heading(root[:, 3:7]), np.linspace(-0.25, 0.25, 10).astype(np.float32),
                       np.linspace(-0.5, 0.5, 20).astype(np.float32))
    px, py = map_index(pts[..., 0], hscale, hf_shape[0]), map_index(pts[..., 1], hscale, hf_shape[1])
    out = {}
    for env in range(E):                             # ascending member, ascending point: flat index order
        cells = out.setdefault(env // group_size, {})
        for p in range(200):
            cells[(int(px[env, p]), int(py[env, p]))] = env
    return out


def probe_points(rb, head_body, res, extent):
    head = rb[:, head_body]
    xy = np.linspace(-extent, extent, res).astype(np.float32)
    return world_points(head[:, :3], heading(head[:, 3:7]), xy, xy)


def clear_of_boundaries(rb, head_body, res, extent, hscale, margin=2e-5):
    """no probe, root point or centre probe of the envs of `rb` within `margin` metres of a cell boundary: float32 rounding moves a
    coordinate below 10 m by about 4e-6 m, so the float32 kernels and this float64 restatement then agree on every cell"""
    rb = np.asarray(rb, np.float32).reshape(-1, NB, 13)
    root = rb[:, 0]
    pts = [probe_points(rb, head_body, res, extent),
           world_points(root[:, :3], heading(root[:, 3:7]), np.linspace(-0.25, 0.25, 10).astype(np.float32), np.linspace(-0.5, 0.5, 20).astype(np.float32)),
           world_points(root[:, :3], 2.0 * np.arctan2(root[:, 5].astype(np.float64), root[:, 6].astype(np.float64)),
                        np.linspace(-0.1, 0.1, 3), np.linspace(-0.2, 0.2, 3))]
    c = np.concatenate([p.ravel() for p in pts]) / hscale
    return bool(np.abs(c - np.round(c)).min() * hscale > margin)


def sensor(rb, hf, hscale, vscale, head_body, res, extent, channels, stamps, group_size, env_ids=None):
    """(rows [n][res * res * channels], mirrored rows) of the listed envs (all: None), float64, clipped and scaled"""
    rb = np.asarray(rb, np.float32).reshape(-1, NB, 13)
    E = rb.shape[0]
    ids = np.arange(E) if env_ids is None else np.asarray(env_ids)
    own = owners(rb, hf.shape, hscale, group_size) if stamps else None
    units = stamp_units(vscale)
    cm = center_mean(rb, hf, hscale, vscale)
    pts = probe_points(rb, head_body, res, extent)
    px, py = map_index(pts[..., 0], hscale, hf.shape[0]), map_index(pts[..., 1], hscale, hf.shape[1])
    rows = np.zeros((len(ids), res * res, channels))
    for r, env in enumerate(ids):
        cells = own[env // group_size] if stamps else {}
        root = rb[env, 0]
        v_own = root[7:10].astype(np.float64)
        yaw = heading(root[3:7])
        for p in range(res * res):
            a, b = (int(px[env, p]), int(py[env, p])), (int(px[env, p]) + 1, int(py[env, p]) + 1)
            h1 = _wrap16(int(hf[a]) + (units if a in cells else 0))          # torch's int16 addition wraps
            h2 = _wrap16(int(hf[b]) + (units if b in cells else 0))
            rows[r, p, 0] = cm[env] - float(min(h1, h2)) * vscale
            if channels == 3:
                v_cell = rb[cells[a], 0, 7:10].astype(np.float64) if a in cells else np.zeros(3)
                rows[r, p, 1:] = rot_z(-yaw, v_cell - v_own)[:2]
    rows = np.clip(rows, -3.0, 3.0) * 5.0
    flip = rows.reshape(len(ids), res, res, channels)[:, :, ::-1].reshape(len(ids), -1)       # j reversed, no sign change (:471)
    return rows.reshape(len(ids), -1), flip


def _near(c, hscale, margin):
    q = np.asarray(c, np.float64) / hscale
    return np.abs(q - np.round(q)) * hscale <= margin


def unsure(rb, hf_shape, hscale, head_body, res, extent, stamps, group_size, margin=2e-5):
    """[E][res * res] bool, for states nobody placed: the probes whose value hangs on float32 rounding -- a probe or a centre probe
    of the env within `margin` of a cell boundary, or a diagonal cell that a root point of a member within `margin` of a boundary
    may or may not have stamped"""
    rb = np.asarray(rb, np.float32).reshape(-1, NB, 13)
    E = rb.shape[0]
    root = rb[:, 0]
    pts = probe_points(rb, head_body, res, extent)
    out = _near(pts[..., 0], hscale, margin) | _near(pts[..., 1], hscale, margin)
    cen = world_points(root[:, :3], 2.0 * np.arctan2(root[:, 5].astype(np.float64), root[:, 6].astype(np.float64)),
                       np.linspace(-0.1, 0.1, 3), np.linspace(-0.2, 0.2, 3))
    out |= _near(cen, hscale, margin).any(axis=(1, 2))[:, None]
    if stamps:
        rp = world_points(root[:, :3], heading(root[:, 3:7]), np.linspace(-0.25, 0.25, 10).astype(np.float32),
                          np.linspace(-0.5, 0.5, 20).astype(np.float32))
        doubt = {}
        for env, p in zip(*np.nonzero(_near(rp[..., 0], hscale, margin) | _near(rp[..., 1], hscale, margin))):
            for dx in (-margin, margin):
                for dy in (-margin, margin):
                    doubt.setdefault(env // group_size, set()).add((int(map_index(rp[env, p, 0] + dx, hscale, hf_shape[0])),
                                                                     int(map_index(rp[env, p, 1] + dy, hscale, hf_shape[1]))))
        px, py = map_index(pts[..., 0], hscale, hf_shape[0]), map_index(pts[..., 1], hscale, hf_shape[1])
        for env in range(E):
            cells = doubt.get(env // group_size, ())
            if cells:
                out[env] |= np.array([(a, b) in cells or (a + 1, b + 1) in cells for a, b in zip(px[env].tolist(), py[env].tolist())])
    return out

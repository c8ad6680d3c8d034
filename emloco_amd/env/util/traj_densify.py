"""Waypoint tracks to dense path vertices through a natural cubic spline.

What social-transmotion/load_jta_traj.py:66-121 (and load_jrdb_traj.py) does per track with
`scipy.interpolate.CubicSpline(traj_phase, way, axis=0, bc_type='natural')(np.arange(101))`: 13 waypoints at 0.4 s become the 101
vertices `TrajGenerator` follows; vertices 85..100 lie behind the last waypoint and are extrapolated with the last piece.

`densify` takes a batch: CUDA tensors go to the device kernel (emloco_traj_densify, csrc/traj_kernels.hip) on the current stream,
CPU tensors / arrays to a float64 host path (numpy, below) that the exporters use when no device is present.
"""
import numpy as np
import torch

# load_jta_traj.py:72 -- the phase of the 13 waypoints (2.5 fps) on the 101-vertex path of an episode
TRAJ_PHASE = np.array([0.0000, 0.0707, 0.1414, 0.2122, 0.2829, 0.3536, 0.4243, 0.4950, 0.5658, 0.6365, 0.7072, 0.7779, 0.8487]) * 100
NUM_VERTS = 101
MIN_KNOTS, MAX_KNOTS, MAX_QUERY = 4, 16, 128
DENSIFY_ORIGIN = 1          # EMLOCO_DENSIFY_ORIGIN


def _check(knot_t, query_t, way_shape):
    if not (MIN_KNOTS <= knot_t.size <= MAX_KNOTS):
        raise ValueError(f"densify: {knot_t.size} knots, the spline takes {MIN_KNOTS}..{MAX_KNOTS}")
    if not (1 <= query_t.size <= MAX_QUERY):
        raise ValueError(f"densify: {query_t.size} queries, at most {MAX_QUERY} and at least one")
    if not (np.isfinite(knot_t).all() and np.isfinite(query_t).all() and (np.diff(knot_t) > 0).all()):
        raise ValueError("densify: knots must be finite and strictly increasing, queries finite")
    if len(way_shape) != 3 or way_shape[1] != knot_t.size or way_shape[2] != 3:
        raise ValueError(f"densify: waypoints of shape {tuple(way_shape)}, expected (n_traj, {knot_t.size}, 3)")


def densify_host(way, knot_t, query_t, origin=False):
    """float64: (n, K, 3) waypoints -> ((n, Q, 3) vertices, (n,) bool valid).  The second derivatives M of the natural spline from
    the tridiagonal system  h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1] = 6 (s[i] - s[i-1])  (Thomas), then Horner on the piece
    of every query; in coordinates shifted by the first waypoint (x, y), as the kernel solves."""
    way = np.array(way, np.float64)
    t, x = np.asarray(knot_t, np.float64), np.asarray(query_t, np.float64)
    n, K = way.shape[0], t.size
    valid = np.isfinite(way).all(axis=(1, 2))
    way[~valid] = 0.0
    org = np.zeros((n, 1, 3))
    org[:, 0, :2] = way[:, 0, :2]
    y = way - org
    h = np.diff(t)
    s = (y[:, 1:] - y[:, :-1]) / h[:, None]
    M = np.zeros_like(y)
    cp, dp = np.zeros(K), np.zeros((K, n, 3))
    for i in range(1, K - 1):
        den = 2.0 * (h[i - 1] + h[i]) - h[i - 1] * cp[i - 1]
        cp[i] = h[i] / den
        dp[i] = (6.0 * (s[:, i] - s[:, i - 1]) - h[i - 1] * dp[i - 1]) / den
    for i in range(K - 2, 0, -1):
        M[:, i] = dp[i] - cp[i] * M[:, i + 1]
    b = s - h[:, None] * (2.0 * M[:, :-1] + M[:, 1:]) / 6.0
    p = np.clip(np.searchsorted(t, x, side="right") - 1, 0, K - 2)
    d = (x - t[p])[None, :, None]
    out = y[:, p] + d * (b[:, p] + d * (0.5 * M[:, p] + d * ((M[:, p + 1] - M[:, p]) / (6.0 * h[p])[:, None])))
    if not origin:
        out = out + org
    out[~valid] = 0.0
    return out, valid


def densify(way, knot_t=TRAJ_PHASE, query_t=None, origin=False):
    """(n_traj, n_knots, 3) waypoint tracks -> (dense (n_traj, n_query, 3), valid (n_traj,) bool).

    Natural cubic spline through the waypoints at `knot_t` (shared by the batch, strictly increasing, 4..16), evaluated at `query_t`
    (default arange(101); any order, inside or outside the knots, 1..128).  `origin=True` returns the vertices relative to the track's
    first waypoint (x, y) -- the form TrajGenerator wants.  A track with a non-finite waypoint has valid False and zeros.
    CUDA `way`: float32 on the device, current stream.  CPU tensor or array: float64 on the host, returned as what came in."""
    knot = np.asarray(knot_t.detach().cpu() if torch.is_tensor(knot_t) else knot_t, np.float64).reshape(-1)
    query = np.arange(NUM_VERTS, dtype=np.float64) if query_t is None else \
        np.asarray(query_t.detach().cpu() if torch.is_tensor(query_t) else query_t, np.float64).reshape(-1)
    _check(knot, query, way.shape)
    if torch.is_tensor(way) and way.is_cuda:
        from ... import _lib as L
        from ...sim import current_stream_handle
        lib = L.require_device()
        w = way.detach().float().contiguous()
        out = torch.empty((w.shape[0], query.size, 3), dtype=torch.float32, device=w.device)
        valid = torch.empty((w.shape[0],), dtype=torch.uint8, device=w.device)
        k32, q32 = np.ascontiguousarray(knot, np.float32), np.ascontiguousarray(query, np.float32)
        with torch.cuda.device(w.device):
            L.check(lib.emloco_traj_densify(k32.ctypes.data, int(k32.size), w.data_ptr(), int(w.shape[0]), q32.ctypes.data, int(q32.size),
                                            out.data_ptr(), valid.data_ptr(), DENSIFY_ORIGIN if origin else 0,
                                            current_stream_handle(w.device)), "emloco_traj_densify")
        return out, valid.bool()
    if torch.is_tensor(way):
        out, valid = densify_host(way.detach().numpy(), knot, query, origin)
        return torch.from_numpy(out), torch.from_numpy(valid)
    return densify_host(way, knot, query, origin)

"""Scenes and contact counting for the contact-matrix layout tests (tests/test_emu_sim_contact_layout.py on the CPU emulator,
tests/test_gpu_sim_contact_layout.py on the device).

The rigid-body kernel keeps the contact matrix of an env-substep in one of two LDS layouts, chosen on the number of contacts
(csrc/sim_kernels.hip: SQ_MAXC = 14): the full square up to 14 contacts, the packed lower triangle above.  The scenes here are
chosen so that single-substep steps (n_sub = 1) pass through every regime: no contact, one tile of the Gram build (1-10 contacts),
the second tile row of the square layout (11-14), both sides of the switch (exactly 14, exactly 15) and more candidates inside the
contact offset than contact slots (> 20: the shallowest are dropped).  `contact_counts` recomputes the number of candidates inside
the contact offset from the oracle's body states, so the coverage is asserted, not hoped for.
"""
import numpy as np

from helpers import bumpy_heightfield, scene_state, varied_models

NAMES = ("root_state", "dof_state", "rb_state", "contact_force", "dof_force", "lambda_ws")
E = 8
STEPS = 6
MARGIN = 1e-5          # a candidate this close to the contact offset could fall on either side in fp32: such env-substeps are not counted
MAXC = 20


def scene(ground):
    """Eight humanoids, models / root / dof / targets: two standing (feet flat: box corners), six lying on the back / side / front
    at heights from pressed into the ground to just above it.  `ground`: "plane" or "hf" (the scene is lifted by the field's
    height under each env on a height field, see `heightfield`)."""
    models = varied_models(E, seed=5)
    root, dof, tgt = scene_state(E, seed=6, height=0.93, perturbed_from=2)
    s = np.sin(np.pi / 4)
    poses = {2: ((1.0, 0.0, 0.0), LYING[0]), 3: ((0.0, 1.0, 0.0), LYING[1]), 4: ((-1.0, 0.0, 0.0), LYING[2]),
             5: ((1.0, 0.0, 0.0), LYING[3]), 6: ((0.0, 1.0, 0.0), LYING[4]), 7: ((-1.0, 0.0, 0.0), LYING[5])}
    for e, (ax, z) in poses.items():
        root[e, 3:7] = [ax[0] * s, ax[1] * s, ax[2] * s, np.cos(np.pi / 4)]
        root[e, 2] = z
        root[e, 7:13] *= 0.25
    root[0, 2], root[1, 2] = STANDING
    if ground == "hf":
        hf = heightfield()
        for e in range(E):
            root[e, 2] += _hf_height(hf, float(root[e, 0]), float(root[e, 1]))
    return models, root, dof, tgt


STANDING = (0.93, 1.05)                                    # env 0 on its feet, env 1 dropped from 12 cm
LYING = (0.06, 0.10, 0.08, 0.13, 0.16, 0.30)


def heightfield():
    """A small sloped, bumpy field over the region the scenes lie in (0.1 m grid)."""
    return bumpy_heightfield(n=640, seed=3, amp=0.03, slope=0.05)


def _hf_plane(hf, cx, cy):
    """csrc/sim_kernels.hip: hf_plane in float64: height of the cell triangle's plane under (cx, cy), its unit normal, the triangle's id."""
    smp, hs, vs = hf["samples"], hf["horizontal_scale"], hf["vertical_scale"]
    nx, ny = smp.shape
    gx, gy = (cx - hf.get("origin_x", 0.0)) / hs, (cy - hf.get("origin_y", 0.0)) / hs      # sample (0, 0) sits at the origin
    i, j = int(np.clip(np.floor(gx), 0, nx - 2)), int(np.clip(np.floor(gy), 0, ny - 2))
    u, v = gx - i, gy - j
    h00, h01, h10, h11 = (vs * float(smp[i, j]), vs * float(smp[i, j + 1]), vs * float(smp[i + 1, j]), vs * float(smp[i + 1, j + 1]))
    if u >= v:
        zx, zy = h10 - h00, h11 - h10
    else:
        zy, zx = h01 - h00, h11 - h01
    zt = h00 + u * zx + v * zy
    sx, sy = zx / hs, zy / hs
    inv = 1.0 / np.sqrt(1.0 + sx * sx + sy * sy)
    return zt, (-sx * inv, -sy * inv, inv), (i, j, u >= v)


def _hf_height(hf, cx, cy):
    return _hf_plane(hf, cx, cy)[0]


def _hf_distance(hf, p, rad):
    """Phase 5 of the kernel on a height field (no slope-corrected mesh): the sphere's centre against the plane of the triangle under
    it and, for a sphere with a radius, against the triangles under four probes one radius out."""
    zt, n, tid0 = _hf_plane(hf, p[0], p[1])
    dperp = (p[2] - zt) * n[2]
    if rad > 0.0:
        for ex, ey in ((rad, 0.0), (-rad, 0.0), (0.0, rad), (0.0, -rad)):
            ztq, nq, tidq = _hf_plane(hf, p[0] + ex, p[1] + ey)
            dq = (p[2] - ztq) * nq[2] - (ex * nq[0] + ey * nq[1])
            tidf = _hf_plane(hf, p[0] - dq * nq[0], p[1] - dq * nq[1])[2]
            if tidq != tid0 and tidf == tidq and dq < dperp:
                dperp = dq
    return dperp - rad


def _rotate(q, v):
    """v rotated by the quaternion q = (x, y, z, w)"""
    u, w = q[:3], q[3]
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def contact_counts(osim, hf=None):
    """Per env: (candidates certainly inside the contact offset, candidates possibly inside it) at the body states in
    osim.rb_state -- the state the NEXT substep detects its contacts in.  The candidate list is the kernel's: the centre of a
    sphere, the two ends of a capsule, the eight corners of a box (oracle_sim.c: find_contacts)."""
    from emloco_amd.model import GEOM_CAPSULE, GEOM_SPHERE
    a, prm = osim.arr, osim.params
    rb = osim.rb_state.astype(np.float64)
    lo, hi = np.zeros(osim.E, int), np.zeros(osim.E, int)
    for e in range(osim.E):
        for b, gt in enumerate(a["geom_type"]):
            ga, gb, rad = a["geom_a"][e, b].astype(np.float64), a["geom_b"][e, b].astype(np.float64), float(a["geom_r"][e, b])
            if gt == GEOM_SPHERE:
                pts = [ga]
            elif gt == GEOM_CAPSULE:
                pts = [ga, gb]
            else:
                pts = [ga + np.where([k & 1, k & 2, k & 4], gb, -gb) for k in range(8)]
            for lp in pts:
                p = rb[e, b, :3] + _rotate(rb[e, b, 3:7], lp)
                dist = (p[2] - prm.ground_z) - rad if hf is None else _hf_distance(hf, p, rad)
                lo[e] += dist < prm.contact_offset - MARGIN
                hi[e] += dist < prm.contact_offset + MARGIN
    return lo, hi


class Coverage:
    """Contact counts of the env-substeps a run went through (those whose count is beyond doubt)."""

    def __init__(self):
        self.counts = []

    def add(self, osim, hf=None):
        lo, hi = contact_counts(osim, hf)
        self.counts += [int(n) for n, m in zip(lo, hi) if n == m]

    def check(self):
        c = set(self.counts)
        assert 0 in c, sorted(c)
        assert c & set(range(1, 11)), sorted(c)                       # one tile of the Gram build
        assert c & set(range(11, 15)), sorted(c)                      # square layout, second tile row
        assert 14 in c and 15 in c, sorted(c)                         # last square case, first packed case
        assert any(n > MAXC for n in c), sorted(c)                    # more candidates than slots: the shallowest dropped

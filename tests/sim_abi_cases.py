"""Case tables of the rigid-body step's conformance matrix (include/emloco_sim.h): plain numpy and the oracle, shared by
tests/test_sim_abi_cpu.py (the kernels on the CPU emulator) and tests/test_gpu_sim_matrix.py (the device, through the C ABI), so the
two runs differ in the executor only.

The existing scenarios (tests/test_gpu_sim.py) all pass through n_sub = 2 x n_calls = 2, a split into 2 or 4 parts, square height
fields with their first sample at the world origin, and indexed setters that are handed the simulator's own tensor.  The tables here
hold what they leave out: every way the substeps of a step fall into parts (uneven, odd, more parts than substeps), env counts at the
edges of a wave and of the cost sort, a height field that is neither square nor at the origin, id lists with -1 padding for the row
copy of the indexed setters, and the key of the cost-ordered dispatch recomputed from float64 contact counts.
"""
import numpy as np

import contact_layout_cases as K
from helpers import oracle_sim, scene_state, varied_models

NAMES = K.NAMES                      # root_state, dof_state, rb_state, contact_force, dof_force, lambda_ws (the warm start)

# ---------------------------------------------------------------------------------------------------- split launch
# (n_sub, n_calls, n_parts): the substep window of part p is [n_sub_total * p / n_parts, n_sub_total * (p + 1) / n_parts)
SPLIT_CASES = (
    (1, 1, 1), (3, 1, 1), (5, 1, 1), (1, 3, 1),                 # unsplit, at substep totals no scenario uses
    (3, 1, 2), (3, 1, 3), (4, 1, 3),                            # 1 + 2, 1 + 1 + 1, 1 + 1 + 2
    (5, 1, 2), (5, 1, 3), (5, 1, 4),                            # 2 + 3, 1 + 2 + 2, 1 + 1 + 1 + 2
    (2, 3, 4), (1, 2, 2), (7, 1, 4),                            # 1 + 2 + 1 + 2, 1 + 1, 1 + 2 + 2 + 2
    (1, 1, 4), (2, 1, 3),                                       # more parts than substeps: clamped to 1 and to 2 parts
)
SPLIT_SUBSET_CASES = ((3, 1, 2), (5, 1, 3))                     # uneven cases the device also issues as skip flags + id list
SPLIT_STEPS = 3
SPLIT_ENVS_EMU, SPLIT_ENVS_DEVICE = 3, 5
ENV_COUNTS = (1, 2, 63, 64, 65)                                 # one env, and both sides of a 64-lane wave


def split_scene(E):
    """models / root / dof / targets of the split and env-count cases: env 0 stands, the others start perturbed"""
    return (varied_models(E, 31),) + scene_state(E, 32)


def split_oracle(E, n_sub, n_calls):
    """The oracle runs the n_sub * n_calls substeps of a control step as one call (the device fuses them into one launch)."""
    models, root, dof, tgt = split_scene(E)
    return oracle_sim(models, root, dof, tgt, self_collision=True, n_sub=n_sub * n_calls)


# ---------------------------------------------------------------------------------------------------- height field
HF_NX, HF_NY = 90, 41
HF_ORIGIN = (float(np.float32(48.3)), float(np.float32(52.7)))  # as the C ABI's float parameters hold them
HF_HS, HF_VS = 0.1, 0.005
HF_KINDS = ("slope_x", "slope_y", "slope_x_risers")
HF_STEPS = 12
HF_XY = ((50.0, 55.0), (50.7, 53.0), (48.0, 55.2), (57.5, 56.9))   # two inside, one before the first row, one behind the last row (and column)
HF_DROP = 0.95


def offset_field(kind):
    """A height field that is not square (90 x 41 samples) and does not start at the world origin (sample (0, 0) at (48.3, 52.7)): a
    gradient of 0.3 along x or y about (50, 55).  `..._risers`: plus a plateau and a trench bounded by one-cell 15 cm risers, with the
    vertex moves of the slope-corrected mesh (terrain_utils.convert_heightfield_to_trimesh, threshold 0.9) -- risers looking along x
    and along y, so the mesh path is taken.  A swapped nx / ny or a dropped origin moves every humanoid of `hf_scene` off its ground."""
    risers = kind.endswith("_risers")
    base = kind[:-len("_risers")] if risers else kind
    x = HF_ORIGIN[0] + np.arange(HF_NX)[:, None] * HF_HS
    y = HF_ORIGIN[1] + np.arange(HF_NY)[None, :] * HF_HS
    z = {"slope_x": 0.3 * (x - 50.0) + 0.0 * y, "slope_y": 0.3 * (y - 55.0) + 0.0 * x}[base]
    samples = np.rint(z / HF_VS).astype(np.int16)
    hf = dict(samples=samples, horizontal_scale=HF_HS, vertical_scale=HF_VS, origin_x=HF_ORIGIN[0], origin_y=HF_ORIGIN[1])
    if risers:
        samples[19:27, :] += 30                                 # plateau: risers across x at x = 50.2 and 51.0
        samples[:, 25:30] -= 30                                 # trench: risers across y at y = 55.2 and 55.7
        from emloco_amd.gym import terrain_utils as T
        verts, _ = T.convert_heightfield_to_trimesh(samples, HF_HS, HF_VS, 0.9)
        mx, my = T.mesh_vertex_moves(verts, samples.shape, HF_HS)
        assert (mx != 0).any() and (my != 0).any()
        hf.update(move_x=mx, move_y=my)
    assert samples.shape == (HF_NX, HF_NY)
    return hf


def hf_scene(hf):
    """Four humanoids on `offset_field`: two inside the field, one before its first row, one behind its last row, each HF_DROP above
    the nearest sample."""
    E = len(HF_XY)
    models = varied_models(E, 31)
    root, dof, tgt = scene_state(E, 32, perturbed_from=0)
    smp = hf["samples"]
    for e, (px, py) in enumerate(HF_XY):
        i = int(np.clip(np.rint((px - hf["origin_x"]) / HF_HS), 0, HF_NX - 1))
        j = int(np.clip(np.rint((py - hf["origin_y"]) / HF_HS), 0, HF_NY - 1))
        root[e, 0], root[e, 1], root[e, 2] = px, py, HF_DROP + HF_VS * float(smp[i, j])
    return models, root, dof, tgt


def hf_oracle(kind, n_sub):
    hf = offset_field(kind)
    models, root, dof, tgt = hf_scene(hf)
    return oracle_sim(models, root, dof, tgt, self_collision=True, heightfield=hf, n_sub=n_sub), hf


# ---------------------------------------------------------------------------------------------------- indexed setters
COPY_ENVS = 6


def id_lists(n_env=COPY_ENVS):
    """(name, int32 list, n_env it needs): id lists of the indexed setters -- valid ids first, -1 padding after them."""
    long = np.full(300, -1, np.int32)                           # beyond the 256 workgroups of the forward-kinematics launch
    long[:40] = np.random.default_rng(7).permutation(300)[:40]
    return (("two", np.array([3, 1], np.int32), n_env), ("first", np.array([0], np.int32), n_env),
            ("last", np.array([n_env - 1], np.int32), n_env), ("padded", np.array([2, -1, -1], np.int32), n_env),
            ("only_padding", np.array([-1], np.int32), n_env), ("300_entries", long, 300))


# ---------------------------------------------------------------------------------------------------- cost key
KEY_STEPS = 6
KEY_SCENES = ("plane", "hf", "slope_x", "slope_y")
KEY_MAX_DOUBTFUL = 0.10


def cost_key(counts):
    """The key of the cost-ordered dispatch (csrc/sim_kernels.hip: `work`) of one env's step from the number of contact candidates
    inside the contact offset at each of its substeps: 10 + the contacts kept (at most EMLOCO_MAXC = 20) where there are any."""
    return int(sum(10 + min(int(n), K.MAXC) if n else 0 for n in counts))


def key_oracle(scene):
    """(oracle at n_sub = 1, height field or None) of a cost-key scene"""
    if scene in ("plane", "hf"):
        models, root, dof, tgt = K.scene(scene)
        hf = K.heightfield() if scene == "hf" else None
        return oracle_sim(models, root, dof, tgt, self_collision=True, heightfield=hf, n_sub=1), hf
    return hf_oracle(scene, 1)


class KeyCheck:
    """Collects, per env-step, the float64 contact count at the state the step starts from and the key the step reported."""

    def __init__(self):
        self.compared, self.doubtful, self.cov = 0, 0, K.Coverage()

    def before_step(self, osim, hf):
        self.lo, self.hi = K.contact_counts(osim, hf)
        self.cov.counts += [int(n) for n, m in zip(self.lo, self.hi) if n == m]

    def after_step(self, keys, what):
        for e, (n, m) in enumerate(zip(self.lo, self.hi)):
            if n != m:
                self.doubtful += 1
                continue
            self.compared += 1
            assert int(keys[e]) == cost_key([n]), f"{what} env {e}: key {int(keys[e])}, {n} contacts give {cost_key([n])}"

    def share_doubtful(self):
        return self.doubtful / float(self.doubtful + self.compared)

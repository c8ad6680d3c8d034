#!/usr/bin/env python3
"""Golden vectors of TrajGenerator.reset under --pred_path, from the REFERENCE's own code (traj_generator.py:53-54,163-175).

    python tests/golden/gen_golden_pred_path.py          # writes tests/golden/traj_reset_pred.npz

In the manner of gen_golden.py: the reference is imported read-only through _ref_shim.py; only the inputs, the rows it sampled and
the vertices it produced are stored.  Its constructor loads data/traj/traj_pred_data.pkl from a hard-coded relative path, so the
generator is built with the flag off and handed the table the way the constructor stores it (:54).  `random.sample(dict.keys(), n)`
(:165) is handed a list of the keys where this Python refuses a key view: the same sample.

Two cases of 16 envs on a table of 24 rows (world coordinates, +-100 m): `plain` (no flag) and `heading` (init_heading +
heading_inversion + adjust_root_vel: the pred branch does not rescale speeds, :174).  Keys are stored with a case prefix.
"""
import os
import random as pyrandom
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim  # noqa: E402

E, ROWS, NV = 16, 24, 101


def pred_table(seed):
    """{key: {'coord_dense': (101, 3) float64, ...}} as evaluate_jta --save_pred_trajs writes it: key = sample * 20 + mode."""
    r = np.random.RandomState(seed)
    out = {}
    for i in range(ROWS):
        speed, turn = r.uniform(0.05, 2.5), r.uniform(-0.4, 0.4)
        tt = np.arange(NV) * 0.056
        th = r.uniform(-np.pi, np.pi) + turn * tt
        xy = np.cumsum(np.stack([np.cos(th), np.sin(th)], -1) * speed * 0.056, 0) + r.uniform(-100, 100, 2)
        z = np.full((NV, 1), r.uniform(0.8, 1.0))
        key = (i // 3) * 20 + (i % 3) * 7
        out[key] = {"coord_dense": np.concatenate([xy, z], -1), "sample": i // 3, "mode": (i % 3) * 7}
    return out          # (no standing start: the reference's alignment check, :221-226, cannot index a zero first segment under heading_inversion)


def main():
    _ref_shim.install_pacer()
    import env.util.traj_generator as TG
    from utils.flags import flags
    TG.random = SimpleNamespace(sample=lambda population, k: pyrandom.sample(list(population), k))
    g = torch.Generator().manual_seed(2024)
    init_pos = torch.stack([torch.rand(E, generator=g) * 40 + 30, torch.rand(E, generator=g) * 40 + 30, torch.rand(E, generator=g) * 0.4 + 0.7], -1)
    root_vel = torch.randn(E, 3, generator=g)
    root_vel[3] = 0.0                                       # a standing root: the heading block's zero-vector branch
    table = pred_table(11)
    keys = list(table.keys())
    out = dict(init_pos=init_pos.numpy(), root_vel=root_vel.numpy(), pred_keys=np.array(keys, np.int64),
               pred_table=np.stack([v["coord_dense"] for v in table.values()]).astype(np.float64))
    env_ids = torch.arange(E, dtype=torch.long)
    for tag, heading in (("plain", False), ("heading", True)):
        for k, val in dict(real_path=False, jta_path=False, jrdb_path=False, pred_path=False, fixed_path=False, slow=False,
                           adjust_root_vel=heading, init_heading=heading, heading_inversion=heading, add_noise=False, vru=False).items():
            setattr(flags, k, val)
        tg = TG.TrajGenerator(E, 168 * (2 / 60.0), NV, "cpu", 2.0, 0.0005, 3.0, 2.0, 0.02, None, hybridInitProb=0.5, flags=flags)
        flags.pred_path = True
        tg.traj_pred_data = table
        tg.inverted[:] = True
        torch.manual_seed(130 + heading)
        pyrandom.seed(140 + heading)
        st, pst = torch.get_rng_state(), pyrandom.getstate()
        tg.reset(env_ids, init_pos.clone(), root_vel.clone())
        # replay of the draws in the reference's call order (:64-77, :165, :196)
        torch.set_rng_state(st)
        pyrandom.setstate(pst)
        r1 = torch.rand([E, NV - 1]); r2 = torch.rand([E, NV - 1])
        bern = torch.bernoulli(0.02 * torch.ones(E, NV - 1))
        r3 = torch.rand([E]); r4 = torch.rand([E, NV - 1]); r5 = torch.rand([E])
        rids = pyrandom.sample(keys, E)
        r6 = torch.rand(E)
        case = dict(r_dtheta=r1, r_dtheta_sharp=r2, bern_sharp=bern, r_heading=r3, r_dspeed=r4, r_speed0=r5, r_inversion=r6,
                    pred_rids=np.array([keys.index(k) for k in rids], np.int64), verts=tg._verts.clone(),
                    inverted=tg.inverted.clone().long())
        for k, v in case.items():
            out[f"{tag}_{k}"] = v.numpy() if isinstance(v, torch.Tensor) else v
        flags.pred_path = False
    out["dt_vert"] = np.array(168 * (2 / 60.0) / (NV - 1), np.float64)
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(HERE, "traj_reset_pred.npz"), **out)
    print("wrote traj_reset_pred", {k: tuple(np.shape(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()

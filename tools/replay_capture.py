"""Replay the captures of a flight-recorder file (`run.py --capture`, learning/flight_recorder.py) through the CPU oracle, step by step
and bit for bit -- where gdb can reach the step that a training run blew up in.

    python tools/replay_capture.py FILE [--capture K] [--dump DIR]

For capture K (default: every capture of the file) an `oracle.Sim` of the ONE captured env is built from the model rows, engine
parameters and ground the file stores, with the file's substeps per control step as its `n_sub` (the device runs a control step as
one fused launch).  For each valid record i the oracle takes root state, dof state, warm start and drive input from
the record and steps one control step.  Where record i + 1 continues the episode (its progress is record i's + 1) the oracle's root, dof
and warm start are compared with it word for word; a record behind a reset is a fresh start and is not compared.  The step from the last
record is compared against all six arrays of the state after the step.  Per step: whether it matched, the fastest body and its speed,
the contacts that carry an impulse, the first differing word.  Exit status 1 when any compared step differs -- which is a finding of its
own: the record then leaves out something the step reads.

`--dump DIR` writes `capture<K>_rb.npy`, the oracle's body states [steps][24][13] after every replayed step, for plotting.

Uses the CPU oracle (oracle/), like the tests; no device and no device library."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEXT_ARRAYS = ("root", "dof", "warm")
POST_ARRAYS = ("root", "dof", "warm", "rb", "contact_force", "dof_force")


def build_sim(d, k):
    """oracle.Sim of the env of capture k, from what the file stores"""
    import oracle
    from emloco_amd.learning.flight_recorder import PARAM_FIELDS, SHARED_MODEL_KEYS, SHARED_SC_KEYS
    ints = ("n_sub", "n_iter", "drive_mode")
    params = oracle.default_params(**{f: (int(d["params/" + f]) if f in ints else float(d["params/" + f])) for f in PARAM_FIELDS})
    params.n_sub = int(d["substeps"])         # a control step is ONE fused launch of n_sub x controlFrequencyInv substeps: one oracle call
    packed = {key[6:]: (v if key[6:] in SHARED_MODEL_KEYS else v[k:k + 1]) for key, v in d.items() if key.startswith("model/")}
    sc = None
    if int(d["sc_on"]):
        sc = {}
        for key, v in d.items():
            if key.startswith("sc/"):
                name = key[3:]
                sc[name] = (float(v) if v.ndim == 0 else v) if name in SHARED_SC_KEYS else v[k:k + 1]
    hf = None
    if "ground/samples" in d:
        hf = dict(samples=d["ground/samples"], **{f: float(d["ground/" + f]) for f in ("horizontal_scale", "vertical_scale", "origin_x", "origin_y")})
        if "ground/move_x" in d:
            hf.update(move_x=d["ground/move_x"], move_y=d["ground/move_y"])
    else:
        params.ground_z = float(d["ground/plane_z"])
    return oracle.Sim(packed, params, self_collision=sc, heightfield=hf)


def _first_diff(sim_arrays, want, names):
    for name in names:
        got, ref = np.ascontiguousarray(sim_arrays[name]).view(np.uint32).ravel(), np.ascontiguousarray(want[name]).view(np.uint32).ravel()
        bad = np.nonzero(got != ref)[0]
        if bad.size:
            i = int(bad[0])
            return dict(array=name, index=i, got=int(got[i]), want=int(ref[i]), n_diff=int(bad.size))
    return None


def replay(file_or_dict, k, dump_dir=None):
    """-> report: dict(capture, env, t, cause, causes, n_valid, matched, compared, steps=[dict(t, progress, against, matched,
    first_diff, fastest_body, speed, contacts)]).  `against` is "next" (the following record), "post" (the state after the step) or
    None (a reset lies between: not compared)."""
    from emloco_amd.learning import flight_recorder as FR
    d = FR.load(file_or_dict) if isinstance(file_or_dict, (str, os.PathLike)) else file_or_dict
    depth = int(d["depth"])
    slot = FR.parse_slot(d["captures"][k], depth)
    sim = build_sim(d, k)
    recs, steps, bodies = slot["records"], [], []
    for i, rec in enumerate(recs):
        sim.root_state[0], sim.dof_state[0], sim.lambda_ws[0], sim.pd_target[0] = rec["root"], rec["dof"], rec["warm"], rec["drive"]
        sim.params.drive_mode = rec["drive_mode"]
        sim.step(1)
        now = dict(root=sim.root_state[0], dof=sim.dof_state[0], warm=sim.lambda_ws[0], rb=sim.rb_state[0],
                   contact_force=sim.contact_force[0], dof_force=sim.dof_force[0])
        if i + 1 < len(recs):
            cont = recs[i + 1]["progress"] == rec["progress"] + 1
            against, diff = ("next", _first_diff(now, recs[i + 1], NEXT_ARRAYS)) if cont else (None, None)
        else:
            against, diff = "post", _first_diff(now, slot["post"], POST_ARRAYS)
        rb = sim.rb_state[0].astype(np.float64)
        with np.errstate(all="ignore"):
            speed = np.sqrt((rb[:, 7:10] ** 2).sum(axis=1))
        fastest = int(np.nanargmax(speed)) if np.isfinite(speed).any() else -1
        steps.append(dict(t=rec["t"], progress=rec["progress"], against=against, matched=None if against is None else diff is None,
                          first_diff=diff, fastest_body=fastest, speed=float(speed[fastest]) if fastest >= 0 else float("nan"),
                          contacts=int((sim.lambda_ws[0].reshape(-1, 3) != 0).any(axis=1).sum())))
        bodies.append(sim.rb_state[0].copy())
    if dump_dir is not None:
        os.makedirs(dump_dir, exist_ok=True)
        np.save(os.path.join(dump_dir, f"capture{k}_rb.npy"), np.stack(bodies) if bodies else np.zeros((0, 24, 13), np.float32))
    compared = [s for s in steps if s["against"] is not None]
    return dict(capture=int(k), env=slot["env"], t=slot["t"], cause=slot["cause"], causes=FR.cause_names(slot["cause"]),
                n_valid=slot["n_valid"], steps=steps, compared=len(compared), matched=all(s["matched"] for s in compared))


def describe(report):
    lines = [f"capture {report['capture']}: env {report['env']} at step {report['t']}, cause {'+'.join(report['causes']) or '-'}, "
             f"{report['n_valid']} records"]
    for s in report["steps"]:
        what = "not compared (reset)" if s["against"] is None else ("matched" if s["matched"] else "MISMATCH") + f" ({s['against']})"
        line = f"  t {s['t']:>7d}  progress {s['progress']:>4d}  {what:<22s} fastest body {s['fastest_body']:>2d} {s['speed']:9.3f} m/s  contacts {s['contacts']:>2d}"
        if s["first_diff"]:
            f = s["first_diff"]
            line += f"  first difference: {f['array']}[{f['index']}] 0x{f['got']:08x} != 0x{f['want']:08x} ({f['n_diff']} words)"
        lines.append(line)
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--capture", type=int, default=None, help="index of the capture to replay (default: all)")
    ap.add_argument("--dump", default=None, metavar="DIR", help="write per-step body states here")
    a = ap.parse_args(argv)
    from emloco_amd.learning import flight_recorder as FR
    d = FR.load(a.file)
    n = int(d["captures"].shape[0])
    if a.capture is not None and not 0 <= a.capture < n:
        ap.error(f"--capture {a.capture}: the file holds {n} captures")
    ok = True
    for k in ([a.capture] if a.capture is not None else range(n)):
        report = replay(d, k, a.dump)
        print(describe(report))
        ok = ok and report["matched"]
    missed = {c: int(v) for c, v in zip(FR.CAUSES, d["overflow"]) if int(v)}
    print(f"{n} captures, {'every compared step matched' if ok else 'MISMATCH'}" + (f"; no slot left for {missed}" if missed else ""))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

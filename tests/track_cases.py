"""TEST INFRASTRUCTURE ONLY: scripted streams for the path tracking of the LocoVal evaluation (emloco_locoval_eval_track, `run.py --test
--eval_tracks`) and a float64 numpy restatement of the tracker, shared by tests/test_locoval_eval_track_cpu.py (the kernels on the CPU
emulator) and tests/test_gpu_locoval_eval_track.py (the library on the device).

What is restated, and in what precision.  The inputs (vertices, root positions, dt, traj_dur) are fp32 values, exact in float64.  The
target is calc_pos (traj_generator.py:278-296; pinned to the reference by the task tests' goldens): the segment (i0, i1) and the weight
`lerp` are DEFINED by its fp32 time / phase arithmetic -- (float)progress * dt, / traj_dur, clipped to [0, 1], * 100, floor / ceil -- and
are taken here in fp32 exactly as defined (numpy float32 scalars: one correctly rounded operation each, no contraction).  Everything after
that is float64: the interpolation (1 - lerp) v0 + lerp v1, the deviation, the sums, the means, the walked length, the samples.

The bound of the float fields (issue: not a free number).  With C the largest coordinate magnitude of the case, the device's fp32 target
differs from the float64 one by at most 2.5 * 2^-24 C per axis (the rounding of 1 - lerp, of the two products and of their sum); a
deviation then costs two subtractions, two products, one sum and one square root in fp32, each relative 2^-24 of a quantity no larger
than the deviation (squared): |dev32 - dev64| <= sqrt(2) 2.5 * 2^-24 C + 3 * 2^-24 dev < 8 * 2^-24 C + 8 * 2^-24 dev.  Means and maxima
of deviations inherit it (the sums are doubles; the one cast to fp32 is inside the relative part), the walked length is a double sum of
fp32 step lengths of exact inputs (relative only).  So every float field of a record is held to
    |got - want| <= 8 * 2^-24 * C + 8 * 2^-24 * |want|.

The stored samples.  The issue holds them to "1 ulp of the coordinate": here ulp(C) = np.spacing(float32(C)), the spacing of fp32 at the
case's largest coordinate (between 2^-24 C and 2^-23 C), for all four components against the float64 restatement.  What derives it, half
by half: the WALKED half is one fp32 subtraction of two exact inputs, wrong by at most half an ulp of its result, and the result (a
position relative to the path's first vertex) is far smaller than C -- inside the bound with room.  The TARGET half subtracts the first
vertex from the device's fp32 target, which already carries the interpolation's 2.5 * 2^-24 C (1.25 to 2.5 ulp(C)) at worst: against
float64 the issue's 1 ulp is therefore NOT guaranteed by derivation for this half; the test holds it all the same, as the issue sets it
(measured: 0.91 ulp(C) in the cap case).  What IS derived for the target half is checked beside it: against calc_pos restated operation
by operation in fp32 (`target32`), the stored value is one fp32 subtraction, so at most half an ulp of its own value away.
"""
import numpy as np

TRACK_SAMPLES = 16
F32 = np.float32
RECORD_FLOATS = ("ade", "fde", "mean_dev", "max_dev", "final_dev", "path_len")
ROOT_STRIDE = 5                       # floats between the root positions of consecutive envs in the scripted root tensor (x, y, z, junk, junk)


def _path(rng, origin, step, turn):
    """101 fp32 vertices from `origin`: steps of `step` metres whose heading drifts by `turn` rad per vertex (+ noise)."""
    heading = rng.uniform(-np.pi, np.pi) + np.cumsum(turn + 0.02 * rng.standard_normal(100))
    xy = np.concatenate([[origin], origin + np.cumsum(step * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)])
    return np.concatenate([xy, rng.uniform(0.0, 1.0, (101, 1))], axis=1).astype(F32)


def calc_pos32(verts, progress, dt, traj_dur):
    """(i0, i1, lerp) of calc_pos in its own fp32 arithmetic (csrc/task_device.h: calc_pos)."""
    time = F32(progress) * F32(dt)
    phase = F32(time / F32(traj_dur))
    phase = min(max(phase, F32(0.0)), F32(1.0))
    seg = F32(phase * F32(verts.shape[0] - 1))
    i0, i1 = int(np.floor(seg)), int(np.ceil(seg))
    return i0, i1, F32(seg - F32(i0))


def target64(verts, progress, dt, traj_dur):
    i0, i1, lerp = calc_pos32(verts, progress, dt, traj_dur)
    lerp = np.float64(lerp)
    return (1.0 - lerp) * verts[i0].astype(np.float64) + lerp * verts[i1].astype(np.float64)


def target32(verts, progress, dt, traj_dur):
    """calc_pos operation by operation in fp32, as the device computes it without contraction."""
    i0, i1, lerp = calc_pos32(verts, progress, dt, traj_dur)
    return F32(F32(F32(1.0) - lerp) * verts[i0]) + F32(lerp * verts[i1])


def make_case(lengths, games_per_env, stride, traj_dur, origins, filler=25, drift=(), seed=0, total=None):
    """Scripted streams of E = len(lengths) envs: env e plays games of lengths[e] steps one after another, then games of `filler` steps
    until the last step T (`total`, or the longest env's scripted games).  Every game walks a path of its own (the reset rewrites the
    env's vertices) starting near origins[e]; the root follows the target with a wobble of a few decimetres, and in the (env, game)
    pairs of `drift` runs away from it by metres.  Returns per step t: verts [T, E, 101, 3], root [T, E, ROOT_STRIDE], progress [T, E]
    (the step of the game, from 1: after the increment), dones [T, E]; `game` [T, E] is the game's index in the env."""
    rng = np.random.default_rng(seed)
    E = len(lengths)
    dt = F32(1.0 / 30.0)
    T = int(total if total is not None else max(sum(L) for L in lengths))
    verts = np.zeros((T, E, 101, 3), F32)
    root = rng.uniform(-64.0, 64.0, (T, E, ROOT_STRIDE)).astype(F32)
    progress = np.zeros((T, E), np.int64)
    dones = np.zeros((T, E), np.int64)
    game = np.zeros((T, E), np.int64)
    for e in range(E):
        t, g, todo = 0, 0, list(lengths[e])
        while t < T:
            n = todo.pop(0) if todo else filler
            v = _path(rng, np.asarray(origins[e], np.float64) + rng.uniform(-1.0, 1.0, 2), rng.uniform(0.04, 0.09), rng.uniform(-0.03, 0.03))
            phase = rng.uniform(0.0, 6.0)
            for k in range(1, n + 1):
                if t >= T:
                    break
                tar = target64(v, k, dt, traj_dur)[:2]
                off = np.array([0.3 * np.sin(0.11 * k + phase), 0.2 * np.cos(0.07 * k + phase)])
                if (e, g) in drift:
                    off = off + 0.05 * k * np.array([np.cos(phase), np.sin(phase)])
                verts[t, e], progress[t, e], game[t, e] = v, k, g
                root[t, e, :2] = (tar + off).astype(F32)
                dones[t, e] = 1 if k == n else 0
                t += 1
            g += 1
    assert np.abs(verts[..., :2]).max() <= 64.0 and np.abs(root).max() <= 64.0
    return dict(E=E, G=int(games_per_env), T=T, stride=int(stride), dt=dt, traj_dur=F32(traj_dur), verts=verts, root=root,
                progress=progress, dones=dones, game=game, lengths=[list(L) for L in lengths])


def main_case():
    """The issue's cases: 5 envs (no multiple of 4 or 256), 2 games each, stride 12, dt 1/30; a game that ends at its first step, one
    that ends on a sample step (12), one a step after it (13), a full one of 168 steps (14 samples), env 3 playing a third (and fourth)
    game after its quota is met, boundaries shifted between the envs; env 2's second game is still running at the end (its record slot
    stays empty, its first sample is already stored).  traj_dur 5.0 s: the steps past 150 clip at the last vertex.  Env 4's second
    game drifts beyond fail_dist."""
    lengths = [[1, 12], [13, 168], [168, 30], [12, 13, 20, 31], [5, 90]]
    origins = [(50.0, -45.0), (-48.0, 40.0), (3.0, 2.0), (-20.0, -50.0), (30.0, 0.5)]
    return make_case(lengths, 2, 12, 5.0, origins, drift={(4, 1)}, seed=7, total=181)


def cap_case():
    """Stride 1 and games longer than EMLOCO_TRACK_SAMPLES steps: the samples past the cap are dropped and not counted."""
    return make_case([[20], [16], [17]], 1, 1, 0.5, [(10.0, 10.0), (-40.0, 5.0), (0.0, -50.0)], seed=11)


def coord_max(case):
    """The largest coordinate magnitude the tracker reads (xy of the vertices and of the root)."""
    return float(max(np.abs(case["verts"][..., :2]).max(), np.abs(case["root"][..., :2]).max()))


def restate(case):
    """The tracker in float64: records {field: [E, G]}, samples [E, G, 16, 4], `games` [E], dev_now [T, E], and `touched` [E, G, 16]
    (the sample slots written)."""
    E, G, T, stride = case["E"], case["G"], case["T"], case["stride"]
    rec = {k: np.zeros((E, G), np.float64) for k in RECORD_FLOATS}
    rec["n_samples"] = np.zeros((E, G), np.int64)
    samples = np.zeros((E, G, TRACK_SAMPLES, 4), np.float64)
    touched = np.zeros((E, G, TRACK_SAMPLES), bool)
    target_f32 = np.zeros((E, G, TRACK_SAMPLES, 2), np.float64)          # float64(fp32 target) - first vertex
    games = np.zeros(E, np.int64)
    dev_now = np.zeros((T, E), np.float64)
    for e in range(E):
        devs, smp, walked, prev = [], [], 0.0, None
        for t in range(T):
            v = case["verts"][t, e]
            tar = target64(v, case["progress"][t, e], case["dt"], case["traj_dur"])[:2]
            xy = case["root"][t, e, :2].astype(np.float64)
            dev = float(np.sqrt(((tar - xy) ** 2).sum()))
            dev_now[t, e] = dev
            g = int(games[e])
            if g >= G:
                continue
            devs.append(dev)
            if prev is not None:
                walked += float(np.sqrt(((xy - prev) ** 2).sum()))
            prev = xy
            if case["progress"][t, e] % stride == 0 and len(smp) < TRACK_SAMPLES:
                v0 = v[0, :2].astype(np.float64)
                samples[e, g, len(smp)] = np.concatenate([xy - v0, tar - v0])
                target_f32[e, g, len(smp)] = target32(v, case["progress"][t, e], case["dt"], case["traj_dur"])[:2].astype(np.float64) - v0
                touched[e, g, len(smp)] = True
                smp.append(dev)
            if case["dones"][t, e]:
                rec["ade"][e, g] = np.mean(smp) if smp else 0.0
                rec["fde"][e, g] = smp[-1] if smp else 0.0
                rec["mean_dev"][e, g], rec["max_dev"][e, g], rec["final_dev"][e, g] = np.mean(devs), np.max(devs), devs[-1]
                rec["path_len"][e, g], rec["n_samples"][e, g] = walked, len(smp)
                games[e] = g + 1
                devs, smp, walked, prev = [], [], 0.0, None
    return dict(rec=rec, samples=samples, touched=touched, games=games, dev_now=dev_now, target_f32=target_f32)


def check(case, want, raw_records, samples, games, dev_now=None):
    """Holds a run's outputs (raw_records: [E, G] of TRACK_DTYPE, samples [E, G, 16, 4] fp32, games [E]) to the restatement: integers
    and the written slots exactly, floats to the bounds of the module docstring.  Returns the measured maxima as fractions of the bounds (the samples in ulp(C))."""
    E, G = case["E"], case["G"]
    C_ = coord_max(case)
    eps = 2.0 ** -24
    assert np.array_equal(np.asarray(games, np.int64), want["games"])
    done = np.arange(G)[None, :] < want["games"][:, None]
    assert np.array_equal(raw_records["n_samples"].astype(np.int64)[done], want["rec"]["n_samples"][done])
    # a slot no game was recorded in holds zero bytes, and so does every sample slot no sample went to
    assert not any(raw_records[k][~done].any() for k in raw_records.dtype.names)
    assert not samples[~want["touched"]].view(np.uint8).any()
    worst = {}
    for k in RECORD_FLOATS:
        got, ref = raw_records[k].astype(np.float64)[done], want["rec"][k][done]
        bound = 8 * eps * C_ + 8 * eps * np.abs(ref)
        err = np.abs(got - ref)
        worst[k] = float((err / bound).max())
        print(f"track check: {k}: max |err| {err.max():.3e}, {worst[k]:.3f} of its bound")
        assert (err <= bound).all(), (k, float(err.max()))
    ulp = float(np.spacing(F32(C_)))
    err = np.abs(samples.astype(np.float64) - want["samples"])[want["touched"]]
    worst["samples"] = float(err.max() / ulp)
    print(f"track check: samples: max |err| {err.max():.3e} (walked half {err[:, :2].max():.3e}, target half {err[:, 2:].max():.3e}), "
          f"{worst['samples']:.3f} ulp of {C_:.1f}")
    assert (err <= ulp).all(), float(err.max())
    # the target half as derived: one fp32 subtraction from the fp32 target, half an ulp of the stored value
    got, ref = samples[..., 2:][want["touched"]], want["target_f32"][want["touched"]]
    err = np.abs(got.astype(np.float64) - ref)
    half = 0.5 * np.spacing(np.abs(got).astype(F32)).astype(np.float64)
    worst["target_f32"] = float((err / half).max())
    print(f"track check: target half against the fp32 target: max |err| {err.max():.3e}, {worst['target_f32']:.3f} of half an ulp of the value")
    assert (err <= half).all(), float(err.max())
    if dev_now is not None:
        ref = want["dev_now"]
        err = np.abs(np.asarray(dev_now, np.float64) - ref)
        worst["dev_now"] = float((err / (8 * eps * C_ + 8 * eps * ref)).max())
        print(f"track check: dev_now: max |err| {err.max():.3e}, {worst['dev_now']:.3f} of its bound")
        assert (err <= 8 * eps * C_ + 8 * eps * ref).all()
    # the one-step game: no sample, nothing walked
    one = done & (want["rec"]["n_samples"] == 0)
    assert (raw_records["ade"][one] == 0).all() and (raw_records["fde"][one] == 0).all()
    return worst

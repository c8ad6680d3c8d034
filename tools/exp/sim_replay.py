"""Replay of one rigid-body launch on the host: what would another part plan (emloco_sim_set_plan) make of the same jobs?

    python tools/exp/sim_sched.py --dump trace.npz          # on the GPU box, schedule-trace build, the uniform 4-part launch
    python tools/exp/sim_replay.py trace.npz                # anywhere

A list scheduler with the device's rules as far as the trace shows them: `slots` wave slots (256 CUs x 12); workgroups are
dispatched strictly in index order, each onto the slot that frees first, no faster than the trace's fill rate; a consumer holds
its slot while it waits for its producer's hand-over; it then runs for its job time.  Job times are the trace's, per (env, part):
a part of two substeps costs the sum of its substeps less one prologue (the hand-over it does not take), a tail part costs the
last part's time less the env's median other part -- the final kinematics pass and the write-back -- behind a prologue of its
own, and the last substep's part loses that much.  The model knows nothing of what a job's speed owes to its neighbours on the CU (a wave
runs faster on an emptier SIMD), so the replay of the traced order itself is printed first: candidates rank only beyond its error.
"""
import argparse
import heapq

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--slots", type=int, default=0, help="wave slots (default: the trace's)")
ap.add_argument("--k", default="256,512,1024,1536,2048,3072", help="sizes of the light class (last ranks) to sweep")
a = ap.parse_args()
z = np.load(a.trace)
slots = a.slots or int(z["slots"])
env, part, n_parts = z["env"], z["part"], z["n_parts"]
assert (n_parts == 4).all(), "replay starts from a trace of the uniform 4-part launch"
first, handed, last, rank = z["first"], z["handed"], z["last"], z["rank"]
envs = np.unique(env)
n = len(envs)
pos = {e: i for i, e in enumerate(envs)}
R = np.zeros((n, 4))                                # run time of (env, part)
A0 = np.zeros((n, 4)); H0 = np.zeros((n, 4)); B0 = np.zeros((n, 4))
rk = np.zeros(n, np.int64)
for e, p, f, h, l, r in zip(env, part, first, handed, last, rank):
    i = pos[e]
    R[i, p] = l - h; A0[i, p] = f; H0[i, p] = h; B0[i, p] = l
    rk[i] = r
order = np.argsort(rk, kind="stable")               # traced envs in rank order; their compressed rank is the position here
R, A0, H0, B0 = R[order], A0[order], H0[order], B0[order]
measured = B0.max() - A0.min()
# prologue: a successor that found its hand-over complete -- first instruction to hand-over in
done_before = B0[:, :-1] <= A0[:, 1:]
prologue = float(np.median((H0[:, 1:] - A0[:, 1:])[done_before])) if done_before.any() else 1.0
# hop: producer's last instruction to the hand-over being in, for successors already resident
res = ~done_before
hop = float(np.median((H0[:, 1:] - B0[:, :-1])[res])) if res.any() else prologue
# fill rate: the first `slots` workgroups start as fast as the dispatcher hands them out
starts = np.sort(A0[:, 0])[: min(slots, n)]
rate = float(starts[-1] - starts[0]) / max(len(starts) - 1, 1)
tail_cost = np.maximum(R[:, 3] - np.median(R[:, :3], axis=1), 1.0)
print("trace: %d envs, launch %.1f us; prologue %.2f us, hop %.2f us, fill %.4f us per workgroup (%.1f us for %d slots)" % (
    n, measured, prologue, hop, rate, rate * min(slots, n), slots))
print("job times (us): parts 0-2 median %.1f, part 3 median %.1f, of it the tail (final pass + write-back) median %.1f; sum per env median %.1f" % (
    np.median(R[:, :3]), np.median(R[:, 3]), np.median(tail_cost), np.median(R.sum(1))))
print("work / slots = %.1f us" % (R.sum() / slots))


def build(classes, tail, shift):
    """the index order of csrc/sim_plan.h: by stage, within a stage by rank -> list of (rank, j, n_wg of its class, parts)"""
    out = []
    for stage in range(-4, 9):
        for c, (lo, hi, parts) in enumerate(classes):
            j = stage - (shift if c else 0)
            if 0 <= j < parts + tail:
                out += [(r, j, parts + tail, parts) for r in range(lo, hi)]
    return out


def job(r, j, parts, tail):
    """run time once the hand-over is in (part 0: from the first instruction), as the trace's `last - handed`"""
    if j == parts:
        return tail_cost[r]
    per = 4 // parts
    t = R[r, j * per:(j + 1) * per].sum() - (per - 1) * prologue
    if tail and j == parts - 1:
        t -= tail_cost[r]
    return t


def replay(classes, tail, shift):
    wgs = build(classes, tail, shift)
    free = [0.0] * slots
    heapq.heapify(free)
    end = {}
    t_disp = -rate
    busy = 0.0
    for r, j, n_wg, parts in wgs:
        t_disp = max(t_disp + rate, heapq.heappop(free))
        begin = t_disp if j == 0 else max(t_disp + prologue, end[(r, j - 1)] + hop)
        fin = begin + job(r, j, parts, tail)
        end[(r, j)] = fin
        busy += fin - t_disp
        heapq.heappush(free, fin)
    length = max(end.values())
    return length, 100.0 * (1.0 - busy / (slots * length)), len(wgs)


base, empty, n_wg = replay([(0, n, 4)], 0, 0)
err = base - measured
print("replay of the traced order: %.1f us predicted against %.1f us measured (error %+.1f us, %+.1f %%), empty %.1f %%" % (
    base, measured, err, 100 * err / measured, empty))
print("a candidate's predicted gain counts only beyond that error.")
rows = [("T", [(0, n, 4)], 1, 0)]
for k in [int(x) for x in a.k.split(",")]:
    k = min(k, n)                                        # (a trace holds the envs that were not reset: a few dozen short of the launch)
    rows.append(("C%d" % k, [(0, n - k, 4), (n - k, n, 2)], 0, 0))
    rows.append(("T+C%d" % k, [(0, n - k, 4), (n - k, n, 2)], 1, 0))
    for sh in (-1, 1):
        rows.append(("S%d:%d" % (k, sh), [(0, n - k, 4), (n - k, n, 4)], 0, sh))
        rows.append(("T+S%d:%d" % (k, sh), [(0, n - k, 4), (n - k, n, 4)], 1, sh))
res = []
for name, classes, tail, shift in rows:
    length, empty, n_wg = replay(classes, tail, shift)
    res.append((length, name, empty, n_wg))
print("plans by predicted launch length (parent replayed: %.1f us):" % base)
for length, name, empty, n_wg in sorted(res):
    print("  %-14s %6d workgroups  %7.1f us  %+6.1f us  empty %4.1f %%" % (name, n_wg, length, length - base, empty))

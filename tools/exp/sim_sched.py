"""Schedule of ONE rigid-body launch of the bench workload, workgroup by workgroup (run on the GPU box):

    EMLOCO_HIPCC_EXTRA_SIM="-DEMLOCO_SIM_SCHED=1" python -m emloco_amd.build --force      # diagnostic build
    python tools/exp/sim_sched.py [--envs 4096] [--steps 150]

Needs a library built with -DEMLOCO_SIM_SCHED=1: every workgroup then leaves its wall clock (100 MHz) at its first
instruction, once its predecessor's hand-over is in and at its last instruction (sim_kernels.hip, SCHED_HANDED).  Prints the
launch length, the split of the slot-time (running / waiting for the predecessor / empty), the longest env chains, the
hop time (predecessor's last instruction -> successor has the hand-over) and the run time against the contact-work key."""
import argparse
import ctypes as C
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np
import torch
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=150, help="steps of the rollout loop before the launch that is traced")
ap.add_argument("--slots", type=int, default=3072, help="wave slots of the device for this kernel: 256 CUs x 12")
a = ap.parse_args()
E = a.envs
env = bench.make_env(E, 0)
task = env.task
task.sim.native.set_cost_order(True)
dev = task.device
env.reset(torch.arange(E, device=dev))
bench.stagger_episodes(env, seed=0)
g = torch.Generator(device=dev)
g.manual_seed(1234)
pool = torch.randn(64, E, 69, device=dev, generator=g) * float(np.exp(-2.9))
for k in range(a.steps):
    env.reset_done()
    env.step(pool[k % 64])
torch.cuda.synchronize()
lib = task.sim.native.lib
SENT = 0xFFFFFFFFFFFFFFFF
key_prev = (C.c_uint * E)()
st = (C.c_ulonglong * (16 * E))(*([SENT] * (16 * E)))
lib.emloco_sim_cost_ticks.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_int]
assert lib.emloco_sim_cost_ticks(task.sim.native._h, key_prev, st, E) == 0      # allocates the stamps; key_prev: what the next launch is ordered by
if st[16 * E - 1] == SENT:
    raise SystemExit("this library was not built with -DEMLOCO_SIM_SCHED=1 (see the head of this file)")
for k in range(3):
    env.reset_done()
    env.step(pool[(a.steps + k) % 64])
torch.cuda.synchronize()
key = (C.c_uint * E)()
assert lib.emloco_sim_cost_ticks(task.sim.native._h, key, st, E) == 0
s = np.array(st[:], dtype=np.int64).reshape(4, E, 4)
n_parts = int((s[:, :, 2] > 0).any(axis=1).sum())
s = s[:n_parts]
# envs whose parts all ran in the latest full launch: the reset envs go through the unsplit list launch, their later parts' stamps
# are a step old (launches start ~420 us apart and last ~350)
med = np.median(s[n_parts - 1, :, 2])
ran = ((np.abs(s[:, :, 0] - med) < 35000) & (np.abs(s[:, :, 2] - med) < 35000)).all(axis=0)
us = 0.01                                            # 100 MHz
t_first, t_hand, t_last = s[:, :, 0].astype(np.float64) * us, s[:, :, 1].astype(np.float64) * us, s[:, :, 2].astype(np.float64) * us
slot = s[:, :, 3] >> 8
t0 = t_first[:, ran].min()
t_first -= t0; t_hand -= t0; t_last -= t0
length = t_last[:, ran].max()
print("envs %d (traced %d), parts %d, launch length (first instruction -> last instruction of any workgroup) %.1f us" % (E, ran.sum(), n_parts, length))
run = (t_last - t_hand)[:, ran].sum()
wait = (t_hand - t_first)[1:, ran].sum() if n_parts > 1 else 0.0
run += (t_hand - t_first)[0, ran].sum()              # a first part's state load is its own work
tot = a.slots * length
print("slot-time (%d slots x launch): running %.1f %%, waiting for the predecessor %.1f %%, empty %.1f %%" % (
    a.slots, 100 * run / tot, 100 * wait / tot, 100 * (tot - run - wait) / tot))
if n_parts > 1:
    hop = (t_hand[1:] - t_last[:-1])[:, ran]                               # predecessor's last instruction -> hand-over complete
    queued = np.maximum(t_first[1:] - t_last[:-1], 0.0)[:, ran]            # of it: the successor had no slot yet
    res = t_first[1:, ran] <= t_last[:-1, ran]                             # successor resident before its predecessor ended
    print("hop (predecessor's last instruction -> hand-over complete), all %d: median %.2f  p90 %.2f  max %.2f us" % (
        hop.size, np.median(hop), np.percentile(hop, 90), hop.max()))
    print("  of it queued for a slot: median %.2f  p90 %.2f  max %.2f us;  hop less queueing: median %.2f  p90 %.2f  max %.2f us" % (
        np.median(queued), np.percentile(queued, 90), queued.max(), np.median(hop - queued), np.percentile(hop - queued, 90), (hop - queued).max()))
    if res.any():
        print("  successors already resident (%d): hop median %.2f  p90 %.2f us" % (res.sum(), np.median(hop[res]), np.percentile(hop[res], 90)))
    pick = (t_hand[1:] - t_first[1:])[:, ran]
    print("  successor's first instruction -> hand-over complete: median %.2f  p90 %.2f  max %.2f us" % (np.median(pick), np.percentile(pick, 90), pick.max()))
chain_end = t_last[n_parts - 1]
ids = np.where(ran)[0]
top = ids[np.argsort(chain_end[ids])[::-1][:20]]
print("the 20 env chains that end last (us; launch %.1f):" % length)
print("   env   key slot0  start   end | run per part | queued for a slot per part | hop per part")
keyv = np.array(key[:], dtype=np.int64)
for e in top:
    runp = [t_last[p, e] - (t_hand[p, e] if p else t_first[p, e]) for p in range(n_parts)]
    qd = [max(t_first[p, e] - t_last[p - 1, e], 0.0) for p in range(1, n_parts)]
    hp = [t_hand[p, e] - t_last[p - 1, e] for p in range(1, n_parts)]
    print("  %5d %4d %5d %6.1f %6.1f | %s | %s | %s" % (e, keyv[e], slot[0, e], t_first[0, e], chain_end[e], " ".join("%5.1f" % x for x in runp),
                                                     " ".join("%5.1f" % x for x in qd), " ".join("%5.2f" % x for x in hp)))
chain = (chain_end - t_first[0])[ran]
print("env chain (first part's start -> last part's end): median %.1f  p90 %.1f  max %.1f us; sum of an env's run times: median %.1f  max %.1f us" % (
    np.median(chain), np.percentile(chain, 90), chain.max(), np.median((t_last - np.vstack([t_first[:1], t_hand[1:]]))[:, ran].sum(0)),
    (t_last - np.vstack([t_first[:1], t_hand[1:]]))[:, ran].sum(0).max()))
print("run time of a part against the env's contact-work key of this step (key = sum over substeps of 10 + contacts):")
runs = (t_last - np.vstack([t_first[:1], t_hand[1:]]))[:, ran]
kk = keyv[ran]
edges = [0, 1, 41, 61, 81, 101, 141, 201, 1 << 30]
for lo, hi in zip(edges[:-1], edges[1:]):
    m = (kk >= lo) & (kk < hi)
    if m.any():
        print("  key %4d..%-4s: %5d envs, part run time mean %5.1f  median %5.1f  p90 %5.1f us" % (
            lo, str(hi - 1) if hi < (1 << 30) else "", m.sum(), runs[:, m].mean(), np.median(runs[:, m]), np.percentile(runs[:, m], 90)))
print("env 0: run time per part %s us" % " ".join("%.1f" % x for x in (t_last - np.vstack([t_first[:1], t_hand[1:]]))[:, 0]))

"""Schedule of ONE rigid-body launch of the bench workload, workgroup by workgroup (run on the GPU box):

    EMLOCO_HIPCC_EXTRA_SIM="-DEMLOCO_SIM_SCHED=1" python -m emloco_amd.build --force      # diagnostic build
    python tools/exp/sim_sched.py [--envs 4096] [--steps 150] [--plan T+C1024] [--dump trace.npz]

Needs a library built with -DEMLOCO_SIM_SCHED=1: every workgroup then leaves its wall clock (100 MHz) at its first
instruction, once its predecessor's hand-over is in and at its last instruction (sim_kernels.hip, SCHED_HANDED).  Prints the
launch length, the split of the slot-time (running / waiting for the predecessor / empty), the longest env chains, the
hop time (predecessor's last instruction -> successor has the hand-over) and the run time against the contact-work key; then
the resident workgroups against time in 5 us bins, the empty slot-time in three stretches (until the first slot turns over / between /
after the last workgroup is dispatched) and the run time per part index and cost-key class.  --plan: the part plan of the launch
(EMLOCO_SIM_PLAN, emloco_amd/sim.py: plan_from_spec); --dump: the stamps as an .npz for tools/exp/sim_replay.py.  Envs may differ in
their number of parts under a plan; an env counts as traced when a gap-free run of its parts, at least two, lies in the launch."""
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
ap.add_argument("--plan", default=None, help="part plan of the launch (sets EMLOCO_SIM_PLAN)")
ap.add_argument("--dump", default=None, help="write the stamps of the traced envs to this .npz")
a = ap.parse_args()
if a.plan is not None:
    os.environ["EMLOCO_SIM_PLAN"] = a.plan
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
st = (C.c_ulonglong * (20 * E))(*([SENT] * (20 * E)))        # [5 parts][n_env][4]; a library from before the part plan fills [4 parts]
lib.emloco_sim_cost_ticks.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong), C.c_int]
assert lib.emloco_sim_cost_ticks(task.sim.native._h, key_prev, st, E) == 0      # allocates the stamps; key_prev: what the next launch is ordered by
P_MAX = 5 if st[20 * E - 1] != SENT else 4
if st[16 * E - 1] == SENT:
    raise SystemExit("this library was not built with -DEMLOCO_SIM_SCHED=1 (see the head of this file)")
for k in range(3):
    env.reset_done()
    env.step(pool[(a.steps + k) % 64])
torch.cuda.synchronize()
key = (C.c_uint * E)()
assert lib.emloco_sim_cost_ticks(task.sim.native._h, key, st, E) == 0
s_all = np.array(st[:16 * E if P_MAX == 4 else 20 * E], dtype=np.uint64).reshape(P_MAX, E, 4)
wg_index = (s_all[:, :, 3] >> np.uint64(32)).astype(np.int64)          # workgroup index (0 from a library from before the part plan)
s_all = s_all.astype(np.int64)
s_all[:, :, 3] &= 0xFFFFFFFF
# parts that ran in the latest full launch: the reset envs go through the unsplit list launch, their later parts' stamps are a step
# old (launches start ~420 us apart and last ~350), and under a plan an env has two to five parts
med = np.median(s_all[1, :, 2][s_all[1, :, 2] > 0])
have_all = (s_all[:, :, 2] > 0) & (np.abs(s_all[:, :, 0] - med) < 35000) & (np.abs(s_all[:, :, 2] - med) < 35000)
n_of = np.cumprod(have_all, axis=0).sum(axis=0)                        # gap-free run of parts from part 0
ran_all = (n_of >= 2) & (have_all.sum(axis=0) == n_of)
kinds = sorted(set(n_of[ran_all].tolist()))
print("parts per env among the traced envs: %s" % ", ".join("%d parts: %d envs" % (k, (n_of[ran_all] == k).sum()) for k in kinds))
# the tables of the uniform launch below follow the envs of the most common part count; the plan tables at the end take them all
n_parts = int(np.bincount(n_of[ran_all]).argmax())
s = s_all[:n_parts]
ran = ran_all & (n_of == n_parts)
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

# ---------------------------------------------------------------------------------------------------- the launch as a whole
# every traced workgroup, whatever its env's part count: a = first instruction, h = hand-over in, b = last instruction (us from the
# launch's first instruction)
pp, ee = np.nonzero(have_all & ran_all[None, :])
A = s_all[pp, ee, 0] * us
H = s_all[pp, ee, 1] * us
B = s_all[pp, ee, 2] * us
H = np.where(pp == 0, A, H)
z = A.min()
A, H, B = A - z, H - z, B - z
L = B.max()
last_of = n_of[ee] - 1 == pp


def busy(lo, hi):
    """slot-time of resident workgroups inside [lo, hi)"""
    return np.clip(np.minimum(B, hi) - np.maximum(A, lo), 0.0, None).sum()


print()
print("launch as a whole: %d workgroups of %d envs, %.1f us, slot-time resident %.1f %% (running %.1f %%, waiting %.1f %%), empty %.1f %%" % (
    len(A), ran_all.sum(), L, 100 * busy(0, L) / (a.slots * L), 100 * (B - H).sum() / (a.slots * L), 100 * (H - A).sum() / (a.slots * L),
    100 * (1 - busy(0, L) / (a.slots * L))))
print("resident workgroups against time (5 us bins: mean resident, of %d slots):" % a.slots)
edges5 = np.arange(0.0, L + 5.0, 5.0)
occ = [busy(lo, lo + 5.0) / 5.0 for lo in edges5[:-1]]
for i in range(0, len(occ), 8):
    print("  %5.0f us: %s" % (edges5[i], " ".join("%4.0f" % x for x in occ[i:i + 8])))
t_turn, t_disp = B.min(), A.max()
print("empty slot-time in three stretches (slot-us; share of the launch's %d x %.1f):" % (a.slots, L))
for name, lo, hi in (("until the first slot turns over", 0.0, t_turn), ("between", t_turn, t_disp), ("after the last workgroup is dispatched", t_disp, L)):
    e = a.slots * (hi - lo) - busy(lo, hi)
    print("  %-40s %6.1f .. %6.1f us: %9.0f  %5.2f %%  (= %.1f us of launch length at full occupancy)" % (name, lo, hi, e, 100 * e / (a.slots * L), e / a.slots))
print("run time per part index and cost-key class (median us; count):")
kk_all = keyv[ee]
kedges = [0, 1, 41, 61, 81, 101, 141, 1 << 30]
print("  part   " + " ".join("%13s" % ("key %d..%s" % (lo, hi - 1 if hi < (1 << 30) else "")) for lo, hi in zip(kedges[:-1], kedges[1:])) + "   all")
for p in range(P_MAX):
    for fin in (False, True):
        m = (pp == p) & (last_of == fin)
        if not m.any():
            continue
        cells = []
        for lo, hi in zip(kedges[:-1], kedges[1:]):
            mk = m & (kk_all >= lo) & (kk_all < hi)
            cells.append("%6.1f (%4d)" % (np.median((B - H)[mk]), mk.sum()) if mk.any() else "      -      ")
        print("  %d%s    %s  %6.1f" % (p, "F" if fin else " ", " ".join(cells), np.median((B - H)[m])))
print("  (F: the env's final part -- final kinematics pass and write-back)")
if a.dump:
    np.savez(a.dump, env=ee, part=pp, n_parts=n_of[ee], key=keyv[ee], key_prev=np.array(key_prev[:], dtype=np.int64)[ee], first=A, handed=H, last=B,
             rank=s_all[pp, ee, 3] >> 8, wg=wg_index[pp, ee], slots=a.slots, length=L)
    print("stamps written to", a.dump)

"""Case table and judges of the pooled reset / observation launch (include/emloco_task.h: emloco_task_reset_obs_pooled; reset_obs_kernel in
emloco_amd/csrc/chain_kernels.hip), shared by the emulator run on the CPU (tests/test_chain_cpu.py) and the device run
(tests/test_gpu_chain.py): the two differ in the executor only.  The world is tests/reset_cases.py's: 300 varied models, the synthetic
motion cache with its edge clips, a sloped non-square map, distinguishable real paths.

A sequence (SEQUENCES) is a list of calls (n finished envs, seed, promised next seed, pool) on ONE state; the two pool buffers alternate
the way the task alternates them (this call's `next` is the following call's `cur`).  The LAST call is the judged one: it is run a second
time from the same state (a second executor that replayed the same earlier calls) with pool = NULL, and the two results are compared BIT
FOR BIT in every buffer a reset writes (reset_cases.OUT_KEYS), obs, flip_obs and the AMP buffer.  The direct run of every flag set is
judged against float64 by reset_cases.judge (trajectory, waypoints and the inversion flag included: kernel_refs.reset_trajectory), so
bit equality carries the float64 bars to the pooled runs and no float tolerance appears here.

What else is pinned, per call, against a model of the header's rules (pool_model):
  tags          entries [0, min(k, c + c / 4 + 32)) of `next` carry next_seed, c = ids[cap] the number of finished envs; the tags behind
                them and all of `cur` are as they were (sentinels, or the stale seed of two calls ago)
  pool floats   entries at or behind the draw count keep their sentinel; `cur` is not written
  rnd_ws        the kernel writes a row only for an entry that takes the direct path and nothing reads the workspace after the launch.
                Rows of pool-hit entries keep their sentinel, rows of direct entries equal the direct run's, rows behind the list are
                untouched.  (The header says so: dev_rnd_ws is scratch.)
  hits          which entries hit follows the model (entry < k, tag == seed, seed != 0) and is what the rnd_ws rows show

Sizes are the smallest at which this code can go wrong: k = 64 / 8 / 256 against lists of 0, 1, 12, 20, 40, 50 and 258 entries (258 > 256
reset workgroups: workgroups 0 and 1 walk a pooled entry and then a direct one through the same LDS).

DIRECT_CASES are single launches with supplied random rows (a pool is passed and must be ignored): the rows that close branches no seeded
row reaches -- see tests/test_task_branches_cpu.py for which case closes which line.  A device uniform never exceeds TOP = 1 - 2^-24, and
float32(TOP n) < n for every n (n 2^-24 is at least one ulp below n), so the clamps of reset_pick_motion / the placement pick are
reachable only by a caller-supplied uniform of 1.0: that is the row used, not TOP.
"""
import functools

import numpy as np
import torch

import kernel_refs as R
import reset_cases as RC

E, RND, POOL_FLOATS = RC.E, RC.RND, 512
POST_OBS, POST_AMP_SHIFT, POST_AMP_ROW = 2, 16, 32
LIVE = POST_OBS | POST_AMP_SHIFT | POST_AMP_ROW
OBS = 1422
TAG_SENT = 0xDEADBEEFCAFEF00D                  # tag of a pool entry before any launch (no call uses it as a seed)
POOL_SENT = -1234.5                            # every float of a pool entry before any launch
WS_SENT = -4321.25                             # every float of the random workspace before the judged call
EXTRA_KEYS = ("obs", "flip_obs")
SEEDS = (0x9E3779B97F4A7C15, 0x51A7E5EED0C0FFEE, 0x0000000100000002, 0xFFFFFFFF00000001, 0x123456789ABCDEF1)
WRONG_SEED = 0x0BADC0DE0BADC0DE
BASE_FLAGS = RC.RANDOM_HEADING | RC.INIT_HEADING


def call(n, seed=None, pool=True, live=0, cap=None):
    return dict(n=n, seed=seed, pool=pool, live=live, cap=cap)


# name -> (k, calls); seed None: SEEDS[i] for call i, next seed SEEDS[i + 1] (what the task promises)
SEQUENCES = {
    "all hits": (64, [call(40, cap=E), call(40, cap=E)]),                     # the task's own list: capacity E, -1 behind the finished envs
    "beyond the pool": (8, [call(12), call(12)]),                            # entries 8..11 take the direct path
    "draw count": (64, [call(1), call(50)]),                                 # 33 drawn: 0..32 hit, 33 is the first direct one, tags 33..63 untouched
    "empty first call": (64, [call(0), call(20)]),                           # n = 0 still launches and draws 32
    "wrong seed": (64, [call(40), call(40, seed=WRONG_SEED)]),               # nothing hits
    "stride": (256, [call(258), call(258)]),                                 # workgroups 0, 1: a pooled entry, then entry 256 / 257 direct
    "three calls": (64, [call(40), call(10), call(40)]),                     # A, B, A: 44 drawn by call 2, all 40 hit
    "stale tags": (64, [call(40), call(10), call(8), call(50)]),             # call 3 redraws 42 of B: B[42..63] still carry call 2's seed
    "seed zero": (64, [call(20, seed=0)]),                                    # zeroed pool (as the task allocates it): a zero tag is "empty"
}
EXPECT_HITS = {"all hits": 40, "beyond the pool": 8, "draw count": 33, "empty first call": 20, "wrong seed": 0, "stride": 256, "three calls": 40,
               "stale tags": 42, "seed zero": 0}

# name -> what differs from the base setup (flags, amp_ring, scalars of EmlocoResetBufs)
FLAG_SETS = {
    "base": dict(flags=BASE_FLAGS),
    "inversion": dict(flags=RC.INIT_HEADING | RC.HEADING_INVERSION),
    "hybrid real": dict(flags=RC.REAL_PATH, scalars=dict(hybrid_prob=0.5)),
    "real adjust": dict(flags=RC.REAL_PATH | RC.ADJUST_ROOT_VEL),
    "random heading": dict(flags=RC.RANDOM_HEADING),
    "fixed location": dict(flags=RC.FIXED_LOCATION),
    "no history": dict(flags=BASE_FLAGS | RC.NO_AMP_HISTORY),
    "amp ring": dict(flags=BASE_FLAGS, amp_ring=6),
}
FLAG_SEQUENCES = ("all hits", "draw count")


def setup(flags=BASE_FLAGS, amp_ring=0, scalars=None, const=None):
    return dict(flags=flags, amp_ring=amp_ring, scalars=dict(scalars or {}), const=dict(const or {}), real_key=0)


def matrix():
    """(id, sequence name, setup): every sequence at the base flags, every other flag set under FLAG_SEQUENCES"""
    out = [(f"{s} / base", s, setup()) for s in SEQUENCES]
    out += [(f"{s} / {f}", s, setup(**kw)) for f, kw in FLAG_SETS.items() if f != "base" for s in FLAG_SEQUENCES]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# plans: the arguments of every call of a sequence, and the model of the pool's tags

def _ids(n, cap, rng):
    """[cap + 1]: n distinct envs ascending (the compaction's order), -1 behind them, ids[cap] = n"""
    ids = np.full(cap + 1, -1, np.int32)
    ids[:n] = np.sort(rng.permutation(E)[:n])
    ids[cap] = n
    return ids


def plan(name):
    k, calls = SEQUENCES[name]
    rng = np.random.default_rng(sorted(SEQUENCES).index(name) + 50)
    out = []
    for i, c in enumerate(calls):
        cap = c["cap"] if c["cap"] is not None else c["n"]
        seed = SEEDS[i] if c["seed"] is None else c["seed"]
        out.append(dict(n=c["n"], cap=cap, ids=_ids(c["n"], cap, rng), seed=seed, live=c["live"],
                        pool=dict(k=k, cur=i % 2, cur_tag=i % 2, next=1 - i % 2, next_tag=1 - i % 2, next_seed=SEEDS[i + 1]) if c["pool"] else None))
    return k, out


def draw_count(k, now):
    return min(k, now + now // 4 + 32)


def pool_model(k, calls, tag0):
    """the header's rules replayed on the tags alone: per call (hits [n] bool, tags after the call [2][k])"""
    tags = [[tag0] * k, [tag0] * k]
    out = []
    for c in calls:
        p = c["pool"]
        hits = np.zeros(c["n"], bool)
        if p is not None:
            for bi in range(min(c["n"], k)):
                hits[bi] = c["seed"] != 0 and tags[p["cur"]][bi] == c["seed"]
            for e in range(draw_count(k, c["n"])):
                tags[p["next"]][e] = p["next_seed"]
        out.append((hits, np.array(tags, dtype=np.uint64)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the run of a sequence on two executors
#
# An executor is built from (setup, k, zero_pool) on the initial state reset_cases.initial() and offers
#   launch(ids, cap, seed, pool, live_mode=0, skip=None, rnd=None, real_pick=None) -> return code       pool: None or dict(k, cur, cur_tag, next,
#                                                                      next_tag: index 0 / 1 of its two pool buffers or None, next_seed)
#   post_physics(mode, env_ids)                  emloco_task_post_physics of the listed envs
#   refill()                                     sentinels into rnd_ws (WS_SENT), NaN into obs / flip_obs
#   snapshot() -> dict of numpy copies           OUT_KEYS, obs, flip_obs, ws [E][512], pool [2][k][512], tag [2][k] uint64

def compare(a, b, what, keys=RC.OUT_KEYS + EXTRA_KEYS):
    bad = [k for k in keys if not RC.same_bits(a[k], b[k])]
    assert not bad, (what, "buffers that differ bit for bit", bad)


def check_pool(before, after, c, model_tags, what):
    """tags and pool floats after a call against the model: drawn entries carry next_seed, everything else is as it was"""
    p = c["pool"]
    assert np.array_equal(after["tag"], model_tags), (what, "tags differ from min(k, c + c / 4 + 32) entries of next_seed")
    if p is None:
        assert RC.same_bits(after["pool"], before["pool"]), (what, "a pool buffer was written without a pool")
        return
    cnt = draw_count(p["k"], c["n"])
    assert RC.same_bits(after["pool"][p["cur"]], before["pool"][p["cur"]]), (what, "`cur` was written")
    assert RC.same_bits(after["pool"][p["next"]][cnt:], before["pool"][p["next"]][cnt:]), (what, "an entry at or behind the draw count was written")
    drawn = after["pool"][p["next"]][:cnt]
    # root 13 | gh | time | inv byte | clip id | dof 138 | verts 303 | waypoints 45: floats [0, 15), [20, 158), [160, 463), [464, 509)
    for lo, hi in ((0, 15), (20, 158), (160, 463), (464, 509)):
        assert np.isfinite(drawn[:, lo:hi]).all() and not (drawn[:, lo:hi] == POOL_SENT).any(), (what, "a drawn entry holds an unwritten float", lo)


def run_sequence(make, name, su, zero_pool=False):
    """both executors through the sequence; returns dict(calls, hits, before, pooled, direct): the judged call's arguments, its model
    hits, the state before it and after it with the pool and with pool = NULL"""
    k, calls = plan(name)
    zero_pool = zero_pool or name == "seed zero"
    A, B = make(su, k, zero_pool), make(su, k, zero_pool)
    model = pool_model(k, calls, 0 if zero_pool else TAG_SENT)
    for i, c in enumerate(calls):
        last = i == len(calls) - 1
        if last:
            A.refill()
            B.refill()
            before = B.snapshot()
            compare(A.snapshot(), before, (name, "the two executors disagree before the judged call"), RC.OUT_KEYS + EXTRA_KEYS + ("ws", "pool"))
        sa = A.snapshot()
        assert A.launch(c["ids"], c["cap"], c["seed"], c["pool"], c["live"]) == 0
        assert B.launch(c["ids"], c["cap"], c["seed"], None if last else c["pool"], c["live"]) == 0
        check_pool(sa, A.snapshot(), c, model[i][1], (name, "call", i))
    pooled, direct = A.snapshot(), B.snapshot()
    c, hits = calls[-1], model[-1][0]
    assert int(hits.sum()) == EXPECT_HITS[name], (name, "the model's hit count", int(hits.sum()))
    compare(pooled, direct, (name, "pooled against pool = NULL"))
    # the random workspace: hit rows keep the sentinel, direct rows are the direct run's, rows behind the list are untouched
    n = c["n"]
    assert (pooled["ws"][:n][hits] == WS_SENT).all(), (name, "a pool-hit entry's random row was written")
    assert RC.same_bits(pooled["ws"][:n][~hits], direct["ws"][:n][~hits]), (name, "a direct entry's random row differs")
    assert (direct["ws"][:n] != WS_SENT).all() and (pooled["ws"][n:] == WS_SENT).all() and (direct["ws"][n:] == WS_SENT).all(), (name, "random rows")
    check_pool(before, direct, dict(c, pool=None), model[-2][1] if len(calls) > 1 else before["tag"], (name, "the direct run"))
    return dict(call=c, hits=hits, before=before, pooled=pooled, direct=direct)


def judge_direct(name, su, res, tab, fails, shares=None):
    """the direct run of a judged call against float64 (reset_cases.judge on the rows the seed makes, the real-path key the seed makes)"""
    c = res["call"]
    n, seed = c["n"], c["seed"]
    RC.judge_rnd(c["ids"][:c["cap"]], c["cap"], seed, res["direct"]["ws"][:c["cap"]], np.full((c["cap"], RND), WS_SENT, np.float32), fails)
    case = dict(name=name, n=n, ids=c["ids"][:n], rnd=res["direct"]["ws"][:n], flags=su["flags"], amp_ring=su["amp_ring"], scalars=su["scalars"],
                const=su["const"], real_key=R.seeded_real_key(seed), traj=True)
    RC.judge(case, res["before"], res["direct"], tab, fails, shares, history=not su["flags"] & RC.NO_AMP_HISTORY, amp_row0=False)
    judge_flag_mix(name, su, case, res["direct"])
    return case


def judge_flag_mix(name, su, case, out):
    """a flag set is exercised only if both sides of its draw occur: asserted on the float64 side (the rows), then on the output"""
    u = torch.as_tensor(case["rnd"])
    env = case["ids"][:case["n"]]
    if case["n"] < 20:
        return
    if su["flags"] & RC.HEADING_INVERSION:
        inv = (u[:, R.RND_INVERSION] > 0.5).numpy()
        assert inv.any() and not inv.all(), (name, "the rows invert all or none")
        assert np.array_equal(out["inverted"][env], inv.astype(np.uint8)), (name, "inverted")
    if su["flags"] & RC.REAL_PATH and su["scalars"].get("hybrid_prob", 0.0) > 0.0:
        real = (u[:, RC.RND_REAL] > torch.tensor(su["scalars"]["hybrid_prob"], dtype=torch.float32)).numpy()
        assert real.any() and not real.all(), (name, "the rows make all or no entry a real path")
        z = out["traj_verts"][env].reshape(case["n"], RC.NV, 3)[:, 0, 2]
        assert (z[~real] == 0).all() and len(set(z[real].tolist())) == int(real.sum()), (name, "real and generated paths")


# ---------------------------------------------------------------------------------------------------------------------------------
# single launches with supplied rows (the pool passed beside them is ignored); each judged against float64

@functools.lru_cache(maxsize=None)
def still_const():
    """the world's motion cache with a root that stands still in the near-identity clip (zero root velocity in every frame)"""
    W = RC.world()
    gvs = W.cache["gvs"].clone()
    s = int(W.cache["motion_start"][RC.CLIP_NEAR])
    gvs[s:s + RC.CLIP_FRAMES[RC.CLIP_NEAR], 0] = 0.0
    return dict(gvs=gvs)


def _empty_row(r):
    return (r % 3 == 2) & (r != RC.N_REAL - 1)


@functools.lru_cache(maxsize=None)
def edge_const():
    """the world's real paths with a first segment of 1e-5 m (row % 3 == 1: shorter than speed_min vert_dt = 2.8e-5 m) or an empty one
    (row % 3 == 2, but for the last row, which the clamp of an explicit row lands on)"""
    real = RC.world().real.clone()
    r = torch.arange(RC.N_REAL)
    real[r % 3 == 1, 1, 0] = 1e-5
    real[_empty_row(r), 1, 0] = 0.0
    return dict(real_traj=real)


def _rows(n, seed):
    return torch.rand(n, RND, generator=R._gen(seed))


def direct_cases():
    """name -> (setup, ids [n + 1], rnd [n][512], real_pick or None)"""
    out = {}
    rng = np.random.default_rng(77)
    n = 24
    # a uniform of exactly 1.0 in the clip and the placement draw: both picks are clamped to the last entry
    rnd = _rows(n, 1)
    rnd[0::3, RC.RND_MOTION] = 1.0
    rnd[1::3, RC.RND_LOC] = 1.0
    rnd[2, RC.RND_MOTION], rnd[2, RC.RND_LOC] = RC.TOP, RC.TOP
    out["uniform of one"] = (setup(RC.RANDOM_HEADING), _ids(n, n, rng), rnd, None)
    # explicit real-path rows outside the table (clamped into it) and first segments shorter than speed_min vert_dt, under the speed
    # adjustment and the heading alignment
    pick = np.array([-3, RC.N_REAL + 5, -1, RC.N_REAL, 0, RC.N_REAL - 1] + [r for r in range(1, 40) if r % 3 != 2][:n - 6], np.int32)
    out["real-path edges"] = (setup(RC.REAL_PATH | RC.ADJUST_ROOT_VEL | RC.INIT_HEADING, const=edge_const()), _ids(n, n, rng), _rows(n, 2), pick)
    # an empty first segment has no heading to align
    pick = np.arange(n, dtype=np.int32)
    out["empty first segment"] = (setup(RC.REAL_PATH | RC.INIT_HEADING, const=edge_const()), _ids(n, n, rng), _rows(n, 3), pick)
    # a root that stands still: no heading to align with, ratio 0 under ADJUST_ROOT_VEL (every segment at speed_min)
    rnd = _rows(n, 4)
    rnd[0::2, RC.RND_MOTION] = (RC.CLIP_NEAR + 0.5) / len(RC.CLIP_FRAMES)
    out["still root"] = (setup(RC.INIT_HEADING | RC.ADJUST_ROOT_VEL, const=still_const()), _ids(n, n, rng), rnd, None)
    # REAL_PATH without a table (n_real = 0: every path is generated), and a trajectory shorter than the waypoints' span: lanes whose
    # sample time lies behind traj_dur = 3 s (0.4 s apart: lanes 8..14) take the last vertex
    out["no real table, short trajectory"] = (setup(RC.REAL_PATH, scalars=dict(n_real=0, traj_dur=3.0)), _ids(n, n, rng), _rows(n, 5), None)
    return out


def run_direct(make, name, tab, fails):
    su, ids, rnd, pick = direct_cases()[name]
    n = len(ids) - 1
    rnd = np.ascontiguousarray(rnd.numpy())
    X = make(su, 8, False)
    X.refill()
    before = X.snapshot()
    pool = dict(k=8, cur=0, cur_tag=0, next=1, next_tag=1, next_seed=SEEDS[1])
    assert X.launch(ids, n, SEEDS[0], pool, 0, None, rnd=rnd, real_pick=pick) == 0
    out = X.snapshot()
    # rows supplied: the pool is ignored (`next` and its tags keep their sentinels), the workspace is not written
    assert RC.same_bits(out["pool"], before["pool"]) and np.array_equal(out["tag"], before["tag"]), (name, "the pool was used beside supplied rows")
    assert RC.same_bits(out["ws"], before["ws"]), (name, "the random workspace was written beside supplied rows")
    case = dict(name=name, n=n, ids=ids[:n], rnd=rnd, flags=su["flags"], amp_ring=0, scalars=su["scalars"], const=su["const"], real_key=0,
                real_pick=pick, traj=True)
    RC.judge(case, before, out, tab, fails, amp_row0=False)
    return case, before, out


def check_direct_edges(name, case, out):
    """the edge a direct case is there for occurs in its rows (asserted on the float64 side)"""
    W = RC.world()
    u, env, n = torch.as_tensor(case["rnd"]), case["ids"], case["n"]
    M = len(RC.CLIP_FRAMES)
    if name == "uniform of one":
        assert (u[:, RC.RND_MOTION] * float(M) >= M).any() and (u[:, RC.RND_LOC] * float(RC.N_VALID) >= RC.N_VALID).any()
        assert not (torch.tensor([RC.TOP]) * float(M) >= M).any() and not (torch.tensor([RC.TOP]) * float(RC.N_VALID) >= RC.N_VALID).any()
        assert (out["motion_ids"][env][0::3] == M - 1).all()
        assert (out["root_state"][env][1::3, 0] == W.valid_x[-1].item()).all()
    elif name in ("real-path edges", "empty first segment"):
        rows = np.clip(case["real_pick"][:n].astype(np.int64), 0, RC.N_REAL - 1)
        empty = _empty_row(rows)
        if name == "real-path edges":
            assert (case["real_pick"] < 0).any() and (case["real_pick"] >= RC.N_REAL).any() and (rows % 3 == 1).any() and not empty.any()
        else:
            assert empty.any() and not empty.all()
        assert np.array_equal(out["traj_verts"][env].reshape(n, RC.NV, 3)[:, 0, 2], rows.astype(np.float32))
    elif name == "no real table, short trajectory":
        v = out["traj_verts"][env].reshape(n, RC.NV, 3)
        w = out["waypoint_traj"][env].reshape(n, RC.NS, 3)
        assert (v[:, :, 2] == 0).all() and RC.same_bits(w[:, 8:], np.repeat(v[:, -1:], RC.NS - 8, axis=1))
    elif name == "still root":
        still = out["motion_ids"][env] == RC.CLIP_NEAR
        assert still.any() and not still.all()
        assert (out["root_state"][env][still, 7:10] == 0).all() and (out["init_vel"][env][still] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the live role beside a pool: role indices S | 2 k | E | 14 S

def run_live(make):
    """call 1 resets every env (so that every env holds a state the observations can be built from); call 2 resets 40 of them from the
    pool with live_mode = OBS | AMP_SHIFT | AMP_ROW beside it.  Against: the same call 2 with live_mode = 0 followed by
    emloco_task_post_physics(live_mode) of the envs whose snapshot entry is zero.  Five envs are flagged in the snapshot without being
    listed: the live role must leave them alone (and the reset does not list them), so nothing of them changes."""
    k = 64
    su = setup()
    rng = np.random.default_rng(9)
    ids1 = _ids(E, E, rng)
    ids2 = _ids(40, E, rng)
    ids2[:40] = np.sort(1 + rng.permutation(E - 2)[:40])       # env 0 and the last env stay live (the two whose live workgroups stamp)
    listed = ids2[:40]
    rest = np.setdiff1d(np.arange(E), listed)
    flagged = rest[7::53][:5]
    skip = np.zeros(E, np.int64)
    skip[listed], skip[flagged] = 1, 3
    live = np.setdiff1d(rest, flagged).astype(np.int32)
    p1 = dict(k=k, cur=0, cur_tag=0, next=1, next_tag=1, next_seed=SEEDS[1])
    p2 = dict(k=k, cur=1, cur_tag=1, next=0, next_tag=0, next_seed=SEEDS[2])
    A, B = make(su, k, False), make(su, k, False)
    for X in (A, B):
        assert X.launch(ids1, E, SEEDS[0], p1, 0, None) == 0
        X.refill()
    before = B.snapshot()
    assert A.launch(ids2, E, SEEDS[1], p2, LIVE, skip) == 0
    assert B.launch(ids2, E, SEEDS[1], p2, 0, None) == 0
    padded = np.full(len(live) + 3, -1, np.int32)               # emloco_task_post_physics skips negative ids anywhere in its list
    padded[[i for i in range(len(padded)) if i not in (0, 100, len(padded) - 1)]] = live
    B.post_physics(LIVE, padded)
    fused, sep = A.snapshot(), B.snapshot()
    compare(fused, sep, "live role beside a pool against post_physics of the live envs", RC.OUT_KEYS + EXTRA_KEYS + ("ws", "pool"))
    assert np.array_equal(fused["tag"], sep["tag"])
    assert (fused["ws"][:40] == WS_SENT).all(), "all 40 entries come from the pool"
    for key in RC.OUT_KEYS + EXTRA_KEYS:
        assert RC.same_bits(fused[key][flagged], before[key][flagged]), (key, "an env flagged in the snapshot was touched")
    assert np.isfinite(fused["obs"][live]).all() and np.isfinite(fused["obs"][listed]).all() and np.isnan(fused["obs"][flagged]).all()
    assert not RC.same_bits(fused["amp"][live], before["amp"][live]), "the live envs' AMP rows did not move"
    # an empty list without a pool: only the live role runs (here the history shift without a new row), on every env the snapshot leaves
    none = np.zeros(1, np.int32)
    mode = POST_OBS | POST_AMP_SHIFT
    free = np.flatnonzero(skip == 0).astype(np.int32)
    assert A.launch(none, 0, SEEDS[2], None, mode, skip) == 0
    B.post_physics(mode, free)
    fused, sep = A.snapshot(), B.snapshot()
    compare(fused, sep, "live role alone against post_physics", RC.OUT_KEYS + EXTRA_KEYS + ("ws", "pool"))
    # ... and without a live role there is nothing to launch: 0, nothing written
    assert A.launch(none, 0, SEEDS[2], None, 0, None) == 0
    compare(A.snapshot(), fused, "an empty call wrote", RC.OUT_KEYS + EXTRA_KEYS + ("ws", "pool"))


# ---------------------------------------------------------------------------------------------------------------------------------
# refused pool arguments (include/emloco_task.h: "Rules"): buffers by index 0 / 1 of the executor's two pool buffers

REFUSED = {
    "k < 0": dict(k=-1, cur=0, cur_tag=0, next=1, next_tag=1),
    "k > 4096": dict(k=4097, cur=0, cur_tag=0, next=1, next_tag=1),
    "cur without its tags": dict(k=8, cur=0, cur_tag=None, next=1, next_tag=1),
    "next without its tags": dict(k=8, cur=0, cur_tag=0, next=1, next_tag=None),
    "cur == next": dict(k=8, cur=0, cur_tag=0, next=0, next_tag=1),
    "cur_tag == next_tag": dict(k=8, cur=0, cur_tag=1, next=1, next_tag=1),
}
ACCEPTED = {
    "k == 0 with equal buffers": dict(k=0, cur=0, cur_tag=0, next=0, next_tag=0),          # no pool: nothing of it is read
    "no cur": dict(k=8, cur=None, cur_tag=None, next=1, next_tag=1),
    "no next": dict(k=8, cur=0, cur_tag=0, next=None, next_tag=None),
}


def run_refusals(make):
    k, calls = plan("beyond the pool")
    c = calls[0]
    X = make(setup(), 8, False)
    X.refill()
    before = X.snapshot()
    keys = RC.OUT_KEYS + EXTRA_KEYS + ("ws", "pool")
    for name, p in REFUSED.items():
        assert X.launch(c["ids"], c["cap"], c["seed"], dict(p, next_seed=SEEDS[1]), 0, None) != 0, (name, "was accepted")
        after = X.snapshot()
        compare(after, before, (name, "a refused call wrote"), keys)
        assert np.array_equal(after["tag"], before["tag"]), (name, "a refused call wrote tags")
    for name, p in ACCEPTED.items():
        assert X.launch(c["ids"], c["cap"], c["seed"], dict(p, next_seed=SEEDS[1]), 0, None) == 0, (name, "was refused")

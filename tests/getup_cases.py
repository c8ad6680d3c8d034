"""Case tables of the get-up entry points (include/emloco_task.h: emloco_getup_*), shared by the emulator run on the CPU
(tests/test_emu_getup.py) and the device run (tests/test_gpu_getup.py): the two differ in the executor only.  The reference is
tests/getup_ref.py; every comparison is exact (integer logic and copies).

Split: E = P = 300 -- more than one 256-entry stride, and not a power of four, so the Feistel walk of the slot permutation cycles.
Lists of 0, 1, 37, 261 and 300 entries, as explicit ascending ids (n = the entries) and as a compacted list (n = E, -1 behind the
entries, the count at [E]); probabilities (0, 0), (1, 0), (0, 1), (1, 1), (0.2, 0.1); terminate_buf mixed 0 / 1 / 2.  Pool states:
"mixed" (a third of the listed envs and a third of the others hold slots, a few slots are taken for good), "exact" (as many free
slots after the listed envs gave theirs back as there are fall entries) and "short" (fewer: the surplus turns normal)."""
import numpy as np

import getup_ref as GR

E = P = 300
NDOF, AMP_STEPS, AMP_ROW, MAXCAND = 69, 15, 206, 96
STEPS = 60
LENGTHS = (0, 1, 37, 261, 300)
PROBS = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.2, 0.1))
LIST_KEYS = ("normal", "fall", "recover", "fall_slot")
STATE_KEYS = ("pool_taken", "assign", "counter", "stats")


def _ids(m, kind, rng):
    valid = np.sort(rng.choice(E, size=m, replace=False)).astype(np.int32)
    if kind == "explicit":
        return valid.copy(), m
    return np.concatenate([valid, np.full(E - m, -1, np.int32), [m]]).astype(np.int32), E       # emloco_task_compact_done's layout


def state(rng):
    """the get-up buffers on the host: an empty pool (every slot free, no env holds one), garbage counters, mixed flags"""
    return dict(pool_root=rng.normal(size=(P, 13)).astype(np.float32), pool_dof=rng.normal(size=(P, NDOF, 2)).astype(np.float32),
                pool_taken=np.zeros(P, np.uint8), assign=np.full(E, -1, np.int32), counter=rng.integers(0, 99, E).astype(np.int32),
                progress=rng.integers(0, 200, E).astype(np.int64), reset=rng.integers(0, 2, E).astype(np.int64),
                terminate=rng.integers(0, 3, E).astype(np.int64),              # 2: not the value a termination leaves, never a recovery
                split_ws=np.full(P, -55, np.int32), stats=np.arange(6, dtype=np.int64) * 1000)


def _fill_pool(st, listed, target_free, rng):
    """slots held by listed envs (given back by the call) and by others (kept); with target_free: slots taken for good until exactly
    that many are free once the listed envs gave theirs back"""
    others = np.setdiff1d(np.arange(E), listed)
    n_in, n_out = len(listed) // 3, len(others) // 3
    if target_free is not None:
        n_out = min(n_out, P - target_free)
        n_in = min(n_in, target_free)
    slots = rng.permutation(P)
    holders = np.concatenate([rng.choice(listed, n_in, replace=False) if n_in else [], rng.choice(others, n_out, replace=False) if n_out else []]).astype(int)
    for e, s in zip(holders, slots):
        st["assign"][e] = s
        st["pool_taken"][s] = 1
    rest = slots[len(holders):]
    dead = 5 if target_free is None else P - n_out - target_free
    assert 0 <= dead <= len(rest)
    st["pool_taken"][rest[:dead]] = 1                                # taken for good: no env holds them


def split_case(m, kind, probs, pool, index, seeded=False):
    rng = np.random.default_rng(1000 + index)
    ids, n = _ids(m, kind, rng)
    rnd = None if seeded else rng.random((n, 2)).astype(np.float32)
    if rnd is not None:
        rnd[m:] = np.nan                                             # rows behind the entries are not read
    case = dict(name=f"m={m} {kind} p={probs} pool={pool}" + (" seeded" if seeded else ""), m=m, kind=kind, n=n, ids=ids, rnd=rnd, seed=0xC0FFEE1234 + index,
                recovery_prob=probs[0], fall_prob=probs[1], steps=STEPS, key=(0x1234ABCD + 77 * index) & 0xFFFFFFFF)
    st = state(rng)
    target = None
    if pool != "mixed":
        u = GR.uniforms(case, m)
        rec = (u[:, 0] < np.float32(probs[0])) & (st["terminate"][ids[:m]] == 1)
        want = int(((u[:, 1] < np.float32(probs[1])) & ~rec).sum())
        target = want if pool == "exact" else max(want - 3, 0)
        case["want_fall"], case["free"] = want, target
    _fill_pool(st, ids[:m], target, rng)
    return case, st


def split_cases():
    out, index = [], 0
    for m in LENGTHS:
        for kind in ("explicit", "compacted"):
            for probs in PROBS:
                out.append(split_case(m, kind, probs, "mixed", index))
                index += 1
    for m in (37, 261, 300):
        for probs in ((0.0, 1.0), (1.0, 1.0), (0.2, 0.1)):
            for pool in ("exact", "short"):
                out.append(split_case(m, "compacted" if m != 261 else "explicit", probs, pool, index))
                index += 1
    for m in (0, 37, 300):
        out.append(split_case(m, "compacted", (0.2, 0.1), "mixed", index, seeded=True))
        index += 1
    return out


def judge_split(case, st0, st, lists):
    """`st` / `lists`: what an executor left; against the reference, and the properties the header states"""
    ref_st, ref = GR.split(st0, case)
    name, n, m = case["name"], case["n"], case["m"]
    for k in LIST_KEYS:
        assert lists[k].shape == (n + 1,) and np.array_equal(lists[k], ref[k]), (name, k, lists[k][:8], ref[k][:8])
    for k in STATE_KEYS:
        assert np.array_equal(st[k], ref_st[k]), (name, k)
    for k in ("pool_root", "pool_dof", "progress", "reset", "terminate"):
        assert np.array_equal(st[k], st0[k]), (name, k, "was written")
    cnt = {k: int(lists[k][n]) for k in LIST_KEYS}
    got = np.concatenate([lists[k][:cnt[k]] for k in ("normal", "fall", "recover")])
    assert np.array_equal(np.sort(got), case["ids"][:m]), (name, "the three lists do not partition the input")
    slots = lists["fall_slot"][:cnt["fall"]]
    assert cnt["fall_slot"] == cnt["fall"] and len(set(slots.tolist())) == len(slots) and (slots >= 0).all() and (slots < P).all(), (name, "fall slots")
    held = st["assign"][st["assign"] >= 0]
    assert len(set(held.tolist())) == len(held) and (st["pool_taken"][held] == 1).all(), (name, "a slot is held twice or not marked")
    term = st0["terminate"][lists["recover"][:cnt["recover"]]]
    assert (term == 1).all(), (name, "an env that did not terminate became a recovery episode")
    if "want_fall" in case:
        assert cnt["fall"] == min(case["want_fall"], case["free"]), (name, "fall entries", cnt["fall"], case["want_fall"], case["free"])
        if case["free"] < case["want_fall"]:
            assert cnt["normal"] >= case["want_fall"] - case["free"], (name, "the surplus did not turn normal")
    return cnt


def flags_state():
    """E = 300: counters in {0, 1, 2, 60} x reset x terminate, every combination several times"""
    rng = np.random.default_rng(5)
    st = state(rng)
    i = np.arange(E)
    st["counter"] = np.array([0, 1, 2, 60], np.int32)[i % 4]
    st["reset"] = ((i // 4) % 2).astype(np.int64)
    st["terminate"] = ((i // 8) % 2).astype(np.int64)
    return st


def amp_case(ring, seed=9, n_env=64):
    rng = np.random.default_rng(seed)
    amp = rng.normal(size=(n_env, AMP_STEPS, AMP_ROW)).astype(np.float32)
    ids = np.concatenate([np.sort(rng.choice(n_env, 21, replace=False)), [-1, -1, -1]]).astype(np.int32)
    return amp, ids

"""NumPy restatement of the get-up entry points' integer logic (include/emloco_task.h: emloco_getup_split, emloco_getup_flags,
emloco_getup_amp_default and the pool copy of emloco_getup_apply), written from the header's text: plain loops over the list, no
prefix sums.  The keyed permutation and the device's random rows are the restatements tests/kernel_refs.py already holds."""
import numpy as np

import kernel_refs as R

AMP_STEPS = 15


def present(ids, n, n_env):
    """the list: the entries in front of the first id outside [0, n_env)"""
    m = 0
    while m < n and 0 <= ids[m] < n_env:
        m += 1
    return m


def uniforms(case, m):
    """[m][2] float32: the rows supplied, or the device's hash of (seed, entry, 0 | 1)"""
    if case["rnd"] is not None:
        return np.asarray(case["rnd"], np.float32).reshape(-1, 2)[:m]
    if m == 0:
        return np.zeros((0, 2), np.float32)
    return np.stack([R.reset_rnd_row(case["seed"], i, n=2).numpy() for i in range(m)]).astype(np.float32).reshape(m, 2)


def split(st, case):
    """the state after the call (a copy of `st` with pool_taken, assign, counter, stats advanced) and the four lists"""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    taken, assign, counter, term = st["pool_taken"], st["assign"], st["counter"], st["terminate"]
    E, P, n = len(assign), len(taken), case["n"]
    ids = case["ids"]
    m = present(ids, n, E)
    u = uniforms(case, m)
    rp, fp = np.float32(case["recovery_prob"]), np.float32(case["fall_prob"])
    for i in range(m):                                              # 1.
        e = ids[i]
        if assign[e] >= 0:
            taken[assign[e]] = 0
        assign[e] = -1
    free = [s for s in (R.real_pick_perm(k, P, case["key"]) for k in range(P)) if taken[s] == 0]
    normal, fall, recover, slots = [], [], [], []
    for i in range(m):
        e = int(ids[i])
        if u[i, 0] < rp and term[e] == 1:                           # 2.
            recover.append(e)
            counter[e] = case["steps"]
        elif u[i, 1] < fp and len(fall) < len(free):                # 3., 5.
            s = free[len(fall)]
            fall.append(e)
            slots.append(s)
            taken[s] = 1
            assign[e] = s
            counter[e] = case["steps"]
        else:                                                       # 4. (and the fall entries no slot is left for)
            normal.append(e)
            counter[e] = 0
    pad = lambda x: np.array(x + [-1] * (n - len(x)) + [len(x)], np.int32)
    if st.get("stats") is not None:
        st["stats"][0] += len(recover)
        st["stats"][1] += len(fall)
        st["stats"][2] += len(normal)
    return st, dict(normal=pad(normal), fall=pad(fall), recover=pad(recover), fall_slot=pad(slots))


def flags(st):
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    c = np.maximum(st["counter"] - 1, 0)
    st["counter"] = c.astype(np.int32)
    held = c > 0
    st["reset"][held] = 0
    st["terminate"][held] = 0
    st["progress"][held] -= 1
    if st.get("stats") is not None:
        st["stats"][3] += int(c.sum())
        st["stats"][4] += 1
        st["stats"][5] += int(held.sum())
    return st


def phys_row(ring, k):
    return (ring - 1 + k) % AMP_STEPS if ring else k                # EMLOCO_AMP_PHYS_ROW


def amp_default(amp, ring, ids):
    out = amp.copy()
    for e in ids:
        if e < 0:
            break
        for k in range(1, AMP_STEPS):
            out[e, phys_row(ring, k)] = amp[e, phys_row(ring, 0)]
    return out

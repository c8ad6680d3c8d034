"""The get-up kernels (emloco_amd/csrc/getup_kernels.hip) on the CPU emulator against tests/getup_ref.py: the cases of
tests/getup_cases.py, which tests/test_gpu_getup.py runs on the device.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_getup as EG                                                           # noqa: E402
import getup_cases as GC                                                         # noqa: E402
import getup_ref as GR                                                           # noqa: E402

CASES = GC.split_cases()


def _copy(st):
    return {k: v.copy() for k, v in st.items()}


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0]["name"] for c in CASES])
def test_split_equals_the_reference(index):
    case, st0 = CASES[index]
    st = _copy(st0)
    lists = EG.split(st, case)
    GC.judge_split(case, st0, st, lists)


def test_split_cases_cover_what_they_claim():
    """the table itself: every length, both kinds of list, every pair of probabilities; a short pool that really is short; lists in
    which listed envs and others hold slots; recovery candidates that did not terminate"""
    seen = {(c["m"], c["kind"], (c["recovery_prob"], c["fall_prob"])) for c, _ in CASES}
    for m in GC.LENGTHS:
        for kind in ("explicit", "compacted"):
            for probs in GC.PROBS:
                assert (m, kind, probs) in seen, (m, kind, probs)
    assert any(c.get("free", 0) < c.get("want_fall", 0) for c, _ in CASES) and any("want_fall" in c and c["free"] == c["want_fall"] > 0 for c, _ in CASES)
    case, st = CASES[GC.LENGTHS.index(261) * 10 + 4]
    listed = np.zeros(GC.E, bool)
    listed[case["ids"][:case["m"]]] = True
    assert (st["assign"][listed] >= 0).any() and (st["assign"][~listed] >= 0).any()
    assert (st["terminate"][listed] != 1).any() and (st["terminate"][listed] == 1).any()


def test_split_twice_keeps_the_pool_consistent():
    """two calls in a row on one state (the second list overlaps the first): slots given back and handed out again"""
    (c1, st0), (c2, _) = CASES[GC.LENGTHS.index(261) * 10 + 7], CASES[GC.LENGTHS.index(300) * 10 + 7]
    st = _copy(st0)
    EG.split(st, c1)
    mid = _copy(st)
    lists = EG.split(st, c2)
    GC.judge_split(c2, mid, st, lists)


def test_flags_equal_the_reference():
    st0 = GC.flags_state()
    st = _copy(st0)
    for _ in range(3):                                               # 60 -> 57, 2 -> 0, 1 -> 0: the counters cross zero on the way
        EG.flags(st)
        st0 = GR.flags(st0)
        for k in ("counter", "reset", "terminate", "progress", "stats"):
            assert np.array_equal(st[k], st0[k]), k
    assert st["stats"][4] == 4003 and (st["counter"] == np.array([0, 0, 0, 57])[np.arange(GC.E) % 4]).all()


@pytest.mark.parametrize("ring", [0, 1, 9, 15])
def test_amp_default_fills_the_history_with_the_newest_row(ring):
    amp0, ids = GC.amp_case(ring)
    amp = amp0.copy()
    EG.amp_default(amp, ring, ids)
    want = GR.amp_default(amp0, ring, ids)
    assert np.array_equal(amp.view(np.int32), want.view(np.int32))
    e = ids[0]
    assert all(np.array_equal(amp[e, k], amp0[e, GR.phys_row(ring, 0)]) for k in range(GC.AMP_STEPS))
    others = np.setdiff1d(np.arange(amp.shape[0]), ids[ids >= 0])
    assert np.array_equal(amp[others], amp0[others])


def test_pool_copy_writes_the_listed_rows_only():
    (case, st0) = CASES[GC.LENGTHS.index(261) * 10 + 2]              # probabilities (0, 1): every entry a fall entry
    st = _copy(st0)
    lists = EG.split(st, case)
    rng = np.random.default_rng(3)
    root0, dof0 = rng.normal(size=(GC.E, 13)).astype(np.float32), rng.normal(size=(GC.E, GC.NDOF, 2)).astype(np.float32)
    lam0 = rng.normal(size=(GC.E, GC.MAXCAND * 3)).astype(np.float32)
    root, dof, lam = root0.copy(), dof0.copy(), lam0.copy()
    EG.copy(st, root, dof, lam, lists["fall"], lists["fall_slot"])
    k = int(lists["fall"][-1])
    env, slot = lists["fall"][:k], lists["fall_slot"][:k]
    assert k > 200
    assert np.array_equal(root[env], st["pool_root"][slot]) and np.array_equal(dof[env], st["pool_dof"][slot]) and not lam[env].any()
    rest = np.setdiff1d(np.arange(GC.E), env)
    assert np.array_equal(root[rest], root0[rest]) and np.array_equal(dof[rest], dof0[rest]) and np.array_equal(lam[rest], lam0[rest])

"""Part plans of the rigid-body launch (emloco_sim_set_plan, csrc/sim_plan.h) shared by tests/test_sim_plan_cpu.py (emulator and host)
and tests/test_gpu_sim_plan.py (device): the plans under test, the word layout decoded in numpy and the plan's invariants written
down a second time, independently of the C++ checker."""
import numpy as np

N_SUB = 4
NAMES = ("root_state", "dof_state", "rb_state", "contact_force", "dof_force", "lambda_ws")


def plans(n_env, k=None):
    """name -> (classes, tail, shift): T = tail part; C = the last k ranks in two parts of two substeps; S = the last k ranks one stage
    behind (and, S-, ahead of) the others; T+C.  k defaults to a third of the envs, at least one -- so that with one env the light
    class is everything and the heavy class is empty."""
    k = max(1, n_env // 3) if k is None else k
    h = n_env - k
    return {
        "T": ([(0, n_env, 4)], 1, 0),
        "C": ([(0, h, 4), (h, n_env, 2)], 0, 0),
        "S": ([(0, h, 4), (h, n_env, 4)], 0, 1),
        "S-": ([(0, h, 4), (h, n_env, 4)], 0, -1),
        "T+C": ([(0, h, 4), (h, n_env, 2)], 1, 0),
    }


def flat(classes):
    return np.ascontiguousarray(np.asarray(classes, np.int32).reshape(-1, 3))


def decode(words):
    """the fields of plan words (csrc/sim_plan.h)"""
    w = np.asarray(words, np.uint32).astype(np.int64)
    return dict(rank=w & 0xFFFF, part=w >> 16 & 7, sub_lo=w >> 19 & 7, n_here=w >> 22 & 7, publishes=(w >> 25 & 1).astype(bool),
                consumes=(w >> 26 & 1).astype(bool), final=(w >> 27 & 1).astype(bool), rest=w >> 28)


def assert_invariants(words, n_env, n_sub, classes, tail):
    """exact cover in order, one final workgroup per rank behind its last substep, consumer index > producer index, at most four
    publishers per env -- and the class structure the parameters ask for"""
    f = decode(words)
    assert (f["rest"] == 0).all() and f["rank"].min() >= 0 and f["rank"].max() < n_env
    parts_of = np.zeros(n_env, np.int64)
    for lo, hi, parts in classes:
        parts_of[lo:hi] = parts
    assert len(words) == int((parts_of + tail).sum())
    for r in range(n_env):
        idx = np.nonzero(f["rank"] == r)[0]                                    # ascending workgroup index
        assert len(idx) == parts_of[r] + tail, r
        assert f["part"][idx].tolist() == list(range(len(idx))), r             # numbered in index order: producer index < consumer index
        lo, here = f["sub_lo"][idx], f["n_here"][idx]
        covered = [s for a, n in zip(lo, here) for s in range(a, a + n)]
        assert covered == list(range(n_sub)), (r, covered)                     # every substep exactly once, in order
        assert (lo[1:] == (lo + here)[:-1]).all() and lo[0] == 0
        assert f["final"][idx].sum() == 1 and f["final"][idx[-1]], r           # one final workgroup, the last: behind the last substep
        assert f["publishes"][idx].sum() <= 4 and (f["part"][idx][f["publishes"][idx]] <= 3).all(), r
        assert (f["publishes"][idx] == ~f["final"][idx]).all(), r              # whatever is not final hands its state on
        assert f["consumes"][idx].tolist() == [False] + [True] * (len(idx) - 1), r
        assert (here[:parts_of[r]] == n_sub // parts_of[r]).all(), r
        if tail:
            assert here[-1] == 0 and lo[-1] == n_sub, r

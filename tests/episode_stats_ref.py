"""numpy restatement of the game statistics (emloco_amd/csrc/episode_stats_kernels.hip, include/emloco_task.h): test infrastructure, not
part of the package.  The running values of a game are np.float32 added one step after the other, in step order, as the kernel adds them
(its translation unit is built without contraction, so the bits are the same); the epoch totals are float64.  Shared by
tests/test_episode_stats_cpu.py and tests/test_gpu_episode_stats.py, with the stub agent of the driver tests."""
import numpy as np

from emloco_amd.learning.episode_stats import MOMENT_NAMES, MOMENT_OPS, merge_moments, report_from_moments

F32 = np.float32
RUNS, TIMEOUT, FAR, FALLEN = 0, 1, 2, 3
K = {n: i for i, n in enumerate(MOMENT_NAMES)}


def d2_f32(tar_xy, root_xy):
    """(tx - rx)^2 + (ty - ry)^2 in float32, term by term as task_device.h:301-302"""
    dx = (tar_xy[:, 0].astype(F32) - root_xy[:, 0].astype(F32)).astype(F32)
    dy = (tar_xy[:, 1].astype(F32) - root_xy[:, 1].astype(F32)).astype(F32)
    return (dx * dx + dy * dy).astype(F32)


def speed2_f32(v):
    """(x x + y y) + z z in float32 for [..., 3]; a NaN counts as 0 (the step is counted as non-finite instead)"""
    v = v.astype(F32)
    with np.errstate(all="ignore"):
        s = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(F32) + v[..., 2] * v[..., 2]).astype(F32)
    return np.where(np.isnan(s), F32(0.0), s)


class EpisodeStatsRef:
    def __init__(self, n_env, fail_dist, inverted_penalty=None):
        self.E, self.fail_dist = n_env, F32(fail_dist)
        self.neg_scale = None if inverted_penalty is None else F32(-F32(inverted_penalty))
        self.running = np.zeros((n_env, 4), F32)                      # ret, loc, pow, len
        self.totals = np.zeros((n_env, len(MOMENT_NAMES)), np.float64)
        self.terms = [[] for _ in MOMENT_NAMES]                       # every term that went into a sum of the epoch (for the tolerance)

    def step(self, rew, raw, reset, term, d2, rb_state=None, inverted=None):
        """One env step.  Returns [E][5]: the finished games' ret / loc / pow / len (zeros elsewhere) and the cause."""
        E, tot = self.E, self.totals
        out = np.zeros((E, 5), F32)
        rew, raw, d2 = np.asarray(rew, F32), np.asarray(raw, F32), np.asarray(d2, F32)
        for e in range(E):
            r = rew[e]
            if self.neg_scale is not None and inverted is not None and inverted[e]:
                r = F32(r * self.neg_scale)
            run = self.running[e]
            ret, loc, pw, ln = F32(run[0] + r), F32(run[1] + raw[e, 0]), F32(run[2] + raw[e, 1]), F32(run[3] + F32(1.0))
            if rb_state is not None:
                st = np.asarray(rb_state[e], F32)
                tot[e, K["max_speed2"]] = max(tot[e, K["max_speed2"]], float(speed2_f32(st[:, 7:10]).max()))
                tot[e, K["max_ang_speed2"]] = max(tot[e, K["max_ang_speed2"]], float(speed2_f32(st[:, 10:13]).max()))
                if not np.isfinite(st).all():
                    tot[e, K["nonfinite_steps"]] += 1.0
                    self.terms[K["nonfinite_steps"]].append(1.0)
            done = reset[e] != 0
            if done:
                far = d2[e] > F32(self.fail_dist * self.fail_dist)
                cause = FAR if far else (FALLEN if term[e] != 0 else TIMEOUT)
                first = tot[e, K["games"]] == 0
                dl, dr = float(ln), float(ret)
                adds = {"games": 1.0, MOMENT_NAMES[cause]: 1.0, "sum_len": dl, "sum_len2": dl * dl, "sum_ret": dr, "sum_ret2": dr * dr,
                        "sum_loc": float(loc), "sum_pow": float(pw)}
                for name, x in adds.items():
                    tot[e, K[name]] += x
                    self.terms[K[name]].append(x)
                tot[e, K["min_len"]] = dl if first else min(tot[e, K["min_len"]], dl)
                tot[e, K["max_len"]] = max(tot[e, K["max_len"]], dl)
                out[e] = (ret, loc, pw, ln, cause)
                self.running[e] = 0.0
            else:
                self.running[e] = (ret, loc, pw, ln)
        return out

    def moments(self):
        """The epoch's moment vector over the envs (float64), the sum of |terms| per entry; the totals are cleared afterwards."""
        rows = [self.totals[e] for e in range(self.E)]
        m = merge_moments(*rows) if rows else np.zeros(len(MOMENT_NAMES))
        for k, op in enumerate(MOMENT_OPS):
            if op == "sum":
                m[k] = float(np.sum(self.totals[:, k], dtype=np.float64))
        scale = np.array([float(np.sum(np.abs(t))) for t in self.terms])
        self.totals[:] = 0.0
        self.terms = [[] for _ in MOMENT_NAMES]
        return m, scale

    def report(self):
        return report_from_moments(self.moments()[0])

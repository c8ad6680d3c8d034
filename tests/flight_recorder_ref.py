"""The flight recorder restated in numpy -- TEST INFRASTRUCTURE ONLY: record, cause bits, suppression, claim order and slot layout of
include/emloco_task.h (emloco_recorder_record / emloco_recorder_check), written from the header's text, not from the kernels.

A *state* is a dict of host arrays: root [E][13], dof [E][69][2], warm [E][288], drive [E][69], rb [E][24][13], cf [E][24][3],
df [E][69] (float32); progress, reset, terminate [E] (int64); request [E] (uint8) or None."""
import numpy as np

REC_WORDS, POST_WORDS, COUNTERS = 512, 892, 8
NONFINITE, SPEED, ANG_SPEED, EARLY_FALL, REQUEST = 1, 2, 4, 8, 16
NEVER = -(1 << 30)
FLOAT_KEYS = (("root", 13), ("dof", 138), ("warm", 288), ("drive", 69), ("rb", 312), ("cf", 72), ("df", 69))


def slot_words(R):
    return 4 + R * REC_WORDS + POST_WORDS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic_state(E, seed=0, request=True):
    """every float word distinct across all arrays and envs (a misplaced copy shows), finite"""
    st, base = {}, 1.0 + 65536.0 * seed
    for k, n in FLOAT_KEYS:
        st[k] = (base + np.arange(E * n, dtype=np.float64) * 0.25).astype(np.float32).reshape(E, n)
        base += E * n * 0.25 + 3.0
    st["dof"] = st["dof"].reshape(E, 69, 2)
    st["rb"] = st["rb"].reshape(E, 24, 13)
    st["cf"] = st["cf"].reshape(E, 24, 3)
    st["progress"] = (np.arange(E, dtype=np.int64) * 3 + 7 + seed)
    st["reset"] = np.zeros(E, np.int64)
    st["terminate"] = np.zeros(E, np.int64)
    st["request"] = np.zeros(E, np.uint8) if request else None
    return st


def quiet_state(E, seed=0):
    """a synthetic state whose body velocities are small (no speed cause at limits >= 1)"""
    st = synthetic_state(E, seed)
    st["rb"][:, :, 7:13] = 0.01
    return st


def record_words(st, env, t, drive_mode=0):
    w = np.zeros(REC_WORDS, np.uint32)
    w[0] = np.int32(st["progress"][env]).view(np.uint32)
    w[1] = np.int32(t).view(np.uint32)
    w[2] = drive_mode
    w[4:] = np.concatenate([bits(st[k][env]).ravel() for k in ("root", "dof", "warm", "drive")])
    return w


def post_words(st, env):
    return np.concatenate([bits(st[k][env]).ravel() for k in ("root", "dof", "warm", "rb", "cf", "df")])


def raw_causes(st, cause_mask, speed2, ang2, early_fall):
    """cause bits per env ahead of the suppression"""
    rb = st["rb"].astype(np.float32)
    with np.errstate(all="ignore"):
        v2 = (rb[:, :, 7] * rb[:, :, 7] + rb[:, :, 8] * rb[:, :, 8]) + rb[:, :, 9] * rb[:, :, 9]
        w2 = (rb[:, :, 10] * rb[:, :, 10] + rb[:, :, 11] * rb[:, :, 11]) + rb[:, :, 12] * rb[:, :, 12]
        assert v2.dtype == np.float32
        c = np.where(~np.isfinite(rb).all(axis=(1, 2)), NONFINITE, 0)
        c |= np.where((v2 > np.float32(speed2)).any(axis=1), SPEED, 0)
        c |= np.where((w2 > np.float32(ang2)).any(axis=1), ANG_SPEED, 0)
    c |= np.where((st["terminate"] != 0) & (st["progress"] < early_fall), EARLY_FALL, 0)
    if st.get("request") is not None:
        c |= np.where(st["request"] != 0, REQUEST, 0)
    return (c & cause_mask).astype(np.int32)


class RefRecorder:
    def __init__(self, E, R, C, cause_mask=31, speed2=0.0, ang2=0.0, early_fall=0, drive_mode=0):
        self.E, self.R, self.C = E, R, C
        self.cause_mask, self.speed2, self.ang2, self.early_fall, self.drive_mode = cause_mask, speed2, ang2, early_fall, drive_mode
        self.ring = np.zeros((E, R, REC_WORDS), np.uint32)
        self.slots = np.zeros((C, slot_words(R)), np.uint32)
        self.counters = np.zeros(COUNTERS, np.int32)
        self.last = np.full(E, NEVER, np.int32)
        self.t0 = None
        self.log = []                      # (env, t, cause) of every capture, in claim order

    def record(self, st, t):
        if self.t0 is None:
            self.t0 = t
        for e in range(self.E):
            self.ring[e, t % self.R] = record_words(st, e, t, self.drive_mode)

    def check(self, st, t):
        """-> the step's cause bits after the suppression; st["request"] is written as the device writes it"""
        c = raw_causes(st, self.cause_mask, self.speed2, self.ang2, self.early_fall)
        for e in np.nonzero(c)[0]:
            if t - int(self.last[e]) < self.R:
                if c[e] & REQUEST:
                    st["request"][e] = 0
                c[e] = 0
        n_valid = min(t - self.t0 + 1, self.R)
        for e in np.nonzero(c)[0]:                               # ascending env index
            used = int(self.counters[0])
            if used < self.C:
                s = self.slots[used]
                s[:4] = (e, np.int32(t).view(np.uint32), c[e], n_valid)
                s[4:4 + self.R * REC_WORDS] = 0
                for j in range(n_valid):
                    s[4 + j * REC_WORDS:4 + (j + 1) * REC_WORDS] = self.ring[e, (t - n_valid + 1 + j) % self.R]
                s[4 + self.R * REC_WORDS:] = post_words(st, e)
                self.counters[0] = used + 1
                self.last[e] = t
                if c[e] & REQUEST:
                    st["request"][e] = 0
                self.log.append((int(e), int(t), int(c[e])))
            else:
                for k in range(5):
                    if c[e] & (1 << k):
                        self.counters[1 + k] += 1
        return c

    def drain(self):
        k = int(self.counters[0])
        out = self.slots[:k].copy()
        self.counters[:] = 0
        return out

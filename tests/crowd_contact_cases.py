"""Cases of the crowd contact audit and a vectorised float64 restatement of include/emloco_task.h's definition WITHOUT any cull --
shared by tests/test_crowd_contacts_cpu.py (emulator) and tests/test_gpu_crowd_contacts.py (device).  TEST INFRASTRUCTURE ONLY.

Bounds against float64 (derived, not fitted): everything the narrow phase touches lies within L = 4 m of the env's own root (two
reaches of at most 1.2 m plus the culled root distance), and a penetration goes through about eight fp32 roundings of quantities no
larger than L, so |pen32 - pen64| <= 8 * 2^-24 * 4 = 1.9e-6 m; the root difference is one subtraction of exact inputs, so
|nearest32 - nearest64| <= 4 * 2^-24 * nearest.  Measured on the emulator and, the same bytes, on the device (fraction of the bound, worst env and step of
the case): spheres pen 0.000 / nearest 0.06, people 0.021 / 0.50, wide 0.033 / 0.33.  The float64 restatement was also held against an
op-by-op float32 numpy evaluation of the same arithmetic when the bound was derived (SMPL capsules, 540 pairs, near-parallel
segments included): worst differences of a few 1e-8 m, under 0.05 of the bound, and "contact or not" never differed.

The integer fields are compared exactly, so every generator asserts in float64 (`check_margins`): no segment pair's gap dist - rs
within 1e-5 m of zero, no root distance within 1e-5 m of near_dist, no two members within 1e-5 m (+ 1e-6 of the distance) of a tie for
the minimum distance or the maximum penetration -- except the envs a case names, placed on exactly representable, mirrored
coordinates to test the tie rule.  A step that misses a condition has the roots of the envs involved nudged and is checked again."""
import functools

import numpy as np

PEN_BOUND = 8 * 2.0 ** -24 * 4.0
NEAREST_RTOL = 4 * 2.0 ** -24
MARGIN = 1e-5


# ------------------------------------------------------------------------------------------------------------ float64 restatement
def _q2mat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _seg_seg_dist(p0, p1, q0, q1):
    """distance of the closest points of dev_math.h's seg_seg_closest (same branches, EPS 1e-12), broadcast over leading axes"""
    EPS = 1e-12
    dot = lambda u, v: (u * v).sum(-1)
    clip = lambda v: np.clip(v, 0.0, 1.0)
    d1, d2, r = p1 - p0, q1 - q0, p0 - q0
    a, e, f, c, b = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
    with np.errstate(all="ignore"):
        den = a * e - b * b
        s_gen = np.where(den > EPS, clip((b * f - c * e) / den), 0.0)
        t_gen = (b * s_gen + f) / e
        s_lo, s_hi = clip(-c / a), clip((b - c) / a)
        s_full = np.where(t_gen < 0, s_lo, np.where(t_gen > 1, s_hi, s_gen))
        s = np.where(a <= EPS, 0.0, np.where(e <= EPS, s_lo, s_full))
        t = np.where(a <= EPS, np.where(e <= EPS, 0.0, clip(f / e)), np.where(e <= EPS, 0.0, clip(t_gen)))
    dv = (p0 + d1 * s[..., None]) - (q0 + d2 * t[..., None])
    return np.sqrt(dot(dv, dv))


def place(rb, table):
    """(A, B [E][n][3], r [E][n], bound [E], finite [E], root [E][3]) in float64 from the float32 state and capsule table"""
    rb = np.asarray(rb, np.float32).astype(np.float64)
    sb = np.asarray(table["seg_body"]).astype(int)
    finite = np.isfinite(rb[:, :, :7]).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        R = _q2mat(rb[:, sb, 3:7])
        o = rb[:, sb, :3] - rb[:, :1, :3]
        A = o + np.einsum("enij,enj->eni", R, table["cap_a"].astype(np.float64))
        B = o + np.einsum("enij,enj->eni", R, table["cap_b"].astype(np.float64))
        r = table["cap_r"].astype(np.float64)
        bound = (np.maximum(np.linalg.norm(A, axis=-1), np.linalg.norm(B, axis=-1)) + r).max(axis=1)
    return A, B, r, bound, finite, rb[:, 0, :3]


def restate_now(rb, table, group_size, near_dist):
    """The header's definition, every pair of every two finite members of a group.  Returns (now, margins): `now` a dict of [E] arrays
    (float64 nearest / pen, integer fields), `margins` what check_margins looks at."""
    A, B, r, bound, finite, root = place(rb, table)
    E, n = r.shape
    now = dict(nearest=np.zeros(E), pen=np.zeros(E), nearest_member=np.full(E, -1), pen_member=np.full(E, -1), pen_segs=np.full(E, -1),
               n_pen=np.zeros(E, int), n_near=np.zeros(E, int), flags=(~finite).astype(int))
    gap_margin, near_margin = np.full(E, np.inf), np.full(E, np.inf)
    tie_nearest, tie_pen = np.full(E, np.inf), np.full(E, np.inf)
    for e in range(E):
        if not finite[e]:
            continue
        g0 = (e // group_size) * group_size
        ms = np.array([m for m in range(g0, g0 + group_size) if m != e and finite[m]], int)
        if len(ms) == 0:
            continue
        s = root[ms] - root[e]
        d_xy = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1])
        Q0, Q1 = A[ms] + s[:, None, :], B[ms] + s[:, None, :]
        dist = _seg_seg_dist(A[e][None, :, None, :], B[e][None, :, None, :], Q0[:, None, :, :], Q1[:, None, :, :])      # [M][i][j]
        gap = dist - (r[e][None, :, None] + r[ms][:, None, :])
        pen_ij = np.where(gap < 0, -gap, 0.0)
        pen_m = pen_ij.max(axis=(1, 2))
        k = int(np.argmin(d_xy))                                 # (the first of equals: the lowest member)
        now["nearest"][e], now["nearest_member"][e] = d_xy[k], ms[k]
        now["n_near"][e] = int((d_xy < near_dist).sum())
        now["n_pen"][e] = int((pen_m > 0).sum())
        if pen_m.max() > 0:
            flat = int(np.argmax(pen_ij))                        # C order over (m, i, j), members ascending: the lexicographically lowest
            mi, i, j = np.unravel_index(flat, pen_ij.shape)
            now["pen"][e], now["pen_member"][e], now["pen_segs"][e] = pen_ij[mi, i, j], ms[mi], int(i) | (int(j) << 8)
        gap_margin[e] = np.abs(gap).min()
        near_margin[e] = np.abs(d_xy - near_dist).min()
        if len(ms) > 1:
            d2 = np.sort(d_xy)
            tie_nearest[e] = (d2[1] - d2[0]) - 1e-6 * d2[0]
            p2 = np.sort(pen_m)[::-1]
            if p2[0] > 0:
                tie_pen[e] = p2[0] - p2[1]
    return now, dict(gap=gap_margin, near=near_margin, tie_nearest=tie_nearest, tie_pen=tie_pen)


def bad_envs(margins, ties_allowed=()):
    """the envs that miss a condition of the module's docstring"""
    bad = (margins["gap"] < MARGIN) | (margins["near"] < MARGIN)
    tie = (margins["tie_nearest"] < MARGIN) | (margins["tie_pen"] < MARGIN)
    tie[list(ties_allowed)] = False
    return np.nonzero(bad | tie)[0]


def settle(rb, table, group_size, near_dist, rng, ties_allowed=(), fixed=()):
    """nudges the roots (all bodies) of the envs that miss a condition by up to 1 cm until none does; returns (rb, now)"""
    for _ in range(50):
        now, margins = restate_now(rb, table, group_size, near_dist)
        bad = [e for e in bad_envs(margins, ties_allowed) if e not in fixed]
        if len(bad_envs(margins, ties_allowed)) == 0:
            return rb, now
        assert bad, "a placed env misses the case conditions"
        for e in bad:
            rb[e, :, :2] += np.float32(rng.uniform(-0.01, 0.01, 2))
    raise AssertionError("the case does not settle")


# ------------------------------------------------------------------------------------------------------------ bookkeeping in numpy
def restate_books(now_seq, done_seq, slot_seq, games_per_env, n_totals=13):
    """(records [E][G] as a dict of arrays, written [E][G] bool, totals [E][n_totals]) of emloco_crowd_contacts_accumulate over the
    steps, from the now[] the kernels themselves gave (NOW_DTYPE arrays): integer logic, float32 min / max, double sums in step order."""
    from emu_crowd_contacts import RECORD_DTYPE
    E = len(now_seq[0])
    G = max(games_per_env, 1)
    rec = np.zeros((E, G), RECORD_DTYPE)
    written = np.zeros((E, G), bool)
    tot = np.zeros((E, n_totals))
    zero = lambda: dict(sum=0.0, mn=np.float32(0), mx=np.float32(0), calls=0, steps=0, nonf=0, neigh=0, near=0, cs=0, c=0, pm=0, ps=0, pstep=0, first=0)
    game = [zero() for _ in range(E)]
    for now, done, slot in zip(now_seq, done_seq, slot_seq):
        for e in range(E):
            g, n = game[e], now[e]
            finite = (n["flags"] & 1) == 0
            neigh = finite and n["nearest_member"] >= 0
            g["calls"] += 1
            g["steps" if finite else "nonf"] += 1
            tot[e, 0 if finite else 1] += 1
            if neigh:
                g["sum"] += float(n["nearest"])
                g["mn"] = n["nearest"] if g["neigh"] == 0 or n["nearest"] < g["mn"] else g["mn"]
                tot[e, 8] = float(n["nearest"]) if tot[e, 12] == 0 or float(n["nearest"]) < tot[e, 8] else tot[e, 8]
                g["neigh"] += 1
                tot[e, 12] += 1
                tot[e, 5] += float(n["nearest"])
                tot[e, 6] += float(n["pen"])
                tot[e, 7] = max(tot[e, 7], float(n["pen"]))
                if n["n_near"] > 0:
                    g["near"] += 1
                    tot[e, 4] += 1
                if n["n_pen"] > 0:
                    g["cs"] += 1
                    g["c"] += int(n["n_pen"])
                    tot[e, 2] += 1
                    tot[e, 3] += int(n["n_pen"])
                    if g["first"] == 0:
                        g["first"] = g["calls"]
                    if n["pen"] > g["mx"]:
                        g["mx"], g["pm"], g["ps"], g["pstep"] = n["pen"], int(n["pen_member"]), int(n["pen_segs"]), g["calls"]
            if done[e]:
                tot[e, 9] += 1
                tot[e, 10] += g["cs"] > 0
                tot[e, 11] += g["first"] == 1
                if games_per_env > 0 and 0 <= slot[e] < games_per_env:
                    touch = g["mx"] > 0
                    rec[e, slot[e]] = (g["mn"] if g["neigh"] else -1.0, np.float32(g["sum"] / g["neigh"]) if g["neigh"] else 0.0, g["mx"],
                                       g["steps"], g["nonf"], g["near"], g["cs"], g["c"], g["pm"] if touch else -1, g["ps"] if touch else -1,
                                       g["pstep"] if touch else -1, g["first"] if g["first"] else -1)
                    written[e, slot[e]] = True
                game[e] = zero()
    return rec, written, tot


def restate_moments(rec, games):
    """emloco_crowd_contacts_reduce in numpy (float64 sums; the order differs from the kernel's tree: rtol 1e-12)"""
    m = np.zeros(13)
    for e in range(rec.shape[0]):
        for r in rec[e, :games[e]]:
            m[0] += 1
            m[3] += r["steps"]; m[4] += r["contact_steps"]; m[5] += r["near_steps"]; m[6] += r["contacts"]; m[7] += r["nonfinite_steps"]
            if r["contact_steps"] > 0:
                m[1] += 1
                m[2] += r["first_contact_step"] == 1
                m[8] += float(r["max_pen"]); m[9] += float(r["max_pen"]) ** 2
            if r["min_nearest"] >= 0:
                m[12] += 1
                m[10] += float(r["min_nearest"]); m[11] += float(r["mean_nearest"])
    return m


def restate_epoch(tot):
    out = tot.sum(axis=0)
    out[7] = tot[:, 7].max()
    met = tot[:, 12] > 0
    out[8] = tot[met, 8].min() if met.any() else 0.0
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
def _identity_state(n_env):
    rb = np.zeros((n_env, 24, 13), np.float32)
    rb[:, :, 6] = 1
    return rb


@functools.lru_cache(maxsize=None)
def spheres():
    """E = 12 in groups of 4, n_seg = 24: every capsule a sphere of radius 0.1 at its body's origin, body b 0.0625 b above the root,
    identity quaternions, every coordinate a multiple of 2^-4 -- the answers are known by hand (test_*_spheres_by_hand)."""
    E, gs = 12, 4
    table = dict(cap_a=np.zeros((E, 24, 3), np.float32), cap_b=np.zeros((E, 24, 3), np.float32), cap_r=np.full((E, 24), 0.1, np.float32),
                 seg_body=np.arange(24, dtype=np.uint8))
    rb = _identity_state(E)
    xy = {0: (0, 0), 1: (0.125, 0), 2: (-0.125, 0), 3: (10, 0),            # 1 and 2 mirrored about 0: env 0 ties, the lowest index wins
          4: (10, 0), 5: (10.25, 0.5), 6: (9.5, -0.5), 7: (10.5, 0.25),    # 4 on env 3's spot, in another group; 5: NaN, 6: Inf
          8: (-20, 5), 9: (-20, 5.125), 10: (-20.125, 5), 11: (-19.875, 5)}     # 9 .. 11 non-finite: env 8 has nobody
    for e, (x, y) in xy.items():
        rb[e, :, 0], rb[e, :, 1] = x, y
        rb[e, :, 2] = 1.0 + 0.0625 * np.arange(24)
    rb[5, 7, 0] = np.nan
    rb[6, 3, 6] = np.inf
    rb[9, 0, 2] = -np.inf
    rb[10, 23, 3] = np.nan
    rb[11, 0, 0] = np.nan
    rb[:, :, 7:] = 0.5                                       # velocities are not read
    now, margins = restate_now(rb, table, gs, 1.0)
    assert len(bad_envs(margins, ties_allowed=(0,))) == 0
    return dict(name="spheres", E=E, gs=gs, near_dist=1.0, table=table, rb=rb[None], now=[now])


def _people_table(n_env):
    from emloco_amd.model import pack_self_collision, smpl_humanoid
    base = smpl_humanoid()
    models = [base.scaled(0.92, 0.9) if e % 2 else base.scaled(1.06, 1.1) for e in range(n_env)]
    pw = []
    for m in models:
        p = np.zeros((24, 3))
        for i in range(1, 24):
            p[i] = p[m.parent[i]] + m.joint_off[i]
        pw.append(p)
    sc = pack_self_collision(models)
    return {k: sc[k] for k in ("cap_a", "cap_b", "cap_r", "seg_body")}, np.asarray(pw)


def _posed(rng, pw, roots):
    """bodies at their bind-pose offsets from the root, every body with a random rotation of its own (not normalised in float32)"""
    E = len(roots)
    rb = np.zeros((E, 24, 13), np.float32)
    rb[:, :, :3] = roots[:, None, :] + pw
    q = rng.normal(size=(E, 24, 4))
    rb[:, :, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True) * rng.uniform(0.999, 1.001, (E, 24, 1))
    rb[:, :, 7:] = rng.normal(size=(E, 24, 6))
    return rb


@functools.lru_cache(maxsize=None)
def people():
    """E = 12 in groups of 4, the real table of pack_self_collision for two scaled SMPL models alternating (26 segments), random body
    rotations, root distances 0.05 .. 3 m, T = 40 steps with scripted game ends (games_per_env = 3):
      env 0, 1   0.12 m apart at every step: their games start in contact;  env 1 ends five games: it plays on after its quota
      env 2      ends games at steps 0 and 1: a game that ends at its first step
      env 3      at least 3.1 m from everybody: never touches; one game end, slots 1 and 2 stay zero bytes
      every env  a game still running at the end
      env 6      NaN at steps 10 .. 12 (non-finite steps inside a game)"""
    E, gs, T, G = 12, 4, 40, 3
    rng = np.random.default_rng(7)
    table, pw = _people_table(E)
    centres = np.array([[30.0 * (e // gs), -12.0 * (e // gs), 0.95] for e in range(E)])
    rbs, nows = [], []
    for t in range(T):
        roots = centres.copy()
        ang, rad = rng.uniform(0, 2 * np.pi, E), rng.uniform(0.05, 1.5, E)
        roots[:, 0] += rad * np.cos(ang); roots[:, 1] += rad * np.sin(ang)
        roots[:, 2] += rng.uniform(-0.1, 0.1, E)
        roots[1] = roots[0] + [0.12, 0.0, 0.0]
        roots[3, :2] = centres[3, :2] + [4.8, 0.0]
        rb = _posed(rng, pw, roots)
        if 10 <= t <= 12:
            rb[6, 4, 1] = np.nan
        rb, now = settle(rb, table, gs, 1.0, rng)
        assert now["n_pen"][0] > 0 and now["n_pen"][1] > 0 and now["n_pen"][3] == 0 and now["nearest"][3] > 3.1
        rbs.append(rb); nows.append(now)
    done = np.zeros((T, E), np.uint8)
    done[[3, 9, 17, 25, 33], 1] = 1
    done[[0, 1, 30], 2] = 1
    done[20, 3] = 1
    done[[11, 28], 6] = 1
    for e in (0, 4, 5, 7, 8, 9, 10, 11):
        done[5 + 3 * e, e] = 1
        done[36, e] = e % 2
    slot = np.zeros((T, E), np.int32)
    for t in range(1, T):
        slot[t] = slot[t - 1] + done[t - 1]
    return dict(name="people", E=E, gs=gs, near_dist=1.0, table=table, rb=np.stack(rbs), now=nows, done=done, slot=slot, G=G,
                games=np.minimum(slot[-1] + done[-1], G).astype(np.int32))


@functools.lru_cache(maxsize=None)
def wide():
    """E = 140 in groups of 70 (no multiple of 64: members on either side of a wave's first 64), three steps of geometry, the roots in
    clusters spread over +-170 m.  Members 0 / 65, 1 / 69 and 63 / 64 of each group stand 5 mm inside, 5 mm outside and 0.5 mm inside
    bound_e + bound_m: the member cull changes nothing against this un-culled restatement."""
    E, gs, T = 140, 70, 3
    rng = np.random.default_rng(11)
    table, pw = _people_table(E)
    rbs, nows = [], []
    for t in range(T):
        n_clusters = 10
        cl = rng.uniform(-170, 170, (E // gs, n_clusters, 2))
        roots = np.zeros((E, 3))
        for e in range(E):
            ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 1.5)
            roots[e, :2] = cl[e // gs, rng.integers(n_clusters)] + rad * np.array([np.cos(ang), np.sin(ang)])
            roots[e, 2] = 0.95 + rng.uniform(-0.1, 0.1)
        rb = _posed(rng, pw, roots)
        bound = place(rb, table)[3]
        fixed = []
        for g in range(E // gs):
            for k, (a, b, off) in enumerate(((0, 65, -0.005), (1, 69, 0.005), (63, 64, -0.0005))):
                a, b = g * gs + a, g * gs + b
                spot = np.array([150.0 - 40 * k, -160.0 + 300 * g, 0.95])       # away from the clusters' members only by chance: settle() checks
                u = rng.normal(size=3); u[2] *= 0.2; u /= np.linalg.norm(u)
                for e, at in ((a, spot), (b, spot + u * (bound[a] + bound[b] + off))):
                    rb[e, :, :3] = np.float32(rb[e, :, :3].astype(np.float64) - rb[e, 0, :3].astype(np.float64) + at)
                fixed += [a, b]
        rb, now = settle(rb, table, gs, 1.0, rng, fixed=tuple(fixed))
        A, B, r, bound, finite, root = place(rb, table)
        for g in range(E // gs):                               # the three pairs are where they were put
            for a, b, off in ((0, 65, -0.005), (1, 69, 0.005), (63, 64, -0.0005)):
                d = np.linalg.norm(root[g * gs + b] - root[g * gs + a]) - (bound[g * gs + a] + bound[g * gs + b])
                assert abs(d - off) < 2e-4, (a, b, d, off)
        rbs.append(rb); nows.append(now)
    return dict(name="wide", E=E, gs=gs, near_dist=1.0, table=table, rb=np.stack(rbs), now=nows)


CASES = {"spheres": spheres, "people": people, "wide": wide}


# ------------------------------------------------------------------------------------------------------------ comparisons
def check_now(got, want, label=""):
    """`got` (NOW_DTYPE) against the restatement: floats within the bounds, integers exact; returns the fractions of the bounds used"""
    for k in ("nearest_member", "pen_member", "pen_segs", "n_pen", "n_near", "flags"):
        assert np.array_equal(got[k], want[k]), (label, k, np.nonzero(got[k] != want[k])[0][:8], got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])
    pen_err = np.abs(got["pen"].astype(np.float64) - want["pen"])
    near_err = np.abs(got["nearest"].astype(np.float64) - want["nearest"])
    near_bound = NEAREST_RTOL * want["nearest"]
    with np.errstate(all="ignore"):
        frac = pen_err.max() / PEN_BOUND, float(np.nanmax(np.where(near_bound > 0, near_err / near_bound, 0.0)))
    print(f"{label}: pen error {pen_err.max():.3g} m = {frac[0]:.3f} of the bound, nearest error {frac[1]:.3f} of the bound")
    assert (pen_err <= PEN_BOUND).all() and (near_err <= near_bound).all(), (label, frac)
    return frac

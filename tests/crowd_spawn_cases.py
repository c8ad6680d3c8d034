"""The crowd spawn's rule (include/emloco_task.h: EmlocoCrowdSpawn) restated in numpy float32, and the cases both test files run --
TEST INFRASTRUCTURE ONLY.  Every operation of the rule is exact or correctly rounded in fp32 (a multiply, an add, a subtract, a divide,
a truncation, comparisons), and numpy's float32 scalars and arrays round each of them once, as the kernel built without contraction
does: the tests hold positions, clearance2, tried, flags and order bit for bit.

A case is a dict: the scalars of the structure, `walkable` [rows][cols] int16, `centres` [G][2], `roots` [E][stride] float32, `ids`
(None or a list) and `u` [n][tries][2] float32."""
import numpy as np

f32 = np.float32
CROWDED, NO_GROUND = 1, 2
INF = f32(np.inf)
INFO = np.dtype([("clearance2", np.float32), ("tried", np.int32), ("flags", np.int32), ("order", np.int32)])


def positions(case):
    """{env: its lowest list position}"""
    E = case["n_env"]
    if case["ids"] is None:
        return {e: e for e in range(E)}
    pos = {}
    for i, e in enumerate(case["ids"]):
        if 0 <= e < E:
            pos.setdefault(int(e), i)
    return pos


def admissible(case, cx, cy):
    if not (case["min_x"] <= cx <= case["max_x"] and case["min_y"] <= cy <= case["max_y"]):
        return False
    h = f32(case["hscale"])
    qx, qy = cx / h, cy / h
    rows, cols = case["walkable"].shape
    if not (qx > -1 and qx < rows and qy > -1 and qy < cols):
        return False
    return case["walkable"][int(np.trunc(qx)), int(np.trunc(qy))] == 0


def clearance2(x, y, stands, cx, cy):
    if not stands.any():
        return INF
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = x[stands] - cx, y[stands] - cy
        return ((dx * dx) + (dy * dy)).min()


def spawn_f32(case, roots=None, ids="case", u=None):
    """(place_xy {env: (x, y)}, info {env: (clearance2, tried, flags, order)}) of the listed envs"""
    case = dict(case)
    if roots is not None:
        case["roots"] = roots
    if ids != "case":
        case["ids"] = ids
    if u is not None:
        case["u"] = u
    gs, K = case["group_size"], case["tries"]
    roots, u = np.asarray(case["roots"], f32), np.asarray(case["u"], f32)
    centres = np.asarray(case["centres"], f32)
    extent, md = f32(case["extent"]), f32(case["min_dist"])
    md2 = md * md
    pos = positions(case)
    place, info = {}, {}
    for g in sorted({e // gs for e in pos}):
        g0 = g * gs
        x, y = roots[g0:g0 + gs, 0].copy(), roots[g0:g0 + gs, 1].copy()
        members = sorted(e for e in pos if e // gs == g)
        stands = np.isfinite(x) & np.isfinite(y)
        stands[[e - g0 for e in members]] = False
        cgx, cgy = centres[g]
        for order, e in enumerate(members):
            cand = []
            for k in range(K):
                ux, uy = u[pos[e], k]
                tx, ty = f32(2) * ux - f32(1), f32(2) * uy - f32(1)
                cx, cy = cgx + extent * tx, cgy + extent * ty
                cand.append((admissible(case, cx, cy), clearance2(x, y, stands, cx, cy), cx, cy))
            ok = [k for k in range(K) if cand[k][0]]
            good = [k for k in ok if cand[k][1] >= md2]
            flags = 0
            if good:
                k = good[0]
            elif ok:
                k = max(ok, key=lambda k: (cand[k][1], -k))
                flags = CROWDED
            else:
                k = -1
            if k >= 0:
                _, c2, px, py = cand[k]
            else:
                px, py = cgx, cgy
                c2 = clearance2(x, y, stands, cgx, cgy)
                flags = NO_GROUND | (CROWDED if c2 < md2 else 0)
            place[e], info[e] = (f32(px), f32(py)), (f32(c2), k, flags, order)
            x[e - g0], y[e - g0] = px, py
            stands[e - g0] = bool(np.isfinite(px) and np.isfinite(py))
    return place, info


def expected_arrays(case, place_prefill, info_prefill, **kw):
    """the output buffers after the call: the prefill with the listed envs' rows replaced"""
    place, info = spawn_f32(case, **kw)
    xy, inf = place_prefill.copy(), info_prefill.copy()
    for e in place:
        xy[e] = place[e]
        inf[e] = info[e]
    return xy, inf


# ---------------------------------------------------------------------------------------------- the cases
def base(n_env, group_size, tries, extent, min_dist=1.0, rows=400, cols=400, hscale=0.1, centre=(20.0, 20.0), stride=13):
    G = n_env // group_size
    return dict(n_env=n_env, group_size=group_size, tries=tries, root_stride=stride, hscale=hscale, min_x=f32(0.0), max_x=f32(rows * hscale - 1),
                min_y=f32(0.0), max_y=f32(cols * hscale - 1), extent=f32(extent), min_dist=f32(min_dist),
                walkable=np.zeros((rows, cols), np.int16), centres=np.tile(np.asarray(centre, f32), (G, 1)),
                roots=np.tile(np.asarray(list(centre) + [0.9] + [0.0] * (stride - 3), f32), (n_env, 1)), ids=None, u=None)


def uniforms(rng, n, tries):
    return rng.random((n, tries, 2), dtype=np.float32)


def case_small_extent():
    """1: two groups of 6, tries 1, full reset, extent 1.5 m: crowded fallbacks occur (seed chosen so that both groups have one)"""
    c = base(12, 6, 1, 1.5)
    c["u"] = uniforms(np.random.default_rng(4), 12, 1)
    return c


def case_padded_list():
    """2: groups of 70 (no multiple of 64), 140 envs, tries 8; unsorted list with -1 padding and env 75 twice; live members inside the
    square; group 0 has no listed member"""
    c = base(140, 70, 8, 6.0, stride=7)
    rng = np.random.default_rng(21)
    c["roots"][:, :2] = 20.0 + rng.uniform(-6, 6, (140, 2)).astype(f32)
    c["ids"] = [139, -1, 75, 71, -1, 120, 75, 70, 101, -1, -1, 88]
    c["u"] = uniforms(rng, len(c["ids"]), 8)
    return c


def case_same_call():
    """3: envs 2 and 5 of one group with identical uniform rows: the second sees the first at its new spot"""
    c = base(8, 8, 4, 5.0)
    rng = np.random.default_rng(31)
    c["roots"][:, :2] = 20.0 + rng.uniform(-5, 5, (8, 2)).astype(f32)
    c["ids"] = [5, 2]
    row = uniforms(rng, 1, 4)
    c["u"] = np.concatenate([row, row])
    return c


def case_threshold():
    """4: candidate 0 of env 0 is (20, 20) + 8 * (0.25, -0.5) = (22, 16); member 1 stands at (22 + 0.75, 16 + 1.0): with min_dist
    1.25 the offset is the 3-4-5 triangle scaled by 1/4 and 0.5625 + 1.0 = 1.5625 = 1.25^2, every step exact in fp32"""
    c = base(4, 4, 2, 8.0, min_dist=1.25)
    c["roots"][:, :2] = [[20, 20], [22.75, 17.0], [35, 35], [35, 36]]
    c["ids"] = [0]
    c["u"] = np.asarray([[[0.625, 0.25], [0.9, 0.9]]], f32)
    return c


def case_fallback_tie():
    """5: both candidates of env 0 are 0.5 m from member 1 at (20, 20), on either side: equal clearance2 0.25, the lower k wins"""
    c = base(4, 4, 2, 8.0)
    c["roots"][:, :2] = [[30, 30], [20, 20], [35, 35], [35, 36]]
    c["ids"] = [0]
    c["u"] = np.asarray([[[0.53125, 0.5], [0.46875, 0.5]]], f32)       # t = +-0.0625, c = 20 +- 0.5
    return c


def case_ground():
    """6: blocked cells, a box that cuts the square, a field smaller than the box.  Centres (20, 20) and (38, 20), extent 8; the box
    starts at y = 16 (the squares start at 12) and ends at x = 45, the field has 400 rows (40 m); rows 220 .. 239 and row 278 are
    blocked.  Env 1's four candidates: x = 22.4 and 23.2 (blocked rows), (16.8, 13.6) (outside the box), x = 27.84 (row 278): none
    admissible.  Env 4's candidate 0 is x = 41.2: inside the box, cell row 412 outside the field."""
    c = base(8, 4, 4, 8.0, rows=400, cols=400)
    c["min_y"], c["max_x"] = f32(16.0), f32(45.0)
    c["centres"] = np.asarray([[20, 20], [38, 20]], f32)
    c["walkable"][220:240, :] = 1
    c["walkable"][278, :] = 1
    rng = np.random.default_rng(61)
    c["roots"][:4, :2] = 20.0 + rng.uniform(-8, 8, (4, 2)).astype(f32)
    c["roots"][4:, :2] = [38, 20] + rng.uniform(-1.5, 1.5, (4, 2)).astype(f32)
    c["ids"] = [0, 1, 2, 4, 5]
    u = uniforms(rng, 5, 4)
    u[1, :, 0] = [0.65, 0.7, 0.3, 0.99]
    u[1, :, 1] = [0.5, 0.6, 0.1, 0.5]
    u[3, 0] = [0.7, 0.5]
    c["u"] = u
    return c


def case_non_finite():
    """7: NaN and inf roots among the live members; group 1: every member but env 4 is listed, and env 4's root is NaN, so the first
    placed (env 5) has nobody standing: clearance2 +inf, candidate 0"""
    c = base(8, 4, 3, 4.0)
    rng = np.random.default_rng(71)
    c["roots"][:, :2] = 20.0 + rng.uniform(-4, 4, (8, 2)).astype(f32)
    c["roots"][1, 0], c["roots"][2, 1], c["roots"][4, 0] = np.nan, np.inf, np.nan
    c["ids"] = [0, 3, 7, 6, 5]
    c["u"] = uniforms(rng, 5, 3)
    return c


def auto_extent(group_size, min_dist):
    return 0.5 * float(np.sqrt(group_size * min_dist * min_dist / 0.2))


def case_shipped():
    """8: one group of 512, tries 8, auto extent (25.3 m), full reset; the seed is chosen so that the restatement flags at most one
    placement crowded"""
    c = base(512, 512, 8, auto_extent(512, 1.0), rows=1200, cols=1200, centre=(60.0, 60.0))
    c["u"] = uniforms(np.random.default_rng(8), 512, 8)
    return c


CASES = {"small_extent": case_small_extent, "padded_list": case_padded_list, "same_call": case_same_call, "threshold": case_threshold,
         "fallback_tie": case_fallback_tie, "ground": case_ground, "non_finite": case_non_finite, "shipped": case_shipped}

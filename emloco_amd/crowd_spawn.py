"""Python side of the crowd spawn (include/emloco_task.h: EmlocoCrowdSpawn, emloco_task_crowd_spawn).

With `group_spawn: True` and `divide_group: True` a reset puts every member of a group on a random admissible spot of the group's
square, at least `group_spawn_min_dist` from every member of the group standing at that moment, instead of on the one fixed spot.
The keys are this project's: the reference's placement for groups (Terrain.sample_valid_locations(..., sample_groups=True),
humanoid_pedestrain_terrain.py:1196-1204) is never called there and checks neither clearance nor walkability.  The rule is stated in
the header, word for word.

`CrowdSpawn` owns what the kernels need beyond the task's root states: the mark workspace, `place_xy`, `info`, the centres and the
walkable field as int16.  The uniforms are drawn with torch.rand on the device; the kernels run on torch's current stream.
"""
import ctypes as C
import math

import torch

from . import _lib as L

DEFAULTS = dict(group_spawn=False, group_spawn_min_dist=1.0, group_spawn_tries=8, group_spawn_extent="auto", group_spawn_centre=None,
                group_spawn_margin=10.0)
DENSITY = 0.2               # members per min_dist^2 of the square at the "auto" extent


class CrowdSpawnError(L.EmlocoError):
    pass


def config_block(env_cfg):
    """The crowd spawn's settings of cfg["env"], defaults filled in: dict(on, min_dist, tries, extent, centre, margin).  `extent` stays
    "auto" and `centre` None (the field's midpoint) until the group size and the field are known (`resolve`)."""
    get = lambda k: env_cfg.get(k, DEFAULTS[k])
    return dict(on=bool(get("group_spawn")), min_dist=get("group_spawn_min_dist"), tries=get("group_spawn_tries"),
                extent=get("group_spawn_extent"), centre=get("group_spawn_centre"), margin=get("group_spawn_margin"))


def auto_extent(group_size, min_dist):
    """Half the side of the square that holds DENSITY members per min_dist^2: 25.3 m at 512 members and 1 m, 4.5 m at 16.  (A numpy
    prototype of the rule at 512 members, 8 tries and this extent gave 0 or 1 crowded placement per full reset over 20 seeds; the
    reference's +-8 m gives about 380 of 512.)"""
    return 0.5 * math.sqrt(group_size * float(min_dist) ** 2 / DENSITY)


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def resolve(block, group_size, field_x, field_y):
    """`block` with the extent and the centre as numbers: "auto" by `auto_extent`, None as the midpoint of the field_x x field_y [m] field"""
    out = dict(block)
    if out["extent"] == "auto" and _number(out["min_dist"]):
        out["extent"] = auto_extent(group_size, out["min_dist"])
    if out["centre"] is None:
        out["centre"] = (0.5 * field_x, 0.5 * field_y)
    return out


def spawn_refusal(env_cfg, group_size=None, field=None, walkable=None, hscale=None):
    """Why cfg["env"] cannot run the crowd spawn, as a sentence that names the key, or None.  With `field` = (x, y) [m], the size of the
    height field, the square is held against it; with `walkable` ([rows][cols], 0: walkable) and `hscale` the centre's cell as well."""
    b = config_block(env_cfg)
    if not b["on"]:
        return None
    if not env_cfg.get("divide_group", False):
        return ("group_spawn: the crowd spawn places the members of a group apart and needs divide_group: True (with num_env_group); "
                "this configuration has no groups")
    if not (_number(b["min_dist"]) and b["min_dist"] >= 0):
        return f"group_spawn_min_dist: {b['min_dist']!r} is not a finite length >= 0 [m]"
    if not (isinstance(b["tries"], int) and not isinstance(b["tries"], bool) and 1 <= b["tries"] <= L.SPAWN_MAX_TRIES):
        return f"group_spawn_tries: {b['tries']!r} is not an integer in 1 .. {L.SPAWN_MAX_TRIES}"
    if b["extent"] != "auto" and not (_number(b["extent"]) and b["extent"] > 0):
        return f"group_spawn_extent: {b['extent']!r} is neither \"auto\" nor a finite positive length [m]"
    if not (_number(b["margin"]) and b["margin"] >= 0):
        return f"group_spawn_margin: {b['margin']!r} is not a finite length >= 0 [m]"
    c = b["centre"]
    if c is not None and not (isinstance(c, (list, tuple)) and len(c) == 2 and all(_number(v) for v in c)):
        return f"group_spawn_centre: {c!r} is not a pair of finite coordinates [m]"
    if group_size is not None and group_size > L.SPAWN_MAX_GROUP:
        return f"group_spawn: num_env_group gives groups of {group_size}; the crowd spawn stages a group on chip and takes at most {L.SPAWN_MAX_GROUP}"
    if group_size is None or field is None:
        return None
    r = resolve(b, group_size, *field)
    (cx, cy), ext, m = r["centre"], r["extent"], r["margin"]
    if cx - ext < m or cx + ext > field[0] - m or cy - ext < m or cy + ext > field[1] - m:
        return (f"group_spawn_extent: the square of +-{ext:.1f} m about group_spawn_centre ({cx:.1f}, {cy:.1f}) with group_spawn_margin "
                f"{m:.1f} m leaves the {field[0]:.1f} x {field[1]:.1f} m field")
    if walkable is not None:
        ix, iy = int(cx / hscale), int(cy / hscale)
        if not (0 <= ix < walkable.shape[0] and 0 <= iy < walkable.shape[1]) or int(walkable[ix, iy]) != 0:
            return (f"group_spawn_centre: ({cx:.1f}, {cy:.1f}) is not walkable ground; the centre is where a member goes when no candidate is "
                    "admissible, so it must be")
    return None


class CrowdSpawn:
    def __init__(self, *, roots, n_env, group_size, walkable, hscale, min_dist, tries, extent, centre, margin):
        """roots: the [E][>= 2] float32 root states, rows a fixed stride apart (a view is fine); walkable: [rows][cols], 0: walkable;
        the box is the field less `margin` on every side."""
        L.require_device()
        from .sim import dptr
        self.lib = L.load()
        assert roots.dtype == torch.float32 and roots.dim() == 2 and roots.shape[0] == int(n_env) and roots.stride(1) == 1
        dev = roots.device
        self.device, self.n_env, self.group_size, self.tries = dev, int(n_env), int(group_size), int(tries)
        if self.group_size < 1 or self.n_env % self.group_size != 0:
            raise CrowdSpawnError(f"num_env_group: numEnvs ({self.n_env}) is not a multiple of the group size ({self.group_size})")
        self.n_groups = self.n_env // self.group_size
        self.min_dist, self.extent, self.margin = float(min_dist), float(extent), float(margin)
        self.walkable = walkable.to(device=dev, dtype=torch.int16).contiguous()
        rows, cols = (int(v) for v in self.walkable.shape)
        self.box = (self.margin, rows * float(hscale) - self.margin, self.margin, cols * float(hscale) - self.margin)
        self.centres = torch.tensor([list(centre)] * self.n_groups, dtype=torch.float32, device=dev)
        self.mark_ws = torch.full((self.n_env,), -1, dtype=torch.int32, device=dev)
        self.place_xy = torch.zeros((self.n_env, 2), dtype=torch.float32, device=dev)
        self.info = torch.zeros((self.n_env, 4), dtype=torch.int32, device=dev)          # EmlocoCrowdSpawnInfo rows, as words
        # placements, crowded, no-ground (int64) and the smallest clearance2 (float32) since the last `totals(clear=True)`
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)
        self.min_c2 = torch.full((), float("inf"), dtype=torch.float32, device=dev)
        self.last_ids, self.last_u, self.last_roots = None, None, None
        self.keep_roots = False              # tests: also keep a copy of the root xy the call read (`last_roots`)
        self._keep = roots
        p = lambda t: dptr(t).value
        self.bufs = L.CrowdSpawn(self.n_env, self.group_size, self.tries, int(roots.stride(0)), rows, cols, float(hscale), *self.box,
                                 self.extent, self.min_dist, 0, roots.data_ptr(), p(self.walkable), p(self.centres), p(self.mark_ws),
                                 p(self.place_xy), p(self.info))

    def clearance2(self):
        """[E] float32 view of info's first word"""
        return self.info[:, 0].view(torch.float32)

    def run(self, env_ids=None, u=None):
        """Place every env, or the envs of an int32 id list on the device (-1 entries are skipped); `u` [n][tries][2] in [0, 1) is drawn
        here unless given.  The ids and the uniforms of the call are kept (`last_ids`, `last_u`)."""
        from .sim import current_stream_handle, dptr
        n = self.n_env if env_ids is None else int(env_ids.numel())
        if n == 0:
            return
        if env_ids is not None:
            env_ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        if u is None:
            u = torch.rand((n, self.tries, 2), dtype=torch.float32, device=self.device)
        assert u.shape == (n, self.tries, 2) and u.dtype == torch.float32 and u.is_contiguous()
        self.last_ids, self.last_u = env_ids, u
        if self.keep_roots:
            self.last_roots = self._keep[:, :2].clone()
        rc = self.lib.emloco_task_crowd_spawn(C.byref(self.bufs), dptr(env_ids), 0 if env_ids is None else n, dptr(u),
                                              current_stream_handle(self.device))
        L.check(rc, "emloco_task_crowd_spawn")
        # the totals, with device ops (duplicates of an id count once: the rows are read through a mask)
        if env_ids is None:
            flags, c2 = self.info[:, 2], self.clearance2()
            placed = torch.tensor(self.n_env, dtype=torch.int64, device=self.device)
        else:
            mask = torch.zeros(self.n_env + 1, dtype=torch.bool, device=self.device)
            idx = env_ids.long()
            mask[torch.where((idx >= 0) & (idx < self.n_env), idx, self.n_env)] = True
            mask = mask[:self.n_env]
            flags = torch.where(mask, self.info[:, 2], 0)
            c2 = torch.where(mask, self.clearance2(), float("inf"))
            placed = mask.sum()
        self.counts += torch.stack([placed, (flags & L.SPAWN_CROWDED).ne(0).sum(), (flags & L.SPAWN_NO_GROUND).ne(0).sum()])
        self.min_c2 = torch.minimum(self.min_c2, c2.min())

    def place(self, env_ids):
        """[n][2] the new root xy of the listed envs (a long or int tensor of env indices), in the list's order"""
        self.run(env_ids)
        return self.place_xy[env_ids.to(self.device).long()]

    def totals(self, clear=False):
        """dict(placements, crowded, no_ground, min_clearance [m] or None) since the last clear: the one host read"""
        n = [int(v) for v in self.counts.cpu()]
        c2 = float(self.min_c2.cpu())
        if clear:
            self.counts.zero_()
            self.min_c2.fill_(float("inf"))
        return dict(placements=n[0], crowded=n[1], no_ground=n[2], crowded_share=n[1] / n[0] if n[0] else 0.0,
                    min_clearance=math.sqrt(c2) if math.isfinite(c2) else None, min_dist=self.min_dist, extent=self.extent, tries=self.tries,
                    group_size=self.group_size)


def report_line(t):
    c = "-" if t["min_clearance"] is None else f"{t['min_clearance']:.2f} m"
    return (f"spawn: {t['placements']} placements in groups of {t['group_size']}, {t['crowded']} crowded ({100 * t['crowded_share']:.2f} %), "
            f"{t['no_ground']} without ground, smallest clearance {c} (min_dist {t['min_dist']:.2f} m, extent {t['extent']:.1f} m, {t['tries']} tries)")


def epoch_tail(t):
    c = "-" if t["min_clearance"] is None else f"{t['min_clearance']:.2f}"
    return f"\tspawn placed/crowded/no-ground {t['placements']}/{t['crowded']}/{t['no_ground']} min_clear {c}"

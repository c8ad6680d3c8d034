"""Python side of the crowd contact audit (include/emloco_task.h: EmlocoCrowdContacts, emloco_crowd_contacts*).

The members of a group see each other on the crowd sensor's height map but do not collide: every env is its own rigid-body problem.
The audit measures how close they come -- once per control step, on the device, without a host read: per env the horizontal distance
to the nearest member of its group and the deepest overlap of its collision capsules (the table the self-collision step uses,
`model.pack_self_collision`) with any member's.  A second launch keeps per-game accumulators and, at a game's end, a 48-byte record;
with epoch totals on it also adds to per-env sums that one reduction folds once per epoch.  The reference computes no such number (its
engine gives a group one collision group, humanoid.py:838-864): the metrics are this project's.

`near_dist` (default 1.0 m: the crowd sensor draws a person as a 0.5 x 1.0 m box) is this project's choice; it is configurable and
written into every report.  The kernels run on torch's current stream.
"""
import ctypes as C

import numpy as np

from . import _lib as L

# EmlocoCrowdContactNow (32 bytes) and EmlocoCrowdContactRecord (48 bytes)
NOW_DTYPE = np.dtype([("nearest", "<f4"), ("pen", "<f4"), ("nearest_member", "<i4"), ("pen_member", "<i4"), ("pen_segs", "<i4"),
                      ("n_pen", "<i4"), ("n_near", "<i4"), ("flags", "<i4")])
RECORD_DTYPE = np.dtype([("min_nearest", "<f4"), ("mean_nearest", "<f4"), ("max_pen", "<f4"), ("steps", "<i4"), ("nonfinite_steps", "<i4"),
                         ("near_steps", "<i4"), ("contact_steps", "<i4"), ("contacts", "<i4"), ("pen_member", "<i4"), ("pen_segs", "<i4"),
                         ("pen_step", "<i4"), ("first_contact_step", "<i4")])
NOW_WORDS, RECORD_WORDS = NOW_DTYPE.itemsize // 4, RECORD_DTYPE.itemsize // 4
# the moment vector of emloco_crowd_contacts_reduce (EMLOCO_CCM_*) and the epoch vector of emloco_crowd_contacts_epoch_reduce (EMLOCO_CCT_*)
MOMENT_NAMES = ("games", "games_contact", "games_start_contact", "sum_steps", "sum_contact_steps", "sum_near_steps", "sum_contacts",
                "sum_nonfinite_steps", "sum_max_pen", "sum_max_pen2", "sum_min_nearest", "sum_mean_nearest", "games_neighbour")
TOTAL_NAMES = ("steps", "nonfinite_steps", "contact_steps", "contacts", "near_steps", "sum_nearest", "sum_pen", "max_pen", "min_nearest",
               "games", "games_contact", "games_start_contact", "neighbour_steps")
assert len(MOMENT_NAMES) == L.CROWD_CONTACT_MOMENTS and len(TOTAL_NAMES) == L.CROWD_CONTACT_TOTALS
DEFAULT_NEAR_DIST = 1.0


class CrowdContactRefusal(ValueError):
    """The audit cannot run on this task or configuration; the text names what is missing."""


def config_refusal(env_cfg):
    """Why the audit cannot run on cfg["env"], or None -- read off the configuration alone, no device touched."""
    if not env_cfg.get("divide_group", False):
        return ("the crowd contact audit measures the members of a group against each other: the configuration has divide_group: False "
                "(no groups, the envs are not meant to meet)")
    if not env_cfg.get("has_self_collision", False):
        return ("the crowd contact audit uses the collision capsules of the self-collision step: the configuration has "
                "has_self_collision: False (no capsule table)")
    return None


def moments_from_records(rec):
    """The moment vector of a structured array of records (the RECORD_DTYPE columns), in float64, summed in record order -- what
    emloco_crowd_contacts_reduce computes on the device (there in a fixed tree order).  Sums and counts only: the moments of two shards
    add up to the moments of their union."""
    m = np.zeros(len(MOMENT_NAMES), np.float64)
    col = lambda k, sel=slice(None): rec[k][sel].astype(np.float64)
    touched, met = rec["contact_steps"] > 0, rec["min_nearest"] >= 0
    m[L.CCM_GAMES], m[L.CCM_GAMES_CONTACT] = len(rec), int(np.count_nonzero(touched))
    m[L.CCM_GAMES_START_CONTACT] = int(np.count_nonzero(touched & (rec["first_contact_step"] == 1)))
    for i, k in ((L.CCM_STEPS, "steps"), (L.CCM_CONTACT_STEPS, "contact_steps"), (L.CCM_NEAR_STEPS, "near_steps"), (L.CCM_CONTACTS, "contacts"),
                 (L.CCM_NONFINITE_STEPS, "nonfinite_steps")):
        m[i] = float(np.add.reduce(col(k)))
    p = col("max_pen", touched)
    m[L.CCM_SUM_MAX_PEN], m[L.CCM_SUM_MAX_PEN2] = float(np.add.reduce(p)), float(np.add.reduce(p * p))
    m[L.CCM_SUM_MIN_NEAREST], m[L.CCM_SUM_MEAN_NEAREST] = float(np.add.reduce(col("min_nearest", met))), float(np.add.reduce(col("mean_nearest", met)))
    m[L.CCM_GAMES_NEIGHBOUR] = int(np.count_nonzero(met))
    return m


def crowd_from_moments(m, near_dist=DEFAULT_NEAR_DIST, group_size=None):
    """The `crowd` block of the report from a moment vector: a dict of the numbers and `lines`.  The penetration is averaged over the
    games with a contact, the distances over the games with a neighbour, the shares of steps over all finite steps.  The deepest
    penetration of all games is not a sum: the evaluator takes it, like the correlations, from the records (`crowd_from_records`)."""
    m = [float(x) for x in m]
    n = m[L.CCM_GAMES]
    base = {"near_dist": float(near_dist), "group_size": group_size}
    if n < 1:
        return dict(base, games=0, lines=["crowd: no game finished"])
    nan = float("nan")
    nc, nn, steps = m[L.CCM_GAMES_CONTACT], m[L.CCM_GAMES_NEIGHBOUR], m[L.CCM_STEPS]
    r = dict(base, games=int(round(n)), games_contact=int(round(nc)), contact_game_share=nc / n,
             start_contact_share=m[L.CCM_GAMES_START_CONTACT] / n,
             contact_step_share=m[L.CCM_CONTACT_STEPS] / steps if steps >= 1 else nan,
             near_step_share=m[L.CCM_NEAR_STEPS] / steps if steps >= 1 else nan,
             contacts_per_step=m[L.CCM_CONTACTS] / steps if steps >= 1 else nan,
             nonfinite_steps=int(round(m[L.CCM_NONFINITE_STEPS])),
             av_max_pen=m[L.CCM_SUM_MAX_PEN] / nc if nc >= 1 else nan,
             std_max_pen=_std(nc, m[L.CCM_SUM_MAX_PEN], m[L.CCM_SUM_MAX_PEN2]) if nc >= 1 else nan,
             av_min_nearest=m[L.CCM_SUM_MIN_NEAREST] / nn if nn >= 1 else nan,
             av_mean_nearest=m[L.CCM_SUM_MEAN_NEAREST] / nn if nn >= 1 else nan)
    r["lines"] = [
        f"crowd: {r['games']} games in groups of {group_size}, near_dist {r['near_dist']:.2f} m; games with a contact: "
        f"{100.0 * r['contact_game_share']:.1f} %, started in contact: {100.0 * r['start_contact_share']:.1f} %",
        f"steps in contact: {100.0 * r['contact_step_share']:.2f} %, steps with a member nearer than near_dist: {100.0 * r['near_step_share']:.2f} %",
        f"av_max_pen: {r['av_max_pen']:.4f}, std_max_pen: {r['std_max_pen']:.4f} (games with a contact), av_min_nearest: {r['av_min_nearest']:.3f}, "
        f"av_mean_nearest: {r['av_mean_nearest']:.3f}",
    ]
    return r


def _std(n, s, s2):
    return float(np.sqrt(max(s2 / n - (s / n) ** 2, 0.0)))


def crowd_from_records(values, rec):
    """What the moments do not carry, in float64 from the gathered records: the deepest penetration of all games, and per network
    (`values`: one array per network, the games of `rec` in its order) Pearson r of `value` against max_pen and against the 0 / 1 "had a
    contact" -- whether LocoVal's value knows anything about the other people.  NaN where a variance is zero."""
    out = {"max_pen": float(rec["max_pen"].max()) if len(rec) else 0.0, "corr_value_max_pen": [], "corr_value_contact": []}
    for v in values:
        v = np.asarray(v).astype(np.float64)
        for name, y in (("max_pen", rec["max_pen"].astype(np.float64)), ("contact", (rec["contact_steps"] > 0).astype(np.float64))):
            ok = len(v) > 1 and v.std() > 0 and y.std() > 0
            out["corr_value_" + name].append(float(np.corrcoef(v, y)[0, 1]) if ok else float("nan"))
    return out


def epoch_from_totals(t, near_dist=DEFAULT_NEAR_DIST, group_size=None):
    """The `crowd` dict of a training epoch from the epoch vector of emloco_crowd_contacts_epoch_reduce."""
    t = [float(x) for x in t]
    steps, met = t[L.CCT_STEPS], t[L.CCT_NEIGHBOUR_STEPS]
    share = lambda x: x / steps if steps >= 1 else 0.0
    out = {k: (int(round(t[i])) if k not in ("sum_nearest", "sum_pen", "max_pen", "min_nearest") else t[i]) for i, k in enumerate(TOTAL_NAMES)}
    out.update(contact_step_share=share(t[L.CCT_CONTACT_STEPS]), near_step_share=share(t[L.CCT_NEAR_STEPS]),
               mean_nearest=t[L.CCT_SUM_NEAREST] / met if met >= 1 else 0.0, near_dist=float(near_dist), group_size=group_size)
    return out


def epoch_tail(crowd):
    """The short tail of the --stats line: share of steps in contact, deepest penetration, mean nearest distance."""
    return f"\tcrowd contact {100.0 * crowd['contact_step_share']:.2f}% pen_max {crowd['max_pen']:.3f} nearest {crowd['mean_nearest']:.2f}"


class CrowdContactAudit:
    """Owns the device copy of the capsule table, the workspaces, now[E], the games' accumulators and, on request, the records
    (`games_per_env` > 0: [E][games_per_env]) and the epoch totals (`totals`).  `task`: the env's task object; its simulator
    (task.sim.native) must hold a self-collision table, and the task must form groups (divide_group)."""

    def __init__(self, task, near_dist=DEFAULT_NEAR_DIST, games_per_env=0, totals=False):
        import torch
        from .crowd_sensor import group_layout
        self.task = task
        if not getattr(task, "_divide_group", False):
            raise CrowdContactRefusal("CrowdContactAudit: the task has divide_group: False -- without groups the envs are not meant to meet, "
                                      "and there is nobody to measure against")
        native = getattr(getattr(task, "sim", None), "native", None)
        sc = getattr(native, "_sc", None)
        if sc is None or sc.get("seg_body") is None:
            raise CrowdContactRefusal("CrowdContactAudit: the task's simulator was built without self-collision (has_self_collision: False): "
                                      "it holds no collision capsule table (model.pack_self_collision)")
        near_dist = float(near_dist)
        if not (np.isfinite(near_dist) and near_dist > 0.0):
            raise CrowdContactRefusal(f"CrowdContactAudit: near_dist {near_dist} is not a finite positive length")
        self.device = torch.device(task.device)
        if self.device.type != "cuda":
            raise RuntimeError("CrowdContactAudit runs HIP kernels: it needs libemloco_hip.so and a gfx950 device")
        self.lib = L.require_device()
        self.native = native
        self.num_envs = E = int(task.num_envs)
        self.group_size = group_layout(E, task._group_num_people)[0]
        if self.group_size < 2:
            raise CrowdContactRefusal(f"CrowdContactAudit: num_env_group gives groups of {self.group_size}: a group needs two members")
        self.near_dist, self.games_per_env = near_dist, int(games_per_env)
        self.n_seg = int(sc["seg_body"].shape[0])
        dev = self.device
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        self.cap_a, self.cap_b, self.cap_r = up(sc["cap_a"], np.float32), up(sc["cap_b"], np.float32), up(sc["cap_r"], np.float32)
        assert tuple(self.cap_a.shape) == (E, self.n_seg, 3) and tuple(self.cap_r.shape) == (E, self.n_seg)
        self.seg_body = up(sc["seg_body"], np.uint8)
        zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        self.caps_ws = torch.zeros(E * 32 * 8, dtype=torch.float32, device=dev)          # EMLOCO_SC_MAXSEG segments of 8 floats
        self.roots_ws = torch.zeros(E * 4, dtype=torch.float32, device=dev)
        self._now = zi(E * NOW_WORDS)
        self.game_ws = torch.zeros(E * L.CROWD_CONTACT_WS // 2, dtype=torch.int64, device=dev)     # (8-byte aligned: it holds doubles)
        self._records = zi(E * self.games_per_env * RECORD_WORDS) if self.games_per_env > 0 else None
        self._totals = torch.zeros(E * L.CROWD_CONTACT_TOTALS, dtype=torch.float64, device=dev) if totals else None
        self._moments = torch.zeros(L.CROWD_CONTACT_MOMENTS, dtype=torch.float64, device=dev)
        self._epoch = torch.zeros(L.CROWD_CONTACT_TOTALS, dtype=torch.float64, device=dev)
        self._slot = None
        self.steps = 0
        rb = native.rigid_body_state
        assert rb.is_contiguous() and rb.dtype == torch.float32 and rb.numel() == E * L.NB * 13
        p = lambda t: None if t is None else t.data_ptr()
        self.bufs = L.CrowdContacts(n_env=E, group_size=self.group_size, n_seg=self.n_seg, games_per_env=self.games_per_env,
                                    near_dist=self.near_dist, rb_state=p(rb), cap_a=p(self.cap_a), cap_b=p(self.cap_b), cap_r=p(self.cap_r),
                                    seg_body=p(self.seg_body), caps_ws=p(self.caps_ws), roots_ws=p(self.roots_ws), game_ws=p(self.game_ws),
                                    records=p(self._records), totals=p(self._totals))

    # ------------------------------------------------------------------ per step
    def geometry(self):
        """now[E] of the simulator's current body state (two launches)."""
        from .sim import current_stream_handle
        L.check(self.lib.emloco_crowd_contacts(C.byref(self.bufs), self._now.data_ptr(), current_stream_handle(self.device)),
                "emloco_crowd_contacts")

    def step(self, done=None, slot=None):
        """The geometry and the bookkeeping of one control step.  done: this step's end-of-game flags on the device (uint8 / bool or
        int64, [E]) or None; slot: int32 [E], the slot of every env's game in progress (needed with records)."""
        import torch
        from .sim import current_stream_handle
        b = self.bufs
        b.done8 = b.done64 = None
        if done is not None:
            assert done.numel() == self.num_envs and done.is_contiguous()
            if done.dtype in (torch.uint8, torch.bool):
                b.done8 = done.data_ptr()
            elif done.dtype == torch.int64:
                b.done64 = done.data_ptr()
            else:
                raise TypeError(f"CrowdContactAudit.step: done must be uint8, bool or int64, not {done.dtype}")
        if slot is not None:
            assert slot.dtype == torch.int32 and slot.numel() == self.num_envs and slot.is_contiguous()
            self._slot = slot
        b.slot = None if slot is None else slot.data_ptr()
        self.geometry()
        L.check(self.lib.emloco_crowd_contacts_accumulate(C.byref(b), self._now.data_ptr(), current_stream_handle(self.device)),
                "emloco_crowd_contacts_accumulate")
        self.steps += 1

    # ------------------------------------------------------------------ reads
    def now(self):
        """now[E] as a structured array (a host read)."""
        return self._now.cpu().numpy().view(NOW_DTYPE).copy()

    def _games(self):
        if self._records is None or self._slot is None:
            raise RuntimeError("CrowdContactAudit: no records (games_per_env = 0, or no step(slot=...) yet)")
        return self._slot

    def records(self):
        """The recorded games (RECORD_DTYPE columns plus `env` and `game`), env-major: the slots below every env's count."""
        E, G = self.num_envs, self.games_per_env
        games = np.minimum(self._games().cpu().numpy(), G)
        raw = self._records.cpu().numpy().view(RECORD_DTYPE).reshape(E, G)
        env, game = np.nonzero(np.arange(G)[None, :] < games[:, None])
        out = np.zeros(len(env), dtype=[(k, RECORD_DTYPE.fields[k][0]) for k in RECORD_DTYPE.names] + [("env", "<i4"), ("game", "<i4")])
        for k in RECORD_DTYPE.names:
            out[k] = raw[k][env, game]
        out["env"], out["game"] = env, game
        return out

    def moments(self):
        """The moment vector of all ranks: one reduction, one all-reduce(sum)."""
        from . import dist as D
        from .sim import current_stream_handle
        L.check(self.lib.emloco_crowd_contacts_reduce(self.num_envs, self.games_per_env, self._records.data_ptr(), self._games().data_ptr(),
                                                      self._moments.data_ptr(), current_stream_handle(self.device)), "emloco_crowd_contacts_reduce")
        m = self._moments.clone()
        D.all_reduce_(m)
        return m.cpu().numpy()

    def end_epoch(self):
        """The epoch's `crowd` dict of this rank (epoch_from_totals): one reduction, one host read; the totals start over."""
        from .sim import current_stream_handle
        if self._totals is None:
            raise RuntimeError("CrowdContactAudit: built without totals")
        L.check(self.lib.emloco_crowd_contacts_epoch_reduce(self.num_envs, self._totals.data_ptr(), self._epoch.data_ptr(),
                                                            current_stream_handle(self.device)), "emloco_crowd_contacts_epoch_reduce")
        return epoch_from_totals(self._epoch.cpu().numpy(), self.near_dist, self.group_size)

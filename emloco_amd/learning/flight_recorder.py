"""Flight recorder: the last few control steps of every env in a ring on the device, frozen into a capture slot when the env trips a
trigger -- a non-finite body state, a body faster than a limit, an early fall, a request of the host -- and written to a file once per
epoch, from which `tools/replay_capture.py` replays each capture through the CPU oracle bit for bit.

Two launches bracket the rigid-body step (include/emloco_task.h, csrc/recorder_kernels.hip):

    record()   behind the step's drive input, ahead of the rigid-body launch: every env's step INPUTS into ring row t % depth
               (`BaseTask.before_physics_launch` is where a bound recorder does it)
    check()    where `EpisodeStats.step()` sits -- behind the post-physics pass, ahead of any reset: cause bits, claim, copy

The recorder reads the simulation and writes only its own buffers.  It needs every writer of the env state ordered on the caller's
stream ahead of those two points.  `fused_chain` keeps the whole chain on one stream and `overlap_obs` moves a reader of the state
aside (the observation launch), so both are supported; `overlap_reset` runs the reset chain -- a writer -- on a second stream beside
the step, and a recorder refuses a task that has it on.

`load()` and the layout helpers are plain numpy: reading a capture file needs neither the device library nor a device."""
import ctypes as C
import types

import numpy as np

NB, NDOF, MAXCAND = 24, 69, 96
REC_WORDS, REC_POST_WORDS, REC_COUNTERS = 512, 892, 8
CAUSES = ("nonfinite", "speed", "ang_speed", "early_fall", "request")              # bit k of the cause word: EMLOCO_REC_*
CAUSE_BITS = {name: 1 << k for k, name in enumerate(CAUSES)}
RECORD_FIELDS = (("root", (13,)), ("dof", (NDOF, 2)), ("warm", (MAXCAND, 3)), ("drive", (NDOF,)))
POST_FIELDS = (("root", (13,)), ("dof", (NDOF, 2)), ("warm", (MAXCAND, 3)), ("rb", (NB, 13)), ("contact_force", (NB, 3)), ("dof_force", (NDOF,)))
SHARED_MODEL_KEYS = ("parent", "geom_type")                    # of pack_models: one row for all envs
SHARED_SC_KEYS = ("pairs", "seg_body", "k", "c", "max_pen", "mu")
PARAM_FIELDS = ("n_sub", "n_iter", "h", "gravity_z", "contact_offset", "erp", "max_depen_vel", "mu", "ang_damping", "max_ang_vel",
                "ground_z", "cfm", "warm", "drive_mode")


def slot_words(depth):
    return 4 + int(depth) * REC_WORDS + REC_POST_WORDS


def cause_names(bits):
    return [n for n, b in CAUSE_BITS.items() if int(bits) & b]


def _split(words, fields):
    out, o = {}, 0
    for name, shape in fields:
        n = int(np.prod(shape))
        out[name] = words[o:o + n].view(np.float32).reshape(shape)
        o += n
    assert o == words.size
    return out


def parse_slot(words, depth):
    """One capture slot (uint32 words) as a dict: env, t, cause, n_valid, records [{progress, t, drive_mode, root, dof, warm, drive}]
    oldest first (the valid ones), post {root, dof, warm, rb, contact_force, dof_force}.  The float arrays are views of `words`."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    assert words.shape == (slot_words(depth),)
    env, t, cause, n_valid = (int(words[0]), int(words[1].view(np.int32)), int(words[2]), int(words[3]))
    records = []
    for j in range(n_valid):
        r = words[4 + j * REC_WORDS:4 + (j + 1) * REC_WORDS]
        rec = dict(progress=int(r[0].view(np.int32)), t=int(r[1].view(np.int32)), drive_mode=int(r[2]))
        rec.update(_split(r[4:], RECORD_FIELDS))
        records.append(rec)
    return dict(env=env, t=t, cause=cause, n_valid=n_valid, records=records, post=_split(words[4 + depth * REC_WORDS:], POST_FIELDS))


def load(path):
    """The dict `save` wrote (plain numpy).  Keys: captures [K][slot words] uint32, depth, n_calls, substeps, overflow [5], params/*,
    model/* and sc/* (per-env arrays: row k belongs to capture k), ground/*."""
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def capture_file(captures, depth, packed, self_collision, params, n_calls=1, heightfield=None, missed=None):
    """The dict of a capture file.  `packed` / `self_collision`: the arrays of model.pack_models / pack_self_collision (or None) for
    ALL envs of the run -- the rows of the captured envs are kept; `params`: an EmlocoSimParams-shaped object; `heightfield`: the
    ground's dict (samples, horizontal_scale, vertical_scale[, origin_x, origin_y, move_x, move_y]) or None for the plane."""
    captures = np.ascontiguousarray(captures, dtype=np.uint32).reshape(-1, slot_words(depth))
    envs = captures[:, 0].astype(np.int64)
    out = dict(captures=captures, depth=np.int32(depth), n_calls=np.int32(n_calls), substeps=np.int32(int(params.n_sub) * int(n_calls)),
               overflow=np.array([int((missed or {}).get(c, 0)) for c in CAUSES], np.int32))
    for f in PARAM_FIELDS:
        out["params/" + f] = np.asarray(getattr(params, f))
    for k, v in packed.items():
        out["model/" + k] = np.asarray(v) if k in SHARED_MODEL_KEYS else np.asarray(v)[envs]
    out["sc_on"] = np.int32(self_collision is not None)
    if self_collision is not None:
        for k, v in self_collision.items():
            if v is not None:
                out["sc/" + k] = np.asarray(v) if k in SHARED_SC_KEYS else np.asarray(v)[envs]
    if heightfield is None:
        out["ground/plane_z"] = np.float32(params.ground_z)
    else:
        out["ground/samples"] = np.ascontiguousarray(heightfield["samples"], dtype=np.int16)
        for k in ("horizontal_scale", "vertical_scale", "origin_x", "origin_y"):
            out["ground/" + k] = np.float32(heightfield.get(k, 0.0))
        if heightfield.get("move_x") is not None:
            out["ground/move_x"] = np.ascontiguousarray(heightfield["move_x"], dtype=np.int8)
            out["ground/move_y"] = np.ascontiguousarray(heightfield["move_y"], dtype=np.int8)
    return out


def write(path, file_dict):
    with open(path, "wb") as f:                                # (a file object: numpy does not append ".npz" to the name)
        np.savez(f, **file_dict)
    return path


def sim_view(native, heightfield=None, n_calls=1):
    """A bare NativeSim with zeroed flag buffers, as the object a FlightRecorder binds to (tests, tools)."""
    import torch
    z = lambda: torch.zeros(native.num_envs, dtype=torch.int64, device=native.device)
    return types.SimpleNamespace(sim=types.SimpleNamespace(native=native, heightfield=heightfield), num_envs=native.num_envs,
                                 device=native.device, control_freq_inv=int(n_calls), progress_buf=z(), reset_buf=z(), _terminate_buf=z())


class FlightRecorder:
    """Owns the ring (n_env x depth x 2 KB: 64 MiB at 4096 x 8), the slots and the counters.  `task`: the env's task object (or
    `sim_view(...)`).  `speed` [m/s], `ang_speed` [rad/s], `early_fall` [steps]: None leaves the cause off."""

    def __init__(self, task, depth=8, slots=16, speed=None, ang_speed=None, early_fall=None, nonfinite=True):
        import torch
        from .. import _lib as L
        self.task = task
        self._refuse_overlap_reset()
        self.device = torch.device(task.device)
        if self.device.type != "cuda":
            raise RuntimeError("FlightRecorder records in HIP kernels: it needs libemloco_hip.so and a gfx950 device")
        self.lib = L.require_device()
        self.native = task.sim.native
        self.num_envs = E = int(task.num_envs)
        self.depth, self.n_slots = int(depth), int(slots)
        if self.depth < 1 or self.n_slots < 1:
            raise ValueError("FlightRecorder: depth and slots must be at least 1")
        for name, v in (("speed", speed), ("ang_speed", ang_speed)):
            if v is not None and not (float(v) >= 0.0):
                raise ValueError(f"FlightRecorder: {name} must be a non-negative number")
        self.cause_mask = ((L.REC_NONFINITE if nonfinite else 0) | (L.REC_SPEED if speed is not None else 0)
                           | (L.REC_ANG_SPEED if ang_speed is not None else 0) | (L.REC_EARLY_FALL if early_fall is not None else 0) | L.REC_REQUEST)
        sq = lambda v: 0.0 if v is None else float(np.float32(v) * np.float32(v))
        self.speed2_limit, self.ang_speed2_limit = sq(speed), sq(ang_speed)
        self.early_fall_steps = 0 if early_fall is None else int(early_fall)
        self.grid = 0
        self.ring = torch.zeros(E, self.depth, REC_WORDS, dtype=torch.int32, device=self.device)
        self.slots = torch.zeros(self.n_slots, slot_words(self.depth), dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(REC_COUNTERS, dtype=torch.int32, device=self.device)
        self.last_capture_step = torch.full((E,), -(1 << 30), dtype=torch.int32, device=self.device)
        self.cause_ws = torch.zeros(E, dtype=torch.int32, device=self.device)
        self.request_buf = torch.zeros(E, dtype=torch.uint8, device=self.device)
        self.t = 0                  # the control step the next record() belongs to
        self.t0 = None
        self._recorded = None       # the step the last record() was for
        self._bufs = None
        self._hooked = False

    def _refuse_overlap_reset(self):
        """A loop may switch the arrangement on after the recorder was built (LocoValRollout does it in its constructor): looked at
        when the recorder is built, when it is bound and ahead of every record() -- one attribute read."""
        if getattr(self.task, "overlap_reset", False):
            raise RuntimeError("FlightRecorder: the task has overlap_reset on -- the reset chain writes env state on a second stream beside "
                               "the step, and the recorder needs every writer ordered on the caller's stream")

    # ------------------------------------------------------------------ the structure
    def _flag_ptrs(self):
        task = self.task
        post = getattr(task, "_post_bufs", None)
        if post is None and hasattr(task, "_ensure_post_bufs"):
            post = task._ensure_post_bufs()
        if post is not None:                                   # the addresses the post-physics kernel itself writes
            return post.progress_buf, post.reset_buf, post.terminate_buf
        return task.progress_buf.data_ptr(), task.reset_buf.data_ptr(), task._terminate_buf.data_ptr()

    def bufs(self):
        """The structure, built once.  The simulator's tensors and the recorder's own buffers live as long as both objects; what may
        change between two calls is refreshed by plain field writes, without a call into the library: the live drive mode (NativeSim
        keeps it), t0, the settings a caller may edit, and the task's three flag buffers (a task may rebuild its EmlocoTaskBufs)."""
        from .. import _lib as L
        n, b = self.native, self._bufs
        if b is None:
            p = lambda t: t.data_ptr()
            b = self._bufs = L.RecorderBufs(
                n_env=self.num_envs, depth=self.depth, n_slots=self.n_slots,
                root_state=p(n.root_state), dof_state=p(n.dof_state), warm_start=p(n.warm_start), drive=p(n.pd_target),
                rb_state=p(n.rigid_body_state), contact_force=p(n.contact_force), dof_force=p(n.dof_force), ring=p(self.ring),
                slots=p(self.slots), counters=p(self.counters), last_capture_step=p(self.last_capture_step), cause_ws=p(self.cause_ws),
                request=p(self.request_buf))
        mode = getattr(n, "drive_mode", None)
        b.drive_mode = int(n.get_params().drive_mode if mode is None else mode)
        b.t0 = int(self.t if self.t0 is None else self.t0)
        b.cause_mask, b.early_fall_steps, b.grid = self.cause_mask, self.early_fall_steps, int(self.grid)
        b.speed2_limit, b.ang_speed2_limit = self.speed2_limit, self.ang_speed2_limit
        b.progress_buf, b.reset_buf, b.terminate_buf = self._flag_ptrs()
        return b

    # ------------------------------------------------------------------ the two launches
    def record(self):
        """The inputs of the step about to be launched into the ring (one launch on the caller's stream)."""
        from .. import _lib as L
        from ..sim import current_stream_handle
        self._refuse_overlap_reset()
        if self.t0 is None:
            self.t0 = self.t
        L.check(self.lib.emloco_recorder_record(C.byref(self.bufs()), self.t, current_stream_handle(self.device)), "emloco_recorder_record")
        self._recorded = self.t

    def check(self):
        """Triggers, claim and copy for the step recorded last (three launches on the caller's stream); then the step counter moves on."""
        from .. import _lib as L
        from ..sim import current_stream_handle
        if self.t0 is None or self._recorded != self.t:
            raise RuntimeError("FlightRecorder.check(): no record() for this step -- call record() ahead of the rigid-body launch "
                               "(bind() hooks it into the task's step)")
        L.check(self.lib.emloco_recorder_check(C.byref(self.bufs()), self.t, current_stream_handle(self.device)), "emloco_recorder_check")
        self.t += 1

    def bind(self):
        """record() from the task's `before_physics_launch` hook (BaseTask.step); returns self.  Raises on a task with overlap_reset on."""
        self._refuse_overlap_reset()
        self.task.before_physics_launch = self.record
        self._hooked = True
        return self

    def unbind(self):
        if self._hooked and getattr(self.task, "before_physics_launch", None) == self.record:
            self.task.before_physics_launch = None
        self._hooked = False

    def request(self, env_ids):
        """Ask for a capture of these envs at the next check(): a device-side write of their request bytes, no synchronisation."""
        import torch
        ids = torch.as_tensor(env_ids, dtype=torch.int64).reshape(-1)
        if ids.device.type == "cpu" and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.num_envs):
            raise ValueError("FlightRecorder.request: env id out of range")          # (a device list is the caller's to keep in range)
        self.request_buf.index_fill_(0, ids.to(self.device, non_blocking=True), 1)

    # ------------------------------------------------------------------ once per epoch
    def drain(self):
        """One read of the counter block; only if captures were taken, one copy of the used slots.  Returns (captures uint32
        [K][slot words], {cause: envs that found no slot}) and clears the counters."""
        counters = self.counters.cpu().numpy()
        k = int(counters[0])
        missed = {name: int(counters[1 + i]) for i, name in enumerate(CAUSES)}
        if k > 0:
            captures = self.slots[:k].cpu().numpy().view(np.uint32).copy()
        else:
            captures = np.zeros((0, slot_words(self.depth)), np.uint32)
        if k > 0 or any(missed.values()):
            self.counters.zero_()
        return captures, missed

    def save(self, path, captures, missed=None):
        """An .npz with everything a replay needs: the captures, the captured envs' model rows (and self-collision rows), the engine
        parameters, the substeps per control step and the ground."""
        n = self.native
        return write(path, capture_file(captures, self.depth, n._packed, getattr(n, "_sc", None), n.get_params(),
                                        int(getattr(self.task, "control_freq_inv", 1)), getattr(self.task.sim, "heightfield", None), missed))


def rank_path(path, rank, world):
    """`PATH` for a single-rank run, `PATH` with `_rank{r}` ahead of the extension for rank r of several"""
    if world <= 1:
        return path
    stem, dot, ext = path.rpartition(".")
    return f"{stem}_rank{rank}.{ext}" if dot and "/" not in ext else f"{path}_rank{rank}"


def part_path(path, part):
    """`PATH` for the first file of a run, `PATH` with `_part{n}` ahead of the extension for the n-th further one"""
    if part <= 0:
        return path
    stem, dot, ext = path.rpartition(".")
    return f"{stem}_part{part}.{ext}" if dot and "/" not in ext else f"{path}_part{part}"


class CaptureLog:
    """What a loop does with a recorder at the end of an epoch: drain, add the captures to the run's file, report the counts.  A file
    holds at most `per_file` captures (default 256, 5 MB at depth 8); then the run goes on in PATH_part1, PATH_part2, ...  -- so the
    host keeps, and an epoch with captures rewrites, one file's worth whatever the length of the run."""

    def __init__(self, recorder, path, per_file=256):
        self.recorder, self.path, self.per_file = recorder, path, max(int(per_file), 1)
        self.captures = np.zeros((0, slot_words(recorder.depth)), np.uint32)        # of the file being filled
        self.missed = {c: 0 for c in CAUSES}                                         # of the whole run so far
        self.part, self.paths, self.total = 0, [], 0

    def _write(self):
        path = part_path(self.path, self.part)
        self.recorder.save(path, self.captures, self.missed)
        if path not in self.paths:
            self.paths.append(path)

    def end_epoch(self):
        """-> dict(captures=<taken this epoch>, captures_missed={cause: count}); `paths` lists the run's files so far"""
        caps, missed = self.recorder.drain()
        for c, v in missed.items():
            self.missed[c] += v
        self.total += int(caps.shape[0])
        todo = caps
        while todo.shape[0]:
            room = self.per_file - self.captures.shape[0]
            if room == 0:                                    # the file is full (and written): the next one
                self.part, self.captures, room = self.part + 1, self.captures[:0], self.per_file
            self.captures = np.concatenate([self.captures, todo[:room]])
            todo = todo[room:]
            self._write()
        if not self.paths:                                   # (a run without captures still leaves a file that says so)
            self._write()
        return dict(captures=int(caps.shape[0]), captures_missed=missed)

"""Device conformance matrix of the rollout's task kernels (include/emloco_task.h) against float64 and the fp32 oracle.

Companion of tests/test_gpu_kernel_matrix.py and tests/test_gpu_elementwise_matrix.py: every case calls a C entry point directly through
ctypes.  Every output is a guarded buffer (a sentinel band before and behind it that must survive, NaN / an integer sentinel in the
logical output before the launch, compared as bits with a clone taken before the launch); every input carries garbage outside its
logical extent.  The case tables, the float64 references and the judges are those of tests/task_cases.py, which
tests/test_task_matrix_cpu.py runs through the emulator on a CPU: the device run differs in the executor only.

Covered: emloco_task_pd_targets / _pd_targets_copy, emloco_task_amp_rows, emloco_task_post_physics (values, the mode bits one by one and
combined, SKIP_DONE, AMP_DONE_ONLY, amp_ring for every head, indexed launches), emloco_task_get_heights on a non-square map,
emloco_task_compact_done / _snapshot / _order(sim = NULL), and emloco_task_traj_reset above 256 list entries (the grid-stride loop)
and with a negative id in the middle of its list.

Bars.  Copies, masks, counts, ids, flags, progress, "left as it was" regions, ring-vs-layout and chunked-vs-whole: bit for bit.  PD
targets: 2^-22 of |offset| + |scale a| (one fused or unfused rounding).  Height observations, map indices, reset / terminate / progress:
equal to the fp32 oracle (oracle.*), whose index and threshold arithmetic defines them.  Every other float output: MARGIN (8) x the
largest float32-vs-float64 error of the same kernel_refs function over the family's cases, measured as max error over the tensor's max
(the power reward: over sum |terms|).

Measured (MI355X, the run that accompanied this file; every run prints the figures, `pytest -s`; tests/test_task_matrix_cpu.py
reproduces the float32 column and the emulator's figures on any machine -- the emulator and the device agree to every digit shown):

    family / output                     float32 reference     bar (8 x)     emulator      device
    amp_rows rotation                   3.563e-07             2.851e-06     5.646e-07     5.646e-07
    amp_rows velocity                   1.705e-07             1.364e-06     1.711e-07     1.711e-07
    amp_rows dof_pos                    3.057e-07             2.445e-06     3.407e-07     3.407e-07
    amp_rows key_pos                    2.121e-07             1.697e-06     1.896e-07     1.896e-07
    post_physics amp rotation           4.142e-07             3.313e-06     5.696e-07     5.696e-07
    post_physics amp velocity           2.159e-07             1.727e-06     2.442e-07     2.442e-07
    post_physics amp dof_pos            3.483e-07             2.786e-06     3.366e-07     3.366e-07
    post_physics amp key_pos            2.668e-07             2.134e-06     2.668e-07     2.668e-07
    post_physics self_obs               2.345e-07             1.876e-06     2.397e-07     2.397e-07
    post_physics flip_self_obs          2.345e-07             1.876e-06     2.397e-07     2.397e-07
    post_physics loc_obs                1.034e-06             8.273e-06     1.034e-06     1.034e-06
    post_physics rew                    1.917e-06             1.534e-05     1.989e-06     1.989e-06
    post_physics loc_reward             6.602e-06             5.282e-05     6.602e-06     6.602e-06
    post_physics power_reward           1.574e-07             1.259e-06     1.756e-07     1.756e-07
    pd_targets (derived bar 2^-22)      --                    2.384e-07     1.132e-07     1.132e-07

(loc_reward = exp(-2 d^2): the 1e-6 class is the float32 rounding of d^2 up to 30 m^2 in the exponent, which the float32 reference shows
as well.)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R                                                          # noqa: E402
import task_cases as TC                                                          # noqa: E402
from task_cases import (POST_ADVANCE, POST_AMP_DONE_ONLY, POST_AMP_ROW, POST_AMP_SHIFT, POST_OBS, POST_RESET, POST_REWARD,  # noqa: E402
                        POST_SKIP_DONE, POST_STEP)
from test_gpu_kernel_matrix import DEV, GARBAGE, SENT, TAIL, _bits, _Guarded, _ptr, _stream          # noqa: E402

ISENT = -0x0123456789ABCDE                # guard-band sentinel of the integer buffers
OBS, AMP_STEPS, AMP_ROW = 1422, 15, 206


def _lib():
    from emloco_amd import _lib as L
    return L.require_device()


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _dev(t):
    _KEEP.append(torch.as_tensor(t).to(DEV).contiguous())
    return _KEEP[-1]


def _padded(t, garbage=None):
    """a device copy of t with garbage ahead of and behind its logical extent; returns the view of the logical part"""
    t = torch.as_tensor(t)
    if garbage is None:
        garbage = GARBAGE if t.dtype.is_floating_point else (30000 if t.dtype == torch.int16 else 77)
    lead = 16 // t.element_size() if t.element_size() <= 16 else 1
    buf = torch.full((lead + t.numel() + TAIL,), garbage, dtype=t.dtype, device=DEV)
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    _KEEP.append(buf)
    return v


class _GuardedInt:
    """an integer output of n entries with a sentinel band before and behind it and the sentinel in the logical output"""

    def __init__(self, n, dtype=torch.int64, fill=None):
        sent = ISENT if dtype == torch.int64 else -0x1234567
        self.n, self.buf = n, torch.full((TAIL + n + TAIL,), sent, dtype=dtype, device=DEV)
        if fill is not None:
            self.view().copy_(torch.as_tensor(fill).to(dtype))
        self.before = self.buf.clone()

    def view(self):
        return self.buf[TAIL:TAIL + self.n]

    def ptr(self):
        return _ptr(self.buf, TAIL)

    def set(self, values):
        self.view().copy_(torch.as_tensor(values).to(self.buf.dtype))
        self.before = self.buf.clone()

    def got(self):
        assert torch.equal(self.buf[:TAIL], self.before[:TAIL]) and torch.equal(self.buf[TAIL + self.n:], self.before[TAIL + self.n:]), \
            "a store landed outside an integer output (guard band changed)"
        return self.view().clone()

    def untouched(self):
        return torch.equal(self.buf, self.before)


def _fout(rows, cols):
    o = _Guarded(1, rows, cols, cols, 0, 4)
    o.fill()
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# pd_targets

@pytest.mark.parametrize("n", TC.PD_SIZES)
def test_pd_targets_and_copy_against_float64(n):
    lib = _lib()
    c = TC.case_pd(n, n)
    act, off, sc, mask = _padded(c["actions"]), _padded(c["offset"]), _padded(c["scale"]), _padded(c["zero_mask"])
    before = act.clone()
    results = []
    for variant in ("plain", "null", "distinct", "alias"):
        out, cp = _fout(n, 69), _fout(n, 69)
        if variant == "plain":
            rc = lib.emloco_task_pd_targets(n, _ptr(act), _ptr(off), _ptr(sc), _ptr(mask), out.ptr(), _stream())
        else:
            copy_ptr = {"null": None, "distinct": cp.ptr(), "alias": _ptr(act)}[variant]
            rc = lib.emloco_task_pd_targets_copy(n, _ptr(act), _ptr(off), _ptr(sc), _ptr(mask), out.ptr(), copy_ptr, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        got, bits = out.got()
        err = TC.judge_pd(c, got[0].cpu())
        print(f"  [pd_targets] n={n} {variant:<8} bar {TC.ULP4:.3e}   device {err:.3e}")
        results.append(bits)
        assert torch.equal(_bits(act), _bits(before)), "actions were written"
        cgot, cbits = cp.got()
        if variant == "distinct":
            assert torch.equal(_bits(cbits[0]), _bits(before)), "the copy is not bit-equal to the actions"
        else:
            assert torch.equal(_bits(cp.buf), _bits(cp.before))
    assert all(torch.equal(_bits(results[0]), _bits(r)) for r in results[1:]), "the four entry variants disagree"


# ---------------------------------------------------------------------------------------------------------------------------------
# amp_rows

def _amp_launch(lib, a, subset, n_sub, out, n=None):
    args = [_padded(a[k]) for k in ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "key_pos", "betas")]
    sub = _dev(torch.tensor(subset, dtype=torch.int32))
    return lib.emloco_task_amp_rows(a["root_pos"].shape[0] if n is None else n, *[_ptr(t) for t in args], _ptr(sub), n_sub, out.ptr(), _stream())


def test_amp_rows_against_float64():
    """The run with a 63-entry subset found that the entry point accepted subsets whose row (35 + 3 n_sub values) does not fit the
    206-value row: 63 entries wrote 224 values per row, 18 of them into the next row and behind the last one.  Subsets above 57 entries
    are refused now."""
    lib = _lib()
    tab, fails = R.Table("task"), []
    for n, seed in TC.AMP_CASES:
        c = R.case_task(n, seed)
        out = _fout(n, AMP_ROW)
        assert _amp_launch(lib, TC.amp_inputs(c), R.DOF_SUBSET, 57, out) == 0
        torch.cuda.synchronize()
        TC.judge_amp_row((n, seed), c, R.DOF_SUBSET, out.got()[0][0].cpu(), tab, fails)
    c = R.case_task(65, 13)
    a = TC.amp_inputs(c)
    out = _fout(65, AMP_ROW)                                   # 3 entries: 44 values per row, the rest of each row stays as it was
    assert _amp_launch(lib, a, R.DOF_SUBSET[:3], 3, out) == 0
    torch.cuda.synchronize()
    got = out.got()[0][0].cpu()
    TC.judge_amp_row((65, 13, "n_sub=3"), c, R.DOF_SUBSET[:3], got, tab, fails)
    assert torch.isnan(got[:, 44:]).all()
    sub63 = tuple(range(63))
    for n_sub in (63, 65, 58):                                 # a row of 35 + 3 n_sub values must fit 206, and joints come in threes
        out = _fout(65, AMP_ROW)
        assert _amp_launch(lib, a, sub63 + (0, 0), n_sub, out) != 0, n_sub
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.buf), _bits(out.before)), "a refused call wrote"
    out = _fout(1, AMP_ROW)
    assert _amp_launch(lib, a, R.DOF_SUBSET, 57, out, n=0) == 0  # n = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.buf), _bits(out.before))
    assert not fails, fails
    tab.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# post_physics

FLOAT_OUT = {"obs": OBS, "flip_obs": OBS, "rew": 1, "reward_raw": 2, "amp": AMP_STEPS * AMP_ROW}
INT_OUT = ("progress", "reset", "terminate")


class Scene:
    """the buffers of one EmlocoTaskBufs, filled by hand: guarded outputs, padded inputs"""

    def __init__(self, c, hf, amp0=None, reset0=None):
        from emloco_amd import _lib as L
        self.c, self.E = c, c["rb_state"].shape[0]
        E = self.E
        self.inp = {k: _padded(c[k]) for k in ("rb_state", "dof_state", "dof_force", "contact_force", "betas", "traj_verts")}
        self.hf = _padded(hf)
        self.l2r = _dev(torch.tensor(R.LEFT_TO_RIGHT, dtype=torch.int32))
        self.mask = _padded(c["contact_body_mask"])
        self.keys = _dev(torch.tensor(R.KEY_BODIES, dtype=torch.int32))
        self.sub = _dev(torch.tensor(R.DOF_SUBSET, dtype=torch.int32))
        self.f = {k: _fout(E, w) for k, w in FLOAT_OUT.items()}
        if amp0 is not None:
            self.f["amp"].fill(torch.as_tensor(amp0).reshape(1, E, -1).to(DEV))
        self.i = {"progress": _GuardedInt(E, fill=c["progress"]), "reset": _GuardedInt(E, fill=reset0), "terminate": _GuardedInt(E)}
        p = lambda t: t.data_ptr()
        self.bufs = L.TaskBufs(E, hf.shape[0], hf.shape[1], R.HEAD_BODY, 57, c["dt"], c["traj_dur"], c["sample_dt"], 0.1, 0.005, c["power_coef"],
                               c["fail_dist"], c["max_episode_length"], p(self.inp["rb_state"]), p(self.inp["dof_state"]), p(self.inp["dof_force"]),
                               p(self.inp["contact_force"]), p(self.inp["betas"]), p(self.inp["traj_verts"]), p(self.hf), p(self.l2r), p(self.mask),
                               p(self.keys), p(self.sub), self.i["progress"].ptr().value, self.i["reset"].ptr().value,
                               self.i["terminate"].ptr().value, *[self.f[k].ptr().value for k in ("obs", "flip_obs", "rew", "reward_raw", "amp")], 0)

    def launch(self, mode, ids=None, n=None):
        d = None if ids is None else _dev(torch.as_tensor(ids, dtype=torch.int32))
        rc = _lib().emloco_task_post_physics(C.byref(self.bufs), int(mode), _ptr(d), 0 if ids is None else (len(ids) if n is None else n), _stream())
        torch.cuda.synchronize()
        return rc

    def state(self):
        """every output as bits ([E][...] int tensors), after the guard bands were checked"""
        s = {k: _bits(o.got()[1][0]).clone() for k, o in self.f.items()}
        s.update({k: o.got() for k, o in self.i.items()})
        return s

    def numpy(self):
        s = {k: o.got()[1][0].cpu().numpy() for k, o in self.f.items()}
        s.update({k: o.got().cpu().numpy() for k, o in self.i.items()})
        s["rew"] = s["rew"].reshape(-1)
        s["amp"] = s["amp"].reshape(self.E, AMP_STEPS, AMP_ROW)
        return s

    def untouched(self):
        return all(torch.equal(_bits(o.buf), _bits(o.before)) for o in self.f.values()) and all(o.untouched() for o in self.i.values())


def _amp0(E, seed):
    return np.random.default_rng(seed).normal(size=(E, AMP_STEPS, AMP_ROW)).astype(np.float32)


def test_post_physics_values_against_float64_and_the_oracle():
    tab, fails = R.Table("task"), []
    hf = R.task_map()
    lib = _lib()
    for E, seed in TC.POST_CASES:
        c = R.case_task(E, seed)
        amp0 = _amp0(E, seed)
        for mode in (POST_STEP, POST_STEP & ~POST_ADVANCE):
            s = Scene(c, hf, amp0)
            assert s.launch(mode) == 0
            TC.judge_post((E, seed, mode), c, hf, mode, amp0, s.numpy(), tab, fails)
            assert all(torch.equal(_bits(v), _bits(_dev(c[k]))) for k, v in s.inp.items()), "an input was written"
        rb = c["rb_state"]
        for grid, pose in ((1, rb[:, R.HEAD_BODY, :7]), (0, rb[:, 0, :7])):
            npt = 1024 if grid else 9
            h, px, py, hfd, pd = _fout(E, npt), _GuardedInt(E * npt), _GuardedInt(E * npt), _padded(hf), _padded(pose.contiguous())
            assert lib.emloco_task_get_heights(_ptr(hfd), hf.shape[0], hf.shape[1], 0.1, 0.005, _ptr(pd), E, grid, h.ptr(), px.ptr(), py.ptr(), _stream()) == 0
            torch.cuda.synchronize()
            got = (h.got()[1][0].cpu().numpy(), px.got().cpu().numpy().reshape(E, npt), py.got().cpu().numpy().reshape(E, npt))
            TC.judge_heights((E, seed), hf.numpy(), pose.numpy(), grid, got, fails)
    assert not fails, fails
    tab.check()


def _algebra_scene(reset0=None, amp_ring=0, amp0=None):
    E, seed = TC.ALGEBRA_CASE
    c = R.case_task(E, seed)
    s = Scene(c, R.task_map(), _amp0(E, seed) if amp0 is None else amp0, reset0)
    s.bufs.amp_ring = amp_ring
    return s


def _entry_flags(E):
    f = torch.zeros(E, dtype=torch.int64)
    f[[1, 7, 8, 30, 64]] = torch.tensor([1, 2, -1, 1 << 40, 1])        # (1 << 40: a flag whose low word is 0)
    return f


def _run(mode, **kw):
    s = _algebra_scene(**kw)
    first = s.state()
    for m in (mode if isinstance(mode, (list, tuple)) else [mode]):
        assert s.launch(m) == 0
    return first, s.state()


OWNER = {POST_ADVANCE: ("progress",), POST_OBS: ("obs", "flip_obs"), POST_REWARD: ("rew", "reward_raw"), POST_RESET: ("reset", "terminate"),
         POST_AMP_SHIFT: ("amp",), POST_AMP_ROW: ("amp",)}


def test_mode_bits_alone_and_combined():
    E = TC.ALGEBRA_CASE[0]
    first, full = _run(POST_STEP)
    for bit, owned in OWNER.items():
        _, st = _run(bit)
        for k in first:
            if k not in owned:
                assert torch.equal(st[k], first[k]), (bit, k, "a buffer the bit does not own changed")
            else:
                assert not torch.equal(st[k], first[k]), (bit, k, "the bit's own buffer did not change")
        amp, amp1 = st["amp"].view(E, AMP_STEPS, AMP_ROW), first["amp"].view(E, AMP_STEPS, AMP_ROW)
        if bit == POST_AMP_SHIFT:                               # a pure copy of rows 0..13 to 1..14; row 0 stays
            assert torch.equal(amp[:, 1:], amp1[:, :-1]) and torch.equal(amp[:, 0], amp1[:, 0])
        if bit == POST_AMP_ROW:
            assert torch.equal(amp[:, 1:], amp1[:, 1:]) and torch.equal(amp[:, 0], full["amp"].view(E, AMP_STEPS, AMP_ROW)[:, 0])
    _, seq = _run([POST_ADVANCE, POST_OBS, POST_REWARD, POST_RESET, POST_AMP_SHIFT, POST_AMP_ROW])
    for k in full:
        assert torch.equal(seq[k], full[k]), (k, "POST_STEP is not ADVANCE followed by the five other bits")


def test_skip_done_and_amp_done_only():
    E = TC.ALGEBRA_CASE[0]
    flags = _entry_flags(E)
    done = flags != 0
    first, full = _run(POST_STEP, reset0=flags)
    _, st = _run(POST_STEP | POST_SKIP_DONE, reset0=flags)
    for k in full:
        assert torch.equal(st[k][done.to(DEV)], first[k][done.to(DEV)]), (k, "SKIP_DONE touched an env whose reset_buf was set")
        assert torch.equal(st[k][~done.to(DEV)], full[k][~done.to(DEV)]), (k, "SKIP_DONE: a live env lacks its POST_STEP bytes")
    # with RESET in the same launch: the envs this launch flags (not those flagged on entry)
    _, st = _run(POST_STEP | POST_AMP_DONE_ONLY, reset0=flags)
    now = full["reset"] != 0
    assert now.any() and not now.all() and not torch.equal(now.cpu(), done)
    for k in full:
        if k != "amp":
            assert torch.equal(st[k], full[k]), (k, "AMP_DONE_ONLY changed something besides the AMP rows")
    assert torch.equal(st["amp"][now], full["amp"][now]) and torch.equal(st["amp"][~now], first["amp"][~now])
    # without RESET: the envs flagged on entry
    _, both = _run(POST_AMP_SHIFT | POST_AMP_ROW, reset0=flags)
    _, st = _run(POST_AMP_SHIFT | POST_AMP_ROW | POST_AMP_DONE_ONLY, reset0=flags)
    d = done.to(DEV)
    assert torch.equal(st["amp"][d], both["amp"][d]) and torch.equal(st["amp"][~d], first["amp"][~d])
    for k in full:
        if k != "amp":
            assert torch.equal(st[k], first[k]), k


def _phys(ring, k):
    return (ring - 1 + k) % AMP_STEPS if ring else k           # EMLOCO_AMP_PHYS_ROW


def test_amp_ring_against_the_layout_run_for_every_head():
    E, seed = TC.ALGEBRA_CASE
    amp0 = _amp0(E, seed)
    _, lay = _run(POST_STEP)
    lay = lay["amp"].view(E, AMP_STEPS, AMP_ROW)
    for h in range(AMP_STEPS):
        ring0 = np.empty_like(amp0)
        for k in range(AMP_STEPS):
            ring0[:, _phys(1 + h, k)] = amp0[:, k]
        h1 = (h + 14) % AMP_STEPS                               # the caller moves the head back by one ahead of the step's launches
        s = _algebra_scene(amp_ring=1 + h1, amp0=ring0)
        first = s.state()
        assert s.launch(POST_AMP_SHIFT) == 0
        assert torch.equal(s.state()["amp"], first["amp"]), "AMP_SHIFT is not a no-op on a ring"
        assert s.launch(POST_STEP) == 0
        got = s.state()["amp"].view(E, AMP_STEPS, AMP_ROW)
        for k in range(AMP_STEPS):
            assert torch.equal(got[:, _phys(1 + h1, k)], lay[:, k]), (h, k)
    # three consecutive steps, the state changing between them
    a, b = _algebra_scene(), _algebra_scene(amp_ring=1 + 4)
    h = 4
    for step in range(3):
        h = (h + 14) % AMP_STEPS
        b.bufs.amp_ring = 1 + h
        for s in (a, b):
            s.inp["dof_state"].mul_(0.9)
            s.inp["rb_state"][:, :, 7:].mul_(1.1)
            assert s.launch(POST_STEP) == 0
        la, rb = a.state()["amp"].view(E, AMP_STEPS, AMP_ROW), b.state()["amp"].view(E, AMP_STEPS, AMP_ROW)
        for k in range(step + 1):                               # (the rows behind them hold each scene's own start values)
            assert torch.equal(rb[:, _phys(1 + h, k)], la[:, k]), (step, k)
    assert not torch.equal(la[:, 0], la[:, 1])


def test_indexed_launches_touch_the_listed_envs_only():
    E = TC.ALGEBRA_CASE[0]
    first, full = _run(POST_STEP)
    g = R._gen(5)
    perm = torch.randperm(E, generator=g)
    short = perm[:20].tolist()
    short[0], short[9], short[19] = -1, -1, -1                  # -1 at the front, in the middle and at the tail
    whole = perm.tolist()
    for pos in (0, 1, 31, 40, E - 1):
        whole[pos] = -1
    for ids in (short, whole):
        s = _algebra_scene()
        assert s.launch(POST_STEP, ids) == 0
        st = s.state()
        listed = torch.zeros(E, dtype=torch.bool)
        listed[[i for i in ids if i >= 0]] = True
        listed = listed.to(DEV)
        for k in full:
            assert torch.equal(st[k][listed], full[k][listed]), (k, "a listed env lacks the full launch's bytes")
            assert torch.equal(st[k][~listed], first[k][~listed]), (k, "an env that is not listed changed")
    s = _algebra_scene()
    assert s.launch(POST_STEP, whole, n=0) == 0 and s.untouched()                    # n = 0: nothing to do
    assert s.launch(POST_STEP, whole + [0], n=E + 1) != 0 and s.untouched()          # n > n_env: refused


# ---------------------------------------------------------------------------------------------------------------------------------
# done-list compaction

@pytest.mark.parametrize("n", TC.COMPACT_SIZES)
def test_compact_done_entry_points(n):
    lib = _lib()
    for pattern in TC.COMPACT_PATTERNS:
        flags = TC.compact_flags_case(n, pattern)
        fd = _padded(flags, garbage=1)                          # (garbage: set flags ahead of and behind the logical n)
        outs = []
        for entry in ("plain", "snapshot", "snapshot_null", "order", "order_null"):
            ids, snap = _GuardedInt(n + 1, torch.int32), _GuardedInt(n)
            sp = None if entry.endswith("null") else snap.ptr()
            if entry == "plain":
                rc = lib.emloco_task_compact_done(_ptr(fd), n, ids.ptr(), _stream())
            elif entry.startswith("snapshot"):
                rc = lib.emloco_task_compact_done_snapshot(_ptr(fd), n, ids.ptr(), sp, _stream())
            else:
                rc = lib.emloco_task_compact_done_order(None, _ptr(fd), n, ids.ptr(), sp, _stream())
            assert rc == 0, (entry, pattern)
            torch.cuda.synchronize()
            got = ids.got().cpu()
            TC.judge_compact(flags, got)
            if entry in ("snapshot", "order"):
                assert torch.equal(snap.got().cpu(), flags), (entry, pattern, "the snapshot is not the flags")
            else:
                assert snap.untouched()
            assert torch.equal(fd.cpu(), flags), "the flags were written"
            outs.append(got)
        assert all(torch.equal(outs[0], o) for o in outs[1:]), (pattern, "the entry points disagree")


# ---------------------------------------------------------------------------------------------------------------------------------
# list-driven reset kernels above 256 entries (grid-stride), and a negative id in the middle of a list

TRAJ_FLAGS = dict(init_heading=True, heading_inversion=True, adjust_root_vel=True)


class TrajScene:
    def __init__(self, golden, N, seed):
        from helpers import traj_reset_bufs
        g = golden("traj_reset_heading")
        gen = R._gen(seed)
        self.N = N
        self.verts, self.inv = _fout(N, 303), torch.full((TAIL + N + TAIL,), 7, dtype=torch.uint8, device=DEV)
        self.inv0 = self.inv.clone()
        self.bufs = traj_reset_bufs(TRAJ_FLAGS, g, self.verts.ptr().value, self.inv.data_ptr() + TAIL, E=N)
        self.rnd = torch.rand(N, 512, generator=gen)
        self.init_pos = torch.cat([torch.rand(N, 2, generator=gen) * 60.0 + 20.0, torch.full((N, 1), 0.9)], dim=1)
        self.root_vel = torch.randn(N, 3, generator=gen)
        self.g = g

    def launch(self, ids, lo=0, hi=None):
        hi = len(ids) if hi is None else hi
        d = [_padded(t[lo:hi].contiguous()) for t in (self.rnd, self.init_pos, self.root_vel)]
        di = _dev(torch.as_tensor(ids[lo:hi], dtype=torch.int32))
        rc = _lib().emloco_task_traj_reset(C.byref(self.bufs), _ptr(di), hi - lo, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _stream())
        torch.cuda.synchronize()
        return rc

    def got(self):
        assert torch.equal(self.inv[:TAIL], self.inv0[:TAIL]) and torch.equal(self.inv[TAIL + self.N:], self.inv0[TAIL + self.N:])
        return _bits(self.verts.got()[1][0]).clone(), self.inv[TAIL:TAIL + self.N].clone()


@pytest.mark.parametrize("n", [257, 700])
def test_traj_reset_in_one_call_equals_calls_of_at_most_256(golden, n):
    from emloco_amd import _lib as L
    from emloco_amd.env.util.traj_generator import TrajGenerator
    from emloco_amd.utils.flags import Flags
    ids = torch.randperm(n, generator=R._gen(n)).tolist()
    one, parts = TrajScene(golden, n, n), TrajScene(golden, n, n)
    assert one.launch(ids) == 0
    for lo in range(0, n, 200):
        assert parts.launch(ids, lo, min(lo + 200, n)) == 0
    (va, ia), (vb, ib) = one.got(), parts.got()
    assert torch.equal(va, vb) and torch.equal(ia, ib), "one call above 256 entries differs from the same entries in calls of <= 256"
    assert (ia <= 1).all(), "an env's inversion flag was not written"
    # the host TrajGenerator on the same draws (the tolerance of test_fused_reset_matches_host_mirror)
    base = dict(real_path=False, jta_path=False, jrdb_path=False, pred_path=False, fixed_path=False, slow=False, adjust_root_vel=False,
                init_heading=False, heading_inversion=False, add_noise=False, vru=False)
    base.update(TRAJ_FLAGS)
    dev = torch.device(DEV)
    tg = TrajGenerator(n, float(one.g["dt_vert"]) * 100.0, 101, dev, 2.0, 0.0005, 3.0, 2.0, 0.02, None, hybridInitProb=0.5, flags=Flags(base))
    by_env = lambda t: torch.empty_like(t).index_copy_(0, torch.tensor(ids), t).to(dev)
    rnd = by_env(one.rnd)
    draws = dict(r_dtheta=rnd[:, L.RND_DTHETA:L.RND_DTHETA + 100], r_dtheta_sharp=rnd[:, L.RND_SHARP:L.RND_SHARP + 100],
                 bern_sharp=(rnd[:, L.RND_BERN:L.RND_BERN + 100] < 0.02).float(), r_heading=rnd[:, L.RND_HEADING],
                 r_dspeed=rnd[:, L.RND_DSPEED:L.RND_DSPEED + 100], r_speed0=rnd[:, L.RND_SPEED0], r_inversion=rnd[:, L.RND_INVERSION])
    tg.reset(torch.arange(n, device=dev), by_env(one.init_pos), by_env(one.root_vel), draws={k: v.clone() for k, v in draws.items()})
    np.testing.assert_allclose(va.view(torch.float32).cpu().numpy().reshape(n, 101, 3), tg._verts.cpu().numpy(), rtol=1e-4, atol=2e-3)
    np.testing.assert_array_equal(ia.cpu().numpy() != 0, tg.inverted.cpu().numpy() != 0)


def test_traj_reset_negative_id_in_the_middle_of_a_long_list(golden):
    """include/emloco_task.h: the env-id-list entry points take lists as emloco_task_compact_done* produces them, negatives only behind
    the last valid id.  A workgroup of a list above 256 entries stops at its first negative id: with -1 at position 3 of 300 entries,
    entry 259 (the same workgroup's next one) is dropped -- its env's rows stay exactly as they were, not half-written -- and every other
    entry gets the bytes of a well-formed call."""
    n = 300
    ids = torch.randperm(n, generator=R._gen(9)).tolist()
    holed = list(ids)
    holed[3] = -1
    a, b = TrajScene(golden, n, 9), TrajScene(golden, n, 9)
    assert a.launch(holed) == 0
    for lo in range(0, n, 200):
        assert b.launch(ids, lo, min(lo + 200, n)) == 0
    (va, ia), (vb, ib) = a.got(), b.got()
    left = torch.zeros(n, dtype=torch.bool)
    left[[ids[3], ids[259]]] = True
    left = left.to(DEV)
    assert torch.equal(va[~left], vb[~left]) and torch.equal(ia[~left], ib[~left])
    nan_bits = _bits(torch.full((1,), float("nan"), device=DEV))
    assert (va[left] == nan_bits).all() and (ia[left] == 7).all(), "a dropped entry's env was written"

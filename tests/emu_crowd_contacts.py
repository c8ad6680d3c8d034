"""CPU execution of emloco_amd/csrc/crowd_contact_kernels.hip through tests/emu/hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY.
tests/emu/emu_crowd_contacts.cpp + tests/emu/emu_runtime.cpp -> tests/emu/_build/libemu_crowd_contacts.so, a library of its own.

`EmuBackend` and `DeviceBackend` (tests/test_gpu_crowd_contacts.py) share `ContactHost`: the audit's buffers as host arrays with guard
words around every one the kernels write, and one method per entry point of include/emloco_task.h."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "_build", "libemu_crowd_contacts.so")
_lib = None
GUARD, FILL = 64, 0xA5A5A5A5
MAXSEG = 32

NOW_DTYPE = np.dtype([("nearest", "<f4"), ("pen", "<f4"), ("nearest_member", "<i4"), ("pen_member", "<i4"), ("pen_segs", "<i4"),
                      ("n_pen", "<i4"), ("n_near", "<i4"), ("flags", "<i4")])
RECORD_DTYPE = np.dtype([("min_nearest", "<f4"), ("mean_nearest", "<f4"), ("max_pen", "<f4"), ("steps", "<i4"), ("nonfinite_steps", "<i4"),
                         ("near_steps", "<i4"), ("contact_steps", "<i4"), ("contacts", "<i4"), ("pen_member", "<i4"), ("pen_segs", "<i4"),
                         ("pen_step", "<i4"), ("first_contact_step", "<i4")])


def build():
    deps = [os.path.join(_HERE, f) for f in ("emu_crowd_contacts.cpp", "emu_runtime.cpp", "hip/hip_runtime.h")]
    deps += [os.path.join(_ROOT, "emloco_amd", "csrc", f) for f in ("crowd_contact_kernels.hip", "dev_math.h")]
    deps += [os.path.join(_ROOT, "include", h) for h in ("emloco_task.h", "emloco_sim.h")]

    def stale():
        return not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        with open(_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = _SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi", "-I", _HERE,
                                       "-o", tmp, os.path.join(_HERE, "emu_crowd_contacts.cpp"), os.path.join(_HERE, "emu_runtime.cpp"), "-lpthread"])
                os.replace(tmp, _SO)
    return _SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp, ci = C.c_void_p, C.c_int
        _lib.emu_crowd_contacts.argtypes, _lib.emu_crowd_contacts.restype = [vp, vp, ci], ci
        _lib.emu_crowd_contacts_accumulate.argtypes, _lib.emu_crowd_contacts_accumulate.restype = [vp, vp], ci
        _lib.emu_crowd_contacts_reduce.argtypes, _lib.emu_crowd_contacts_reduce.restype = [ci, ci, vp, vp, vp], ci
        _lib.emu_crowd_contacts_epoch_reduce.argtypes, _lib.emu_crowd_contacts_epoch_reduce.restype = [ci, vp, vp], ci
        _lib.emu_crowd_contacts_error.restype = C.c_char_p
    return _lib


def guarded(n_words):
    """(whole, view): `view` is n_words zero 32-bit words with GUARD words of FILL on either side inside `whole` (8-byte aligned)"""
    whole = np.full(n_words + 2 * GUARD, FILL, np.uint32)
    view = whole[GUARD:GUARD + n_words]
    view[:] = 0
    assert view.ctypes.data % 8 == 0
    return whole, view


class ContactHost:
    """The audit's buffers on the host.  The subclass gives `ptr(name)` (the address the kernels get for buffer `name`) and the four
    `_call_*`; `sync_in` / `sync_out` move the buffers to and from where the kernels run (nothing to do for the emulator)."""
    WRITTEN = ("caps_ws", "roots_ws", "now", "game_ws", "records", "totals", "moments", "epoch")

    def __init__(self, table, n_env, group_size, near_dist=1.0, games_per_env=0, totals=False, done="done8"):
        from emloco_amd import _lib as L
        self.L = L
        self.E, self.gs, self.near_dist, self.G = n_env, group_size, near_dist, games_per_env
        self.n_seg = int(table["cap_r"].shape[1])
        self.use_totals, self.done_kind = totals, done
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        self.inputs = dict(rb_state=np.zeros((n_env, 24, 13), np.float32), cap_a=f32(table["cap_a"]), cap_b=f32(table["cap_b"]),
                           cap_r=f32(table["cap_r"]), seg_body=np.ascontiguousarray(table["seg_body"], np.uint8),
                           done8=np.zeros(n_env, np.uint8), done64=np.zeros(n_env, np.int64), slot=np.zeros(n_env, np.int32))
        words = dict(caps_ws=n_env * MAXSEG * 8, roots_ws=n_env * 4, now=n_env * 8, game_ws=n_env * L.CROWD_CONTACT_WS,
                     records=n_env * max(games_per_env, 1) * 12, totals=n_env * L.CROWD_CONTACT_TOTALS * 2,
                     moments=L.CROWD_CONTACT_MOMENTS * 2, epoch=L.CROWD_CONTACT_TOTALS * 2)
        self.whole, self.view = {}, {}
        for name in self.WRITTEN:
            self.whole[name], self.view[name] = guarded(words[name])

    def struct(self):
        p = self.ptr
        return self.L.CrowdContacts(self.E, self.gs, self.n_seg, self.G, self.near_dist, 0, p("rb_state"), p("cap_a"), p("cap_b"), p("cap_r"),
                                    p("seg_body"), p("caps_ws"), p("roots_ws"), p("done8") if self.done_kind == "done8" else None,
                                    p("done64") if self.done_kind == "done64" else None, p("slot"), p("game_ws"),
                                    p("records") if self.G > 0 else None, p("totals") if self.use_totals else None)

    # --- the four entry points
    def geometry(self, rb, **kw):
        """now[E] (a copy, NOW_DTYPE) of the state `rb`"""
        np.copyto(self.inputs["rb_state"], np.asarray(rb, np.float32).reshape(self.E, 24, 13))
        self.sync_in()
        self._call_now(self.struct(), **kw)
        self.sync_out()
        return self.now()

    def accumulate(self, done, slot):
        self.inputs["done8"][:] = np.asarray(done) != 0
        self.inputs["done64"][:] = np.asarray(done) != 0
        self.inputs["slot"][:] = slot
        self.sync_in()
        self._call_accumulate(self.struct())
        self.sync_out()

    def reduce(self, games):
        self.inputs["games"] = np.ascontiguousarray(games, np.int32)
        self.sync_in()
        self._call_reduce(self.E, self.G, self.ptr("records"), self.ptr("games"), self.ptr("moments"))
        self.sync_out()
        return self.view["moments"].view(np.float64).copy()

    def epoch_reduce(self):
        self.sync_in()
        self._call_epoch(self.E, self.ptr("totals"), self.ptr("epoch"))
        self.sync_out()
        return self.view["epoch"].view(np.float64).copy()

    # --- views
    def now(self):
        return self.view["now"].view(NOW_DTYPE).copy()

    def records(self):
        return self.view["records"].view(RECORD_DTYPE).reshape(self.E, max(self.G, 1)).copy()

    def totals(self):
        return self.view["totals"].view(np.float64).reshape(self.E, -1).copy()

    def guards(self):
        return all(bool((w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all()) for w in self.whole.values())

    def written_bytes(self):
        return b"".join(self.view[n].tobytes() for n in ("now", "game_ws", "records", "totals"))


class EmuBackend(ContactHost):
    def ptr(self, name):
        return (self.view[name] if name in self.view else self.inputs[name]).ctypes.data

    def sync_in(self):
        pass

    def sync_out(self):
        pass

    def _ok(self, rc):
        assert rc == 0, lib().emu_crowd_contacts_error()

    def _call_now(self, s, grid=0):
        self._ok(lib().emu_crowd_contacts(C.addressof(s), self.ptr("now"), grid))

    def _call_accumulate(self, s):
        self._ok(lib().emu_crowd_contacts_accumulate(C.addressof(s), self.ptr("now")))

    def _call_reduce(self, *a):
        self._ok(lib().emu_crowd_contacts_reduce(*a))

    def _call_epoch(self, *a):
        self._ok(lib().emu_crowd_contacts_epoch_reduce(*a))

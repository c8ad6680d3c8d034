"""The part plan of the rigid-body launch (emloco_sim_set_plan, csrc/sim_plan.h) on the host and on the CPU emulator.

A plan only says which workgroup of the launch runs which substeps of which env, and in which order the workgroups are dispatched;
parts continue from plain copies, so a launch under ANY plan the checker accepts must leave every state buffer and the cost key on the
bytes of the one-part launch.  Three groups: the builder's invariants over a sweep of its parameters (re-derived in numpy,
tests/sim_plan_cases.py); what the builder and the checker refuse; the emulated kernel under plans T, C, S and T+C.  The emulator runs
through a driver of its own (tests/emu/emu_sim_plan.cpp), which hands the kernel a plan as emloco_sim_step does.  The refusals that
need a simulator (not prepared, set_split) are in tests/test_gpu_sim_plan.py: a simulator needs the device."""
import contextlib
import ctypes as C
import fcntl
import functools
import os
import subprocess

import numpy as np
import pytest

import emu
import sim_plan_cases as P
from helpers import bumpy_heightfield, oracle_sim, scene_state, varied_models

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "_build", "libemu_plan.so")


@functools.lru_cache(maxsize=None)
def planlib():
    """g++ over tests/emu/emu_sim_plan.cpp (the rigid-body kernel and the plan driver) and the emulator's runtime, as tests/emu builds"""
    emud, csrc, inc = os.path.join(HERE, "emu"), os.path.join(ROOT, "emloco_amd", "csrc"), os.path.join(ROOT, "include")
    srcs = [os.path.join(emud, s) for s in ("emu_sim_plan.cpp", "emu_runtime.cpp")]
    deps = srcs + [os.path.join(emud, "emu_sim.cpp"), os.path.join(emud, "hip", "hip_runtime.h")]
    deps += [os.path.join(d, f) for d in (csrc, inc) for f in os.listdir(d) if os.path.isfile(os.path.join(d, f))]

    def stale():
        return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps)

    if stale():
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        with open(SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = SO + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-ffp-contract=off", "-Wno-psabi",
                                       "-I", emud, "-o", tmp] + srcs + ["-lpthread"])
                os.replace(tmp, SO)
    lib = C.CDLL(SO)
    lib.emu_sim_plan_error.restype = C.c_char_p
    lib.emu_sim_plan_set.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.emu_sim_plan_words.argtypes = [C.c_void_p, C.c_int]
    lib.emu_sim_plan_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def set_plan(n_env, n_sub, classes, tail, shift):
    """emu_sim_plan_set -> (rc, reason)"""
    lib = planlib()
    c = P.flat(classes) if len(classes) else np.zeros((0, 3), np.int32)
    rc = lib.emu_sim_plan_set(n_env, n_sub, c.ctypes.data, len(c), int(tail), int(shift))
    return rc, lib.emu_sim_plan_error().decode()


def plan_words():
    lib = planlib()
    n = lib.emu_sim_plan_words(None, 0)
    out = np.zeros(n, np.uint32)
    assert lib.emu_sim_plan_words(out.ctypes.data, n) == n
    return out


def check(words, n_env, n_sub):
    w = np.ascontiguousarray(words, np.uint32)
    return planlib().emu_sim_plan_check(w.ctypes.data, len(w), n_env, n_sub)


class _Proxy:
    """the emulator library of tests/emu with its rigid-body step taken from the plan driver"""

    def __init__(self, lib):
        self._lib = lib
        self.emu_sim_step = lib.emu_sim_step_plan

    def __getattr__(self, name):
        return getattr(self._lib, name)


@contextlib.contextmanager
def plan_driver(plan=None, n_env=0):
    """emu.sim_step inside this block launches through tests/emu/emu_sim_plan.cpp, under `plan` = (classes, tail, shift) or none"""
    lib = planlib()
    lib.emu_sim_plan_clear()
    if plan is not None:
        rc, why = set_plan(n_env, P.N_SUB, *plan)
        assert rc == 0, why
    keep = emu._lib
    emu._lib = _Proxy(lib)
    try:
        yield
    finally:
        emu._lib = keep
        lib.emu_sim_plan_clear()


# ------------------------------------------------------------------------------------------------------------ builder invariants
@pytest.mark.parametrize("n_env", [1, 3, 13, 700])
def test_every_plan_the_builder_makes_covers_each_substep_once_and_in_order(n_env):
    seen = set()
    for k in sorted({0, 1, n_env - 1, n_env}):
        for light_parts in (2, 4):
            for tail in (0, 1):
                for shift in (-1, 0, 1):
                    classes = [(0, n_env - k, 4), (n_env - k, n_env, light_parts)]
                    rc, why = set_plan(n_env, P.N_SUB, classes, tail, shift)
                    assert rc == 0, (classes, tail, shift, why)
                    words = plan_words()
                    P.assert_invariants(words, n_env, P.N_SUB, classes, tail)
                    assert check(words, n_env, P.N_SUB) == 0
                    seen.add(words.tobytes())
    assert len(seen) > 1
    # one class, two substeps in two parts or one, and a tail behind a single part
    for parts in (1, 2):
        for tail in (0, 1):
            rc, why = set_plan(n_env, 2, [(0, n_env, parts)], tail, 0)
            assert rc == 0, why
            P.assert_invariants(plan_words(), n_env, 2, [(0, n_env, parts)], tail)


def test_stages_are_dispatched_in_rank_order_and_the_shift_moves_the_light_class():
    """plan T at 3 envs is all first parts, ..., all fourth parts, all tails; under shift +1 the light class's part j stands among
    the heavy class's parts j + 1"""
    assert set_plan(3, 4, [(0, 3, 4)], 1, 0)[0] == 0
    f = P.decode(plan_words())
    assert f["part"].tolist() == [p for p in range(5) for _ in range(3)] and f["rank"].tolist() == [0, 1, 2] * 5
    assert f["n_here"].tolist() == [1] * 12 + [0] * 3 and f["final"].tolist() == [False] * 12 + [True] * 3
    assert set_plan(3, 4, [(0, 2, 4), (2, 3, 4)], 0, 1)[0] == 0
    f = P.decode(plan_words())
    assert list(zip(f["rank"].tolist(), f["part"].tolist())) == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (1, 2), (2, 1), (0, 3), (1, 3),
                                                                 (2, 2), (2, 3)]
    assert set_plan(3, 4, [(0, 2, 4), (2, 3, 2)], 0, 0)[0] == 0                     # C: the light env's two parts of two substeps
    f = P.decode(plan_words())
    light = f["rank"] == 2
    assert f["sub_lo"][light].tolist() == [0, 2] and f["n_here"][light].tolist() == [2, 2] and np.nonzero(light)[0].tolist() == [2, 5]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_the_builder_refuses_bad_parameters_and_keeps_the_plan_in_force():
    assert set_plan(13, 4, [(0, 13, 4)], 1, 0)[0] == 0
    good = plan_words()
    bad = [
        ([(0, 8, 4), (6, 13, 2)], 0, 0, 4, "overlap"),                       # overlapping classes
        ([(5, 13, 4), (0, 5, 2)], 0, 0, 4, ""),                              # descending order of the classes
        ([(0, 8, 4), (13, 8, 2)], 0, 0, 4, "descending"),                    # descending bounds of one class
        ([(0, 5, 4), (7, 13, 2)], 0, 0, 4, "gap"),
        ([(0, 12, 4)], 0, 0, 4, "n_env"),                                    # ranks left over
        ([(0, 14, 4)], 0, 0, 4, "n_env"),
        ([(0, 13, 3)], 0, 0, 4, "divide"),                                   # parts not dividing n_sub
        ([(0, 13, 4)], 0, 0, 2, "divide"),
        ([(0, 13, 0)], 0, 0, 4, "divide"),
        ([(0, 13, 5)], 0, 0, 5, "divide"),                                   # five publishing parts
        ([(0, 13, 4)], 2, 0, 4, "tail"),
        ([(0, 13, 4)], 0, 5, 4, "shift"),
        ([], 0, 0, 4, "classes"),
        ([(0, 13, 1)], 0, 0, 8, "substeps"),                                 # beyond the plan word's 3-bit fields
    ]
    for classes, tail, shift, n_sub, word in bad:
        rc, why = set_plan(13, n_sub, classes, tail, shift)
        assert rc == -1 and why and word in why, (classes, tail, shift, n_sub, why)
        assert np.array_equal(plan_words(), good)
    assert set_plan(0, 4, [(0, 0, 4)], 0, 0)[0] == -1 and set_plan(65537, 4, [(0, 65537, 4)], 0, 0)[0] == -1


def test_the_checker_refuses_plans_that_would_not_compute_the_step_once():
    n_env = 3
    assert set_plan(n_env, 4, [(0, 2, 4), (2, 3, 2)], 1, 0)[0] == 0
    good = plan_words()
    f = P.decode(good)
    assert check(good, n_env, 4) == 0

    def first(rank, part):
        return int(np.nonzero((f["rank"] == rank) & (f["part"] == part))[0][0])

    w = good.copy()
    i, j = first(0, 1), first(0, 2)
    w[[i, j]] = w[[j, i]]
    assert check(w, n_env, 4) == -1                                          # a consumer ahead of its producer in index order
    assert check(np.delete(good, first(1, 2)), n_env, 4) == -1               # a substep covered by nobody
    assert check(np.insert(good, first(1, 2), good[first(1, 2)]), n_env, 4) == -1      # a substep covered twice
    assert check(np.delete(good, first(2, 2)), n_env, 4) == -1               # a rank without its final workgroup
    assert check(np.append(good, good[first(2, 2)]), n_env, 4) == -1         # two final workgroups
    for bit in (25, 26, 27):                                                 # publishes / consumes / final flipped anywhere
        for i in range(len(good)):
            w = good.copy()
            w[i] ^= np.uint32(1 << bit)
            assert check(w, n_env, 4) == -1, (bit, i)
    w = good.copy()
    w[first(0, 0)] |= np.uint32(7)                                           # a rank beyond n_env
    assert check(w, n_env, 4) == -1
    w = good.copy()
    w[3] |= np.uint32(1 << 28)
    assert check(w, n_env, 4) == -1
    # five publishing parts: five one-substep parts and a tail
    five = [r | p << 16 | p << 19 | 1 << 22 | 1 << 25 | (1 << 26 if p else 0) for p in range(5) for r in range(1)] + [5 << 16 | 5 << 19 | 1 << 26 | 1 << 27]
    assert check(np.array(five, np.uint32), 1, 5) == -1
    assert check(good[:0], n_env, 4) == -1


# ------------------------------------------------------------------------------------------------------------ emulated kernel
STEPS = 2


@functools.lru_cache(maxsize=None)
def _scene(n_env, ground):
    models = varied_models(n_env, seed=31)
    root, dof, tgt = scene_state(n_env, seed=32)
    hf = bumpy_heightfield() if ground == "hf" else None
    return lambda: oracle_sim(models, root, dof, tgt, self_collision=True, heightfield=hf, n_sub=P.N_SUB)


def _run(make, n_env, plan, ordered):
    """two steps back to back; -> the six state buffers and the cost key after each step"""
    b = make()
    out = []
    keys = np.zeros(n_env, np.uint32)
    order = np.arange(n_env, dtype=np.int32)[::-1].copy() if ordered else None
    with plan_driver(plan, n_env):
        for _ in range(STEPS):
            emu.sim_step(b, 1, parts=1 if plan is None else 4, cost_ticks=keys, order=order)
            out.append({n: getattr(b, n).copy() for n in P.NAMES} | {"step_ticks": keys.copy()})
            if ordered:
                order = np.argsort(-keys.astype(np.int64), kind="stable").astype(np.int32)       # most contact work first, as sim_order_kernel
    return out


@functools.lru_cache(maxsize=None)
def _reference(n_env, ground, ordered):
    """the one-part launch, computed once per scene and shared by the plans (read only)"""
    ref = _run(_scene(n_env, ground), n_env, None, ordered)
    assert np.abs(ref[-1]["contact_force"]).max() > 0 or n_env == 1
    assert ref[-1]["step_ticks"].max() > 0 or n_env == 1
    for step in ref:
        for v in step.values():
            v.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", ["T", "C", "S", "T+C"])
@pytest.mark.parametrize("ordered", [False, True], ids=["rank_is_env", "cost_order"])
@pytest.mark.parametrize("ground", ["plane", "hf"])
@pytest.mark.parametrize("n_env", [1, 3, 13])
def test_the_emulated_kernel_under_a_plan_is_the_one_part_launch(n_env, ground, ordered, name):
    ref = _reference(n_env, ground, ordered)
    got = _run(_scene(n_env, ground), n_env, P.plans(n_env)[name], ordered)
    for t in range(STEPS):
        for k, v in ref[t].items():
            assert np.array_equal(v, got[t][k]), (name, t, k)


def test_a_lost_hand_over_under_plan_t_raises_the_error_word_and_abandons_that_env_alone(monkeypatch):
    n_env = 3
    make = _scene(n_env, "plane")
    a, b = make(), make()
    a.step(1)
    with plan_driver(P.plans(n_env)["T"], n_env):
        emu.sim_step(b, 1, parts=4)
        before = {n: getattr(b, n).copy() for n in P.NAMES}
        for n in P.NAMES:
            assert np.array_equal(getattr(a, n), before[n]), n                # plan T on the oracle's bytes
        monkeypatch.setenv("EMLOCO_EMU_POISON", "1")
        a.step(1)
        assert emu.sim_step(b, 1, parts=4, expect_error=True) == 1             # EMLOCO_ERR_PART_TIMEOUT
    for n in P.NAMES:
        x, y = getattr(a, n).reshape(n_env, -1), getattr(b, n).reshape(n_env, -1)
        assert np.array_equal(x[[0, 2]], y[[0, 2]]), n                         # the others untouched by it
        assert np.array_equal(y[1], before[n].reshape(n_env, -1)[1]), n        # the poisoned env: abandoned in every buffer

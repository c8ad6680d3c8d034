"""CPU-only: the crowd spawn (include/emloco_task.h: EmlocoCrowdSpawn) -- the kernels of emloco_amd/csrc/crowd_spawn_kernels.hip on the
emulator against the numpy float32 restatement of the rule (tests/crowd_spawn_cases.py), bit for bit: positions, clearance2, tried,
flags and order; after every case mark_ws is -1 again, the guard words are intact and the rows of unlisted envs hold the prefill.
Then the refusals of the entry point, of the configuration and of run.py's flags."""
import ctypes as C
import math

import numpy as np
import pytest

import crowd_spawn_cases as SC
import emu_crowd_spawn as ES


@pytest.fixture(scope="module")
def results():
    """every case run once on the emulator: {name: (case, host, place, info)}"""
    out = {}
    for name, make in SC.CASES.items():
        case = make()
        host = ES.EmuBackend(case).run()
        out[name] = (case, host, *SC.spawn_f32(case))
    return out


@pytest.mark.parametrize("name", list(SC.CASES))
def test_emulator_equals_the_restatement(results, name):
    ES.check_against_restatement(results[name][1])


def check_case_properties(name, case, place, info):
    """what each case is there to show, read off the restatement's result (which the outputs equal bit for bit)"""
    flags = {e: v[2] for e, v in info.items()}
    if name == "small_extent":
        for g in (0, 1):
            members = [e for e in info if e // 6 == g]
            assert [info[e][3] for e in members] == list(range(6)), "order: the rank among the group's placements"
            assert any(flags[e] & SC.CROWDED for e in members), "a crowded fallback in either group"
            assert info[members[0]][0] == np.inf and info[members[0]][1] == 0
    elif name == "padded_list":
        assert sorted(info) == [70, 71, 75, 88, 101, 120, 139] and [info[e][3] for e in sorted(info)] == list(range(7))
        # env 75 is listed at positions 2 and 6: the uniforms of position 2 count
        other = dict(case, u=case["u"].copy())
        other["u"][6] = 0.5
        assert SC.spawn_f32(other)[0][75] == place[75]
        other["u"][2] = 0.5
        assert SC.spawn_f32(other)[0][75] != place[75]
    elif name == "same_call":
        assert (case["u"][0] == case["u"][1]).all() and place[2] != place[5]
        assert info[2][1] == 0 and info[5][1] > 0, "the second finds candidate 0 taken by the first"
    elif name == "threshold":
        md2 = np.float32(case["min_dist"]) * np.float32(case["min_dist"])
        assert info[0][0] == md2 == np.float32(1.5625) and info[0][1] == 0 and flags[0] == 0, "clearance2 == min_dist^2 is accepted"
    elif name == "fallback_tie":
        assert info[0] == (np.float32(0.25), 0, SC.CROWDED, 0) and place[0] == (np.float32(20.5), np.float32(20.0))
    elif name == "ground":
        assert info[1][1] == -1 and flags[1] & SC.NO_GROUND and place[1] == (np.float32(20.0), np.float32(20.0))
        assert not any(flags[e] & SC.NO_GROUND for e in info if e != 1)
        f32 = np.float32
        cand = lambda row, k, g: tuple(case["centres"][g] + case["extent"] * (f32(2) * case["u"][row, k] - f32(1)))
        assert [SC.admissible(case, *cand(1, k, 0)) for k in range(4)] == [False] * 4
        x, y = cand(3, 0, 1)                                       # env 4's candidate 0: inside the box, its cell row outside the field
        assert case["min_x"] <= x <= case["max_x"] and case["min_y"] <= y <= case["max_y"] and int(x / f32(case["hscale"])) >= 400
        assert not SC.admissible(case, x, y) and info[4][1] > 0
        assert any(not SC.admissible(case, *cand(r, k, g)) for r, g in ((0, 0), (2, 0)) for k in range(4)), "some candidates are inadmissible"
    elif name == "non_finite":
        assert info[5] [0] == np.inf and info[5][1] == 0 and info[5][3] == 0, "nobody stands: +inf, candidate 0"
        assert info[0][0] == np.inf, "group 0: members 1 (NaN) and 2 (inf) are skipped, 3 is listed and not yet placed"
        assert all(np.isfinite(info[e][0]) for e in (3, 6, 7))
    elif name == "shipped":
        n_crowded = sum(1 for e in info if flags[e] & SC.CROWDED)
        assert len(info) == 512 and n_crowded <= 1 and not any(flags[e] & SC.NO_GROUND for e in info)
        xy = np.asarray([place[e] for e in sorted(place)], np.float64)
        d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1)) + 1e9 * np.eye(512)
        assert n_crowded > 0 or d.min() >= 1.0 - 1e-6


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_shows_what_it_is_there_for(results, name):
    case, _, place, info = results[name]
    check_case_properties(name, case, place, info)


def test_two_runs_give_the_same_bytes_and_parallel_placement_would_not():
    case = SC.case_same_call()
    a, b = ES.EmuBackend(case).run(), ES.EmuBackend(case).run()
    assert a.written_bytes() == b.written_bytes()
    # placing the two members independently (each against the roots before the call) puts both on one spot: the rule forbids it
    alone = [SC.spawn_f32(case, ids=[e], u=case["u"][:1])[0][e] for e in (2, 5)]
    assert alone[0] == alone[1]


# ------------------------------------------------------------------ refusals of the entry point
def refusal_edits():
    """(structure edits, n, with u, with ids, the name the refusal carries)"""
    nan, inf = float("nan"), float("inf")
    P = ("roots", "walkable", "centres", "mark_ws", "place_xy", "info")
    return ([(dict([(p, None)]), 0, True, False, "null " + p) for p in P] +
            [(dict(group_size=0), 0, True, False, "group_size < 1"), (dict(group_size=5), 0, True, False, "multiple of group_size"),
             (dict(group_size=4096, n_env=4096), 0, True, False, "group_size > 2048"),
             (dict(n_env=0), 0, True, False, "multiple of group_size"), (dict(tries=0), 0, True, False, "tries outside 1..8"),
             (dict(tries=9), 0, True, False, "tries outside 1..8"), (dict(root_stride=1), 0, True, False, "root_stride < 2"),
             (dict(rows=0), 0, True, False, "rows < 1"), (dict(cols=-1), 0, True, False, "cols < 1"), (dict(hscale=0.0), 0, True, False, "hscale"),
             (dict(hscale=nan), 0, True, False, "hscale"), (dict(extent=0.0), 0, True, False, "extent"), (dict(extent=inf), 0, True, False, "extent"),
             (dict(extent=nan), 0, True, False, "extent"), (dict(min_dist=-1.0), 0, True, False, "min_dist"), (dict(min_dist=inf), 0, True, False, "min_dist"),
             (dict(min_x=30.0, max_x=20.0), 0, True, False, "empty box: min_x"), (dict(min_y=nan), 0, True, False, "empty box: min_y"),
             (dict(), -1, True, True, "n < 0"), (dict(), 3, False, True, "null u"), (dict(), 0, False, False, "null u")])


def test_emulated_entry_point_refuses_by_name():
    case = SC.case_ground()
    h = ES.EmuBackend(case)
    before = h.written_bytes()
    lib = ES.lib()
    assert lib.emu_crowd_spawn(None, None, 0, None) == -1 and lib.emu_crowd_spawn_error() == b"null structure"
    for edits, n, with_u, with_ids, name in refusal_edits():
        s = h.struct(**edits)
        rc = lib.emu_crowd_spawn(C.addressof(s), h.ptr("ids") if with_ids else None, n, h.ptr("u") if with_u else None)
        assert rc == -1 and name in lib.emu_crowd_spawn_error().decode(), (edits, lib.emu_crowd_spawn_error())
    # n == 0 with a list: 0, nothing launched, u may be NULL
    s = h.struct()
    assert lib.emu_crowd_spawn(C.addressof(s), h.ptr("ids"), 0, None) == 0
    assert h.written_bytes() == before and h.guards()


def test_binding_and_mirrors():
    from emloco_amd import _abi, _lib as L
    assert _abi.prototypes()["emloco_task_crowd_spawn"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    assert C.sizeof(L.CrowdSpawnInfo) == 16 == SC.INFO.itemsize and C.sizeof(L.CrowdSpawn) == 56 + 6 * 8
    assert (L.SPAWN_CROWDED, L.SPAWN_NO_GROUND) == (SC.CROWDED, SC.NO_GROUND)
    assert hasattr(L.load(), "emloco_task_crowd_spawn")


# ------------------------------------------------------------------ the configuration
def test_config_block_and_auto_extent():
    from emloco_amd import crowd_spawn as S
    assert S.config_block({}) == dict(on=False, min_dist=1.0, tries=8, extent="auto", centre=None, margin=10.0)
    b = S.config_block(dict(group_spawn=True, group_spawn_min_dist=0.75, group_spawn_tries=4, group_spawn_extent=8, group_spawn_centre=[50, 55],
                            group_spawn_margin=2))
    assert b == dict(on=True, min_dist=0.75, tries=4, extent=8, centre=[50, 55], margin=2)
    assert abs(S.auto_extent(512, 1.0) - 25.298) < 1e-3 and abs(S.auto_extent(16, 1.0) - 4.472) < 1e-3
    assert S.auto_extent(512, 1.0) == 0.5 * math.sqrt(512 / 0.2) == SC.auto_extent(512, 1.0)
    r = S.resolve(S.config_block(dict(group_spawn=True)), 16, 120.0, 140.0)
    assert r["centre"] == (60.0, 70.0) and r["extent"] == S.auto_extent(16, 1.0)


def test_config_refusals_name_the_key():
    from emloco_amd.crowd_spawn import spawn_refusal
    on = dict(group_spawn=True, divide_group=True, num_env_group=16)
    walk = np.zeros((1200, 1200), np.int16)
    assert spawn_refusal({}) is None and spawn_refusal(dict(group_spawn=False)) is None
    assert spawn_refusal(on) is None and spawn_refusal(on, 16, (120.0, 120.0), walk, 0.1) is None
    assert "divide_group" in spawn_refusal(dict(group_spawn=True)) and spawn_refusal(dict(group_spawn=True)).startswith("group_spawn:")
    for key, bad in (("group_spawn_min_dist", -1), ("group_spawn_min_dist", float("nan")), ("group_spawn_min_dist", "far"),
                     ("group_spawn_tries", 0), ("group_spawn_tries", 9), ("group_spawn_tries", 2.5), ("group_spawn_extent", 0),
                     ("group_spawn_extent", "wide"), ("group_spawn_extent", float("inf")), ("group_spawn_margin", -1),
                     ("group_spawn_centre", [1, 2, 3]), ("group_spawn_centre", "middle")):
        assert spawn_refusal(dict(on, **{key: bad})).startswith(key + ":"), (key, bad)
    # a square plus margin that leaves the field
    assert spawn_refusal(dict(on, group_spawn_extent=51), 16, (120.0, 120.0)).startswith("group_spawn_extent:")
    assert spawn_refusal(dict(on, group_spawn_extent=50), 16, (120.0, 120.0)) is None
    assert "leaves the" in spawn_refusal(dict(on, group_spawn_centre=[12, 60]), 16, (120.0, 120.0))
    assert "leaves the" in spawn_refusal(on, 2048, (120.0, 120.0))                 # auto extent 50.6 m
    assert "at most 2048" in spawn_refusal(on, 4096, (1200.0, 1200.0))
    # a centre that is not admissible
    walk[600, 600] = 1
    assert spawn_refusal(on, 16, (120.0, 120.0), walk, 0.1).startswith("group_spawn_centre:")
    assert spawn_refusal(dict(on, group_spawn_centre=[60.5, 60]), 16, (120.0, 120.0), walk, 0.1) is None


# ------------------------------------------------------------------ run.py's flags
def test_run_flags_are_parsed_and_refused_by_name(monkeypatch):
    from emloco_amd import run
    monkeypatch.delenv("EMLOCO_OVERLAP_RESET", raising=False)
    argv = ["--test", "--group_spawn", "--group_spawn_min_dist", "0.75", "--num_envs", "64", "--group_spawn_extent", "auto", "--group_spawn_tries", "4"]
    assert run.pop_spawn_options(argv) == dict(group_spawn=True, group_spawn_min_dist=0.75, group_spawn_extent="auto", group_spawn_tries=4)
    assert argv == ["--test", "--num_envs", "64"]
    assert run.pop_spawn_options(["--group_spawn", "--group_spawn_extent", "8"]) == dict(group_spawn=True, group_spawn_extent=8.0)
    assert run.pop_spawn_options(["--num_envs", "64"]) is None
    for sub in ("--group_spawn_min_dist", "--group_spawn_extent", "--group_spawn_tries"):
        with pytest.raises(SystemExit, match=f"{sub}.*--group_spawn"):
            run.pop_spawn_options([sub, "1"])
    with pytest.raises(SystemExit, match="--group_spawn_tries"):
        run.pop_spawn_options(["--group_spawn", "--group_spawn_tries", "many"])
    with pytest.raises(SystemExit, match="--group_spawn_extent"):
        run.pop_spawn_options(["--group_spawn", "--group_spawn_extent", "wide"])
    monkeypatch.setenv("EMLOCO_OVERLAP_RESET", "1")
    with pytest.raises(SystemExit, match="--group_spawn.*EMLOCO_OVERLAP_RESET"):
        run.pop_spawn_options(["--group_spawn"])
    monkeypatch.delenv("EMLOCO_OVERLAP_RESET")
    # on a configuration without divide_group, and with a bad number: refused by name before any device call
    with pytest.raises(SystemExit, match="--group_spawn.*divide_group"):
        run.apply_spawn_options(dict(group_spawn=True), dict(numEnvs=64))
    with pytest.raises(SystemExit, match="--group_spawn.*group_spawn_tries"):
        run.apply_spawn_options(dict(group_spawn=True, group_spawn_tries=12), dict(numEnvs=64, divide_group=True))
    env_cfg = dict(numEnvs=64, divide_group=True, num_env_group=16)
    run.apply_spawn_options(dict(group_spawn=True, group_spawn_min_dist=0.75), env_cfg)
    assert env_cfg["group_spawn"] is True and env_cfg["group_spawn_min_dist"] == 0.75
    untouched = dict(numEnvs=64)
    run.apply_spawn_options(None, untouched)
    assert untouched == dict(numEnvs=64)


def test_run_refuses_group_spawn_without_groups_before_the_device():
    from emloco_amd import run
    with pytest.raises(SystemExit, match="--group_spawn.*divide_group"):
        run.main(["--num_envs", "32", "--seed", "1", "--group_spawn"])               # pacer.yaml has no groups

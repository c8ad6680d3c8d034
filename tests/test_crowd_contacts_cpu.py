"""CPU-only: the crowd contact audit's kernels (emloco_amd/csrc/crowd_contact_kernels.hip) on the emulator against the float64
restatement of tests/crowd_contact_cases.py (bounds and case conditions: that module's docstring), the bookkeeping and both reductions
against numpy run on the emulator's own now[], the refusals of the C ABI through emloco_last_error, and the refusals of run.py and of
the Python classes with no device touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import crowd_contact_cases as K
import emu_crowd_contacts as M
from emloco_amd import _abi, _lib as L, crowd_contacts as CC


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_against_restatement(name):
    c = K.CASES[name]()
    h = M.EmuBackend(c["table"], c["E"], c["gs"], c["near_dist"])
    again = M.EmuBackend(c["table"], c["E"], c["gs"], c["near_dist"])
    for t in range(len(c["rb"])):
        got = h.geometry(c["rb"][t])
        K.check_now(got, c["now"][t], f"{name}[{t}]")
        assert got.tobytes() == again.geometry(c["rb"][t], grid=3).tobytes()          # another launch shape, a fresh workspace: the same bytes
    assert h.guards() and again.guards()


def test_spheres_by_hand():
    c = K.spheres()
    now = M.EmuBackend(c["table"], c["E"], c["gs"], c["near_dist"]).geometry(c["rb"][0])
    rs = np.float32(0.1) + np.float32(0.1)
    # env 0 between 1 and 2, mirrored: the same distance and penetration to both, the lowest index wins; all 24 (i, i) pairs tie: (0, 0)
    assert tuple(now[0]) == (np.float32(0.125), rs - np.float32(0.125), 1, 1, 0, 2, 2, 0)
    assert now[1]["pen_member"] == 0 and now[1]["n_pen"] == 1 and now[1]["n_near"] == 2           # 1 and 2 are 0.25 apart: no contact
    # env 3 and env 4 share a spot but not a group
    assert now[3]["n_pen"] == 0 and now[3]["nearest_member"] == 1 and now[3]["nearest"] == np.float32(9.875)
    assert now[4]["n_pen"] == 0 and now[4]["nearest_member"] == 7 and now[4]["n_near"] == 1
    # NaN position, Inf quaternion: flagged themselves, skipped by the others
    for e in (5, 6, 9, 10, 11):
        assert tuple(now[e]) == (0.0, 0.0, -1, -1, -1, 0, 0, 1)
    assert now[7]["nearest_member"] == 4
    assert tuple(now[8]) == (0.0, 0.0, -1, -1, -1, 0, 0, 0)                                      # everybody else in its group is non-finite


def run_people(backend, done="done8"):
    """the scripted games of the `people` case on a back end: (host, [now per step], moments, epoch vector)"""
    c = K.people()
    h = backend(c["table"], c["E"], c["gs"], c["near_dist"], games_per_env=c["G"], totals=True, done=done)
    nows = []
    for t in range(len(c["rb"])):
        nows.append(h.geometry(c["rb"][t]))
        h.accumulate(c["done"][t], c["slot"][t])
    rec, tot = h.records(), h.totals()
    moments = h.reduce(c["games"])
    epoch = h.epoch_reduce()
    return types.SimpleNamespace(c=c, h=h, nows=nows, rec=rec, tot=tot, moments=moments, epoch=epoch)


@pytest.fixture(scope="module")
def people_run():
    return run_people(M.EmuBackend)


def test_bookkeeping_against_numpy(people_run):
    r, c = people_run, people_run.c
    rec, written, tot = K.restate_books(r.nows, c["done"], c["slot"], c["G"])
    assert written.sum() == c["games"].sum() and (written.sum(axis=1) == c["games"]).all()
    assert r.rec[written].tobytes() == rec[written].tobytes()                 # integers, min / max and the double division: the same bytes
    assert not r.rec[~written].tobytes().strip(b"\0")                         # a game still running, an env past its quota: zero bytes
    assert np.array_equal(r.tot, tot)
    assert r.h.guards()
    # what the script sets up
    assert r.rec[2, 0]["steps"] == 1 and r.rec[2, 1]["steps"] == 1            # a game that ends at its first step
    assert (r.rec[0, 0]["first_contact_step"], r.rec[1, 0]["first_contact_step"]) == (1, 1)      # games that start in contact
    assert r.rec[3, 0]["contact_steps"] == 0 and r.rec[3, 0]["pen_member"] == -1 and r.rec[3, 0]["max_pen"] == 0      # never touches
    assert c["slot"][-1][1] >= c["G"] and written[1].all()                    # env 1 played on after its quota
    assert r.rec[6, 1]["nonfinite_steps"] == 1 and r.rec[6, 0]["nonfinite_steps"] == 2 and r.rec[6, 0]["steps"] == 10
    assert (r.rec[written]["steps"] + r.rec[written]["nonfinite_steps"] > 0).all()
    same_group = r.rec[written]["pen_member"] // c["gs"] == np.nonzero(written)[0] // c["gs"]
    assert (same_group | (r.rec[written]["pen_member"] == -1)).all()


def test_reductions_against_numpy(people_run):
    r, c = people_run, people_run.c
    want = K.restate_moments(r.rec, c["games"])
    np.testing.assert_allclose(r.moments, want, rtol=1e-12, atol=0)
    assert r.moments[L.CCM_GAMES] == c["games"].sum() and r.moments[L.CCM_GAMES_CONTACT] > 0
    # the host-side restatement of the product on the gathered records
    env, game = np.nonzero(np.arange(c["G"])[None, :] < c["games"][:, None])
    np.testing.assert_allclose(CC.moments_from_records(r.rec[env, game]), r.moments, rtol=1e-12, atol=0)
    ep = K.restate_epoch(r.tot)
    np.testing.assert_allclose(r.epoch, ep, rtol=1e-12, atol=0)
    assert r.epoch[L.CCT_MAX_PEN] == r.tot[:, L.CCT_MAX_PEN].max() and r.epoch[L.CCT_STEPS] + r.epoch[L.CCT_NONFINITE_STEPS] == 40 * c["E"]
    assert not r.h.totals().any()                                             # the epoch reduction clears what it has read
    blk = CC.crowd_from_moments(r.moments, 1.0, c["gs"])
    assert blk["games"] == c["games"].sum() and 0 < blk["contact_game_share"] < 1 and len(blk["lines"]) == 3 and blk["near_dist"] == 1.0
    assert CC.crowd_from_moments(np.zeros(L.CROWD_CONTACT_MOMENTS))["lines"] == ["crowd: no game finished"]
    extra = CC.crowd_from_records([np.arange(len(env), dtype=np.float32), np.ones(len(env), np.float32)], r.rec[env, game])
    assert extra["max_pen"] == r.rec["max_pen"].max() and np.isfinite(extra["corr_value_max_pen"][0]) and np.isnan(extra["corr_value_contact"][1])
    e = CC.epoch_from_totals(r.epoch, 1.0, c["gs"])
    assert e["steps"] == int(r.epoch[0]) and 0 < e["contact_step_share"] < 1 and "crowd contact" in CC.epoch_tail(e)


def test_done64_and_two_runs_give_the_same_bytes(people_run):
    other = run_people(M.EmuBackend, done="done64")
    assert other.h.written_bytes() == people_run.h.written_bytes()
    assert other.moments.tobytes() == people_run.moments.tobytes() and other.epoch.tobytes() == people_run.epoch.tobytes()


# ------------------------------------------------------------------------------------------------------------ the C ABI's refusals
def good_struct():
    E = 8
    keep = [np.zeros(E * 32 * 8, np.float32) for _ in range(3)] + [np.zeros(E * 32, np.uint8), np.zeros(E * 16, np.int64)]
    p = [k.ctypes.data for k in keep]
    s = L.CrowdContacts(E, 4, 26, 2, 1.0, 0, p[0], p[0], p[0], p[0], p[3], p[1], p[2], p[3], None, p[4], p[4], p[4], p[4])
    return s, keep


GEOMETRY_REFUSALS = [("n_env", 0, "n_env"), ("group_size", 1, "group_size < 2"), ("group_size", 3, "does not divide"), ("n_seg", 23, "n_seg"),
                     ("n_seg", 33, "n_seg"), ("near_dist", 0.0, "near_dist"), ("near_dist", float("inf"), "near_dist"),
                     ("near_dist", float("nan"), "near_dist"), ("rb_state", None, "rb_state"), ("cap_a", None, "cap_a"), ("cap_b", None, "cap_b"),
                     ("cap_r", None, "cap_r"), ("seg_body", None, "seg_body"), ("caps_ws", None, "caps_ws"), ("roots_ws", None, "roots_ws")]
ACCUMULATE_REFUSALS = [("n_env", 0, "n_env"), ("game_ws", None, "game_ws"), ("done64", "keep", "both"), ("slot", None, "records without slot"),
                       ("games_per_env", 0, "games_per_env")]


@pytest.mark.parametrize("field,value,word", GEOMETRY_REFUSALS)
def test_geometry_refusals(field, value, word, capfd):
    lib = L.load()
    s, keep = good_struct()
    setattr(s, field, value)
    rc = lib.emloco_crowd_contacts(C.byref(s), keep[4].ctypes.data, None)
    msg = lib.emloco_last_error().decode()
    assert rc == -1 and msg.startswith("emloco_crowd_contacts: ") and word in msg
    with pytest.raises(L.EmlocoError, match="emloco_crowd_contacts"):
        L.check(rc, "emloco_crowd_contacts")
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


@pytest.mark.parametrize("field,value,word", ACCUMULATE_REFUSALS)
def test_accumulate_refusals(field, value, word):
    lib = L.load()
    s, keep = good_struct()
    setattr(s, field, keep[4].ctypes.data if value == "keep" else value)
    rc = lib.emloco_crowd_contacts_accumulate(C.byref(s), keep[4].ctypes.data, None)
    msg = lib.emloco_last_error().decode()
    assert rc == -1 and msg.startswith("emloco_crowd_contacts_accumulate: ") and word in msg


def test_null_and_reduction_refusals():
    lib = L.load()
    s, keep = good_struct()
    p = keep[4].ctypes.data
    err = lambda: lib.emloco_last_error().decode()
    assert lib.emloco_crowd_contacts(None, p, None) == -1 and "null structure" in err()
    assert lib.emloco_crowd_contacts(C.byref(s), None, None) == -1 and "null now" in err()
    assert lib.emloco_crowd_contacts_accumulate(None, p, None) == -1 and "null structure" in err()
    assert lib.emloco_crowd_contacts_accumulate(C.byref(s), None, None) == -1 and "null now" in err()
    for args, word in (((0, 2, p, p, p), "n_env"), ((8, 0, p, p, p), "games_per_env"), ((8, 2, None, p, p), "records"),
                       ((8, 2, p, None, p), "games"), ((8, 2, p, p, None), "moments")):
        assert lib.emloco_crowd_contacts_reduce(*args, None) == -1 and err().startswith("emloco_crowd_contacts_reduce: ") and word in err()
    for args, word in (((0, p, p), "n_env"), ((8, None, p), "totals"), ((8, p, None), "epoch")):
        assert lib.emloco_crowd_contacts_epoch_reduce(*args, None) == -1 and err().startswith("emloco_crowd_contacts_epoch_reduce: ") and word in err()


def _header_fields(name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^{}]*)\}\s*%s\s*;" % (name, name), _abi.source("emloco_task.h"))
    fields = []
    scalars = dict(_abi.SCALARS, uint8_t=C.c_uint8)
    for decl in filter(str.strip, m.group(1).split(";")):
        first, *more = decl.replace("*", " * ").split(",")
        base, *first = [w for w in first.split() if w != "const"]
        for d in [first] + [x.split() for x in more]:
            assert len(d) == 1 + ("*" in d) and re.fullmatch(r"\w+", d[-1]), decl
            fields.append((d[-1], "ptr" if "*" in d else scalars[base]))
    return fields


def test_mirrors_follow_the_header(tmp_path):
    pairs = (("EmlocoCrowdContactNow", L.CrowdContactNow), ("EmlocoCrowdContactRecord", L.CrowdContactRecord), ("EmlocoCrowdContacts", L.CrowdContacts))
    for name, mirror in pairs:
        assert [(f, "ptr" if t is C.c_void_p else t) for f, t in mirror._fields_] == _header_fields(name), name
    for dt, mirror in ((CC.NOW_DTYPE, L.CrowdContactNow), (CC.RECORD_DTYPE, L.CrowdContactRecord), (M.NOW_DTYPE, L.CrowdContactNow),
                       (M.RECORD_DTYPE, L.CrowdContactRecord)):
        assert dt.itemsize == C.sizeof(mirror) and list(dt.names) == [f for f, _ in mirror._fields_]
        assert [dt.fields[f][1] for f in dt.names] == [getattr(mirror, f).offset for f in dt.names]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc to ask for sizeof")
    (tmp_path / "size.c").write_text('#include "emloco_task.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", '
                                     'sizeof(EmlocoCrowdContactNow), sizeof(EmlocoCrowdContactRecord), sizeof(EmlocoCrowdContacts)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "size"), str(tmp_path / "size.c")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "size")], text=True).split()] == [32, 48, C.sizeof(L.CrowdContacts)]


# ------------------------------------------------------------------------------------------------------------ Python and run.py refusals
def test_python_refusals_touch_no_device():
    no_groups = types.SimpleNamespace(_divide_group=False, num_envs=8, device="cpu")
    with pytest.raises(CC.CrowdContactRefusal, match="divide_group"):
        CC.CrowdContactAudit(no_groups)
    no_table = types.SimpleNamespace(_divide_group=True, _group_num_people=4, num_envs=8, device="cpu",
                                     sim=types.SimpleNamespace(native=types.SimpleNamespace()))
    with pytest.raises(CC.CrowdContactRefusal, match="self-collision"):
        CC.CrowdContactAudit(no_table)
    table = types.SimpleNamespace(_divide_group=True, _group_num_people=4, num_envs=8, device="cpu",
                                  sim=types.SimpleNamespace(native=types.SimpleNamespace(_sc=dict(seg_body=np.arange(24, dtype=np.uint8)))))
    with pytest.raises(CC.CrowdContactRefusal, match="near_dist"):
        CC.CrowdContactAudit(table, near_dist=0.0)
    assert "divide_group" in CC.config_refusal({}) and "has_self_collision" in CC.config_refusal({"divide_group": True})
    assert CC.config_refusal({"divide_group": True, "has_self_collision": True}) is None
    # the rollout's rule for EMLOCO_OVERLAP_RESET=1, the flight recorder's
    from emloco_amd.learning.locoval_rollout import LocoValRollout
    loop = types.SimpleNamespace(task=types.SimpleNamespace(overlap_reset=True), crowd_audit=None)
    with pytest.raises(RuntimeError, match="overlap_reset"):
        LocoValRollout.attach_crowd_audit(loop, object())
    LocoValRollout.attach_crowd_audit(loop, None)
    loop.task.overlap_reset = False
    LocoValRollout.attach_crowd_audit(loop, "audit")
    assert loop.crowd_audit == "audit"


def test_run_refusals_touch_no_device():
    import emloco_amd
    from emloco_amd import run
    group = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    test = ["--test", "--valuenet_path", "nowhere.pth", "--policy_random_init", "--num_envs", "64"]
    with pytest.raises(SystemExit, match="--eval_crowd audits the crowd contacts of the games of --test"):
        run.main(["--num_envs", "64", "--eval_crowd"])
    with pytest.raises(SystemExit, match="divide_group"):
        run.main(test + ["--eval_crowd"])                                     # the default configuration has no groups
    with pytest.raises(SystemExit, match="divide_group"):
        run.main(["--num_envs", "64", "--stats", "--crowd_audit"])
    with pytest.raises(SystemExit, match="--crowd_near_dist sets up"):
        run.main(["--num_envs", "64", "--crowd_near_dist", "0.5"])
    with pytest.raises(SystemExit, match="finite positive"):
        run.main(test + ["--eval_crowd", "--crowd_near_dist", "-1"])
    with pytest.raises(SystemExit, match="--stats or --experiment"):
        run.main(["--cfg_env", group, "--num_envs", "64", "--crowd_audit"])
    with pytest.raises(SystemExit, match="belongs to training"):
        run.main(test + ["--crowd_audit", "--stats"])
    # the options leave argv and the pinned refusals stay what they were
    argv = ["--test", "--eval_crowd", "--crowd_near_dist", "0.75", "--num_envs", "8"]
    opt = run.pop_test_options(argv)
    assert argv == ["--test", "--num_envs", "8"] and opt["eval_crowd"] is True and opt["crowd_near_dist"] == 0.75
    assert run.pop_test_options(["--test"])["eval_crowd"] is False
    with pytest.raises(SystemExit, match="amp_network_sept_cnn_builder"):
        run.main(["--cfg_env", group, "--num_envs", "64", "--train_policy"])

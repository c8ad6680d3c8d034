"""CPU: several LocoVal networks scored on the same games in one evaluation (`run.py --test --compare_valuenet`).

The kernels (emloco_amd/csrc/locoval_multi.h: locoval_eval_fwd_multi_kernel; eval_kernels.hip: locoval_eval_finish_multi_kernel) run
on the CPU through tests/emu/hip/, beside the single-network path they replace (emloco_locoval_eval_step -> the network's own
forward-rows -> emloco_locoval_eval_finish), on one scripted stream of rewards and dones:
  * every network's record plane equals the single-network run of that network byte for byte, and so do the moments;
  * one network through the new path equals the existing path;
  * the staged inputs are not modified by the forward -- today's contract: neither emloco_locoval_fwd_rows nor the variants'
    forward-rows (called without pose_rot, as the evaluator calls them) writes the rotated pose back, and the new forward takes the
    staged buffers as const: the pose is UNCHANGED after either;
  * the C ABI refuses 0 networks, 9 networks and a bad variant;
  * the command line: --compare_valuenet parsing, the exit on an unknown fc1 width and on a ninth network, the shape of the two files.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import emu
from locoval_harness import DIMS, _ptr, eval_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, T, G, STEP_TO_PRED, GAMMA = 8, 40, 5, 5, 0.99
NETS = (3, 1, 0)                                  # the full, the velocity-only (28) and the trajectory-only (26) network


def params_of(variant, seed):
    n_in, h1, h2, _ = DIMS[variant]
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * sc).astype(np.float32) for s, sc in
            (((h1, n_in), 0.2), ((h1,), 0.1), ((h2, h1), 0.3), ((h2,), 0.1), ((1, h2), 0.5), ((1,), 0.1))]


def script():
    """[T, E] streams: env e's games end where `ends[e]` says.  Env 0 starts with two one-step games (a game that ends at its first
    step), env 1 plays games of STEP_TO_PRED + 1 and + 2 steps (the capture at step_to_pred on the last step, and one step before
    it), env 2 one long game that runs well past step_to_pred, env 7 never finishes its quota; the other boundaries are staggered."""
    ends = [[0, 1, 9, 10, 25, 33], [5, 12, 13, 30, 39], [17, 18, 26, 31, 38], [3, 8, 16, 22, 37, 39], [4, 11, 19, 20, 29],
            [2, 7, 15, 21, 28, 36], [6, 14, 23, 24, 32, 35], [13, 34]]
    dones = np.zeros((T, E), np.int64)
    for e, es in enumerate(ends):
        dones[es, e] = 1
    rng = np.random.default_rng(5)
    return dict(dones=dones, reward_raw=rng.uniform(0, 1, (T, E, 2)).astype(np.float32), disc=rng.uniform(0, 1, (T, E)).astype(np.float32),
                terminate=(dones * rng.integers(0, 2, (T, E))).astype(np.int64), inverted=rng.integers(0, 2, (T, E)).astype(np.uint8),
                wp=np.cumsum(rng.standard_normal((T, E, 15, 3)) * 0.3 + 0.2, axis=2).astype(np.float32),
                ip=(rng.standard_normal((T, E, 24, 3)) * 0.3).astype(np.float32), iv=rng.standard_normal((T, E, 2)).astype(np.float32))


def play(nets, multi):
    """The scripted evaluation.  nets: [(variant, params)].  multi: the table through the two new entry points; otherwise ONE network
    through the existing three launches.  Returns the record planes [N][E][G], the moments [N][20], the games counters and, per step,
    whether the staged pose was left as the step staged it."""
    from emloco_amd.learning.locoval_eval import RECORD_DTYPE, RECORD_WORDS
    from emloco_amd.predictor.ops import LocoValNet, LocoValNets
    lib, s, N = emu.lib(), script(), len(nets)
    assert multi or N == 1
    st, b = eval_state(E, G, STEP_TO_PRED, GAMMA)
    wp, ip, iv = b["waypoint_traj"], b["init_pose"], b["init_vel"]
    values = np.full((N, E), 0.25, np.float32)
    records = np.zeros(N * E * G * RECORD_WORDS, np.int32)
    table = LocoValNets(n_nets=N)
    for k, (v, p) in enumerate(nets):
        table.net[k] = LocoValNet(v, 0, *[a.ctypes.data for a in p], values[k].ctypes.data)
    scratch = [[np.zeros((E, d), np.float32) for d in DIMS[v][:3]] + [np.zeros(E, np.float32)] for v, _ in nets]
    pose_kept, masks = [], []
    for t in range(T):
        wp[:], ip[:], iv[:] = s["wp"][t], s["ip"][t], s["iv"][t]
        args = [_ptr(np.ascontiguousarray(s[k][t])) for k in ("reward_raw", "disc", "dones", "terminate", "inverted")]
        assert lib.emu_locoval_eval_step(C.byref(st), *args) == 0
        staged = {k: b[k].copy() for k in ("traj13", "pose", "vel")}
        masks.append(b["row_mask"].copy())
        if multi:
            assert lib.emu_locoval_eval_fwd_multi(C.byref(st), C.byref(table)) == 0
        else:
            (v, p), (x, h1, h2, ang) = nets[0], scratch[0]
            head = [E, _ptr(b["traj13"]), 3, _ptr(b["pose"]), _ptr(b["vel"]), *[_ptr(a) for a in p], _ptr(values[0]), _ptr(x), _ptr(h1), _ptr(h2), _ptr(ang)]
            if v == 3:                              # as LocoValEvaluator._forward: the full network through its own entry point
                assert lib.emu_locoval_fwd(*head, _ptr(b["row_mask"])) == 0
            else:
                assert lib.emu_locoval_variant_fwd_rows(v, *head, None, _ptr(b["row_mask"])) == 0
        pose_kept.append(all(np.array_equal(staged[k], b[k]) for k in staged))
        if multi:
            assert lib.emu_locoval_eval_finish_multi(C.byref(st), C.byref(table), _ptr(records)) == 0
        else:
            assert lib.emu_locoval_eval_finish(C.byref(st), _ptr(values[0]), _ptr(records)) == 0
    planes = records.view(RECORD_DTYPE).reshape(N, E, G)
    moments = np.zeros((N, 20))
    for k in range(N):
        assert lib.emu_locoval_eval_reduce(E, G, _ptr(planes[k]), _ptr(b["games"]), _ptr(moments[k])) == 0
    return dict(planes=planes, moments=moments, games=b["games"].copy(), n_full=int(b["n_full"][0]), pose_kept=pose_kept, masks=np.array(masks),
                values=values)


@pytest.fixture(scope="module")
def nets():
    return [(v, params_of(v, 100 + v)) for v in NETS]


@pytest.fixture(scope="module")
def multi_run(nets):
    return play(nets, multi=True)


@pytest.fixture(scope="module")
def single_runs(nets):
    return [play([n], multi=False) for n in nets]


def test_the_script_covers_the_games_the_issue_names(single_runs):
    r = single_runs[0]
    steps = r["planes"][0]["steps"]
    recorded = np.arange(G)[None, :] < r["games"][:, None]
    assert list(r["games"]) == [5, 5, 5, 5, 5, 5, 5, 2] and r["n_full"] == 7                 # quota met, and an env that never meets it
    assert steps[0, 0] == 1 and steps[0, 1] == 1                                          # games that end at their first step
    assert STEP_TO_PRED + 1 in steps[recorded] and STEP_TO_PRED + 2 in steps[recorded] and steps[recorded].max() > 2 * STEP_TO_PRED
    starts = [set(np.nonzero(r["masks"][:, e])[0]) for e in range(E)]
    assert len({frozenset(x) for x in starts}) == E                                       # games start at different steps per env
    assert any(0 < m.sum() < E for m in r["masks"]) and any(m.sum() == 0 for m in r["masks"])
    v = r["planes"][0]["value"][recorded]
    assert np.isfinite(v).all() and v.std() > 0.01 and not np.any(v == 0.25)              # every recorded game carries a prediction


def test_every_networks_plane_equals_its_single_network_run_byte_for_byte(multi_run, single_runs):
    for k, single in enumerate(single_runs):
        assert np.array_equal(multi_run["games"], single["games"]) and multi_run["n_full"] == single["n_full"]
        assert multi_run["planes"][k].tobytes() == single["planes"][0].tobytes(), f"network {k}"
        assert np.array_equal(multi_run["planes"][k], single["planes"][0])
        assert np.array_equal(multi_run["values"][k], single["values"][0])                # the rows without a first step included
        assert np.array_equal(multi_run["moments"][k], single["moments"][0]), f"network {k}"


def test_planes_differ_in_value_and_sq_err_alone(multi_run):
    from emloco_amd.learning.locoval_eval import SHARED_FIELDS
    planes = multi_run["planes"]
    for k in range(1, len(NETS)):
        for f in SHARED_FIELDS:
            assert planes[k][f].tobytes() == planes[0][f].tobytes(), f
        assert not np.array_equal(planes[k]["value"], planes[0]["value"])


def test_one_network_through_the_new_path_equals_the_existing_path(nets, single_runs):
    for n, single in zip(nets, single_runs):
        one = play([n], multi=True)
        assert one["planes"].tobytes() == single["planes"].tobytes()
        assert np.array_equal(one["moments"], single["moments"]) and np.array_equal(one["games"], single["games"])
        assert np.array_equal(one["values"], single["values"])


def test_the_same_variant_twice_with_other_weights_and_all_four_variants():
    table = [(3, params_of(3, 1)), (2, params_of(2, 2)), (1, params_of(1, 3)), (0, params_of(0, 4)), (2, params_of(2, 5)), (0, params_of(0, 6)),
             (3, params_of(3, 7)), (1, params_of(1, 8))]                                 # EMLOCO_EVAL_MAX_NETS networks
    got = play(table, multi=True)
    for k, n in enumerate(table):
        single = play([n], multi=False)
        assert got["planes"][k].tobytes() == single["planes"][0].tobytes(), k
        assert np.array_equal(got["moments"][k], single["moments"][0])


def test_the_staged_inputs_are_unchanged_by_the_forward(multi_run, single_runs):
    """Today's contract: the forward-rows of the single path leaves the staged trajectory / pose / velocity as the step staged them
    (no in-place pose rotation reaches the buffer); so does the new forward, for every network of the table."""
    assert all(multi_run["pose_kept"]) and all(all(r["pose_kept"]) for r in single_runs)


# ------------------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_the_entry_points_refuse_no_network_too_many_and_a_bad_variant(capfd):
    """The argument checks come before any launch: they answer without a device."""
    from emloco_amd import _lib as L
    from emloco_amd.predictor.ops import EVAL_MAX_NETS, LocoValNet, LocoValNets
    lib = L.load()
    st, _keep = eval_state(4, 2, step_to_pred=5)
    w = np.zeros(8, np.float32)
    records = np.zeros(4 * 2 * 12 * (EVAL_MAX_NETS + 1), np.int32)
    ok = lambda v: LocoValNet(v, 0, *[w.ctypes.data] * 7)
    assert EVAL_MAX_NETS == 8
    for n_nets, variants in ((0, []), (EVAL_MAX_NETS + 1, [3] * EVAL_MAX_NETS), (-1, [3]), (2, [3, 4]), (1, [-1]), (3, [0, 1, 7])):
        table = LocoValNets(n_nets=n_nets)
        for k, v in enumerate(variants):
            table.net[k] = ok(v)
        assert lib.emloco_locoval_eval_fwd_multi(C.byref(st), C.byref(table), None) == -1, (n_nets, variants)
        assert lib.emloco_locoval_eval_finish_multi(C.byref(st), C.byref(table), _ptr(records), None) == -1, (n_nets, variants)
    table = LocoValNets(n_nets=1)
    table.net[0] = ok(3)
    assert lib.emloco_locoval_eval_fwd_multi(None, C.byref(table), None) == -1 and lib.emloco_locoval_eval_fwd_multi(C.byref(st), None, None) == -1
    assert lib.emloco_locoval_eval_finish_multi(C.byref(st), C.byref(table), None, None) == -1
    table.net[0].w2 = None
    assert lib.emloco_locoval_eval_fwd_multi(C.byref(st), C.byref(table), None) == -1
    assert b"emloco_locoval_eval_fwd_multi" in lib.emloco_last_error()
    assert capfd.readouterr().err == ""                 # the text is returned, not printed


def test_the_table_mirrors_follow_the_header(tmp_path):
    """EmlocoLocoValNet / EmlocoLocoValNets against include/emloco_predictor.h: field names, order and kinds, and the compiler's sizes."""
    from emloco_amd import _abi, _lib as L
    src = _abi.source("emloco_predictor.h")
    for name, mirror in (("EmlocoLocoValNet", L.LocoValNet), ("EmlocoLocoValNets", L.LocoValNets)):
        body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{([^{}]*)\}\s*" + name + r"\s*;", src).group(1)
        fields = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.replace("*", " * ").split(",")
            base, *first = [w_ for w_ in first.split() if w_ != "const"]
            for d in [first] + [m.split() for m in more]:
                fields.append((re.sub(r"\[.*", "", d[-1]), "ptr" if "*" in d else base))
        want = [(f, "ptr" if t is C.c_void_p else {C.c_int32: "int32_t"}.get(t, "EmlocoLocoValNet")) for f, t in mirror._fields_]
        assert fields == want, name
    assert L.LocoValNets._fields_[2][1]._length_ == L.EVAL_MAX_NETS
    if shutil.which("gcc") is None:
        pytest.skip("no gcc to ask for sizeof")
    (tmp_path / "sizes.c").write_text('#include "emloco_predictor.h"\n#include <stdio.h>\nint main(void) {\n'
                                      '    printf("%zu %zu %d\\n", sizeof(EmlocoLocoValNet), sizeof(EmlocoLocoValNets), EMLOCO_EVAL_MAX_NETS);\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "sizes"), str(tmp_path / "sizes.c")])
    a, b, n = map(int, subprocess.check_output([str(tmp_path / "sizes")], text=True).split())
    assert (a, b, n) == (C.sizeof(L.LocoValNet), C.sizeof(L.LocoValNets), L.EVAL_MAX_NETS)


# ------------------------------------------------------------------------------------------------------------ the command line
def _checkpoint(path, variant=None, width=None, seed=0):
    from emloco_amd.learning.value_pose_net import ValuePoseNet
    torch.manual_seed(seed)
    if variant is not None:
        state = ValuePoseNet(use_pose=bool(variant & 2), use_vel=bool(variant & 1)).state_dict()
    else:
        state = {"_network.fc1.weight": torch.zeros(width // 2 - 1, width), "_network.fc1.bias": torch.zeros(width // 2 - 1)}
    torch.save({k: v.cpu() for k, v in state.items()}, str(path))
    return str(path)


def test_compare_valuenet_is_repeatable_and_infers_each_variant(tmp_path):
    from emloco_amd.run import _pop_all, load_compare_valuenets
    argv = ["--test", "--compare_valuenet", "b.pth", "--num_envs", "4", "--compare_valuenet", "c.pth", "--valuenet_path", "a.pth"]
    assert _pop_all(argv, "--compare_valuenet") == ["b.pth", "c.pth"]
    assert argv == ["--test", "--num_envs", "4", "--valuenet_path", "a.pth"]
    with pytest.raises(SystemExit, match="needs a value"):
        _pop_all(["--compare_valuenet"], "--compare_valuenet")
    paths = [_checkpoint(tmp_path / f"v{v}.pth", variant=v) for v in (3, 2, 1, 0)]
    got = load_compare_valuenets(paths)
    assert [(p, v) for p, v, _ in got] == list(zip(paths, (3, 2, 1, 0)))
    assert [int(s["_network.fc1.weight"].shape[1]) for _, _, s in got] == [100, 98, 28, 26]


def test_an_unknown_width_and_a_ninth_network_stop_the_run_naming_the_file(tmp_path):
    from emloco_amd.run import load_compare_valuenets
    good = _checkpoint(tmp_path / "good.pth", variant=1)
    bad = _checkpoint(tmp_path / "odd_width.pth", width=50)
    with pytest.raises(SystemExit, match=r"odd_width\.pth.*50 inputs"):
        load_compare_valuenets([good, bad])
    torch.save({"something": torch.zeros(3)}, str(tmp_path / "not_a_net.pth"))
    with pytest.raises(SystemExit, match=r"not_a_net\.pth"):
        load_compare_valuenets([str(tmp_path / "not_a_net.pth")])
    assert len(load_compare_valuenets([good] * 7)) == 7                                   # eight with --valuenet_path
    ninth = _checkpoint(tmp_path / "ninth.pth", variant=0)
    with pytest.raises(SystemExit, match=r"ninth\.pth.*at most 8"):
        load_compare_valuenets([good] * 7 + [ninth])


def test_run_py_checks_the_added_networks_before_it_touches_a_device(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    good, bad = _checkpoint(tmp_path / "good.pth", variant=3), _checkpoint(tmp_path / "odd_width.pth", width=50)
    base = [sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "4", "--policy_random_init"]
    p = subprocess.run(base + ["--valuenet_path", good, "--compare_valuenet", bad], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "odd_width.pth" in p.stderr and "50 inputs" in p.stderr, p.stderr
    p = subprocess.run(base + ["--valuenet_path", good] + ["--compare_valuenet", good] * 8, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode != 0 and "good.pth" in p.stderr and "at most 8" in p.stderr, p.stderr
    # --valuenet_path keeps its meaning and its error; the new option belongs to --test
    p = subprocess.run(base + ["--compare_valuenet", good], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--valuenet_path" in p.stderr and "required" in p.stderr, p.stderr
    p = subprocess.run([sys.executable, "-m", "emloco_amd.run", "--num_envs", "4", "--compare_valuenet", good], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--compare_valuenet" in p.stderr and "--test" in p.stderr, p.stderr


def _fake_records(n, seed):
    from emloco_amd.learning.locoval_eval import RECORD_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=[(k, RECORD_DTYPE.fields[k][0]) for k in RECORD_DTYPE.names] + [("env", "<i4"), ("game", "<i4")])
    for k in ("disc_to_pred", "cr_to_pred", "loc_to_pred", "pow_to_pred", "cr_end"):
        rec[k] = rng.uniform(0, 5, n)
    rec["norm"] = (rec["cr_to_pred"] + 10) / 110
    rec["steps"], rec["env"], rec["game"] = rng.integers(1, 50, n), np.arange(n) // 2, np.arange(n) % 2
    return rec


def _with_values(shared, seed):
    rec = shared.copy()
    rec["value"] = np.random.default_rng(seed).uniform(0, 1, len(rec)).astype(np.float32)
    rec["sq_err"] = (rec["value"] - rec["norm"]) ** 2
    return rec


def test_paired_block_and_record_columns():
    from emloco_amd.learning.locoval_eval import paired_from_records
    from emloco_amd.run import compare_columns
    shared = _fake_records(24, 1)
    recs = [_with_values(shared, s) for s in (2, 3, 4)]
    paired = paired_from_records(recs)
    assert set(paired) == {"games", "mse", "corr_total", "pairs"} and paired["games"] == 24
    assert [(p["a"], p["b"]) for p in paired["pairs"]] == [(0, 1), (0, 2), (1, 2)]
    mse = [np.mean(r["sq_err"].astype(np.float64)) for r in recs]
    corr = [np.corrcoef(r["value"].astype(np.float64), r["cr_to_pred"].astype(np.float64))[0, 1] for r in recs]
    for p in paired["pairs"]:
        assert p["d_mse"] == mse[p["b"]] - mse[p["a"]] and abs(p["d_corr_total"] - (corr[p["b"]] - corr[p["a"]])) < 1e-15
    other = _with_values(_fake_records(24, 9), 2)                 # other games: the comparison refuses them
    with pytest.raises(AssertionError, match="differs between networks"):
        paired_from_records([recs[0], other])
    with pytest.raises(AssertionError, match="same games"):
        paired_from_records([recs[0], recs[1][:-1]])
    cols = compare_columns(recs)
    assert set(cols) == {"disc_to_pred", "cr_to_pred", "loc_to_pred", "pow_to_pred", "norm", "cr_end", "steps", "terminated", "inverted", "env",
                         "game", "value_0", "sq_err_0", "value_1", "sq_err_1", "value_2", "sq_err_2"}
    for i, r in enumerate(recs):
        assert np.array_equal(cols[f"value_{i}"], r["value"]) and np.array_equal(cols[f"sq_err_{i}"], r["sq_err"])
    assert np.array_equal(cols["cr_to_pred"], shared["cr_to_pred"])

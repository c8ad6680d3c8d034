"""CPU: the path tracking of the LocoVal evaluation (`run.py --test --eval_tracks`; emloco_locoval_eval_track / _track_reduce,
emloco_amd/learning/locoval_eval.py) against the float64 restatement of tests/track_cases.py.

  * the kernels of emloco_amd/csrc/eval_kernels.hip, compiled for the CPU through tests/emu/hip/ and run in the product's order -- the
    real step kernel, the tracker, the real finish kernel -- on the scripted streams: integers and written slots exactly, float fields
    to the bound derived in track_cases.py;
  * the reduction against `track_moments_from_records`, the moments of two shards against those of their union, the `tracking` block;
  * the C entry points' refusals, the ctypes mirror of EmlocoLocoValTrack, the command line's flag and the evaluator's refusals.

Measured on the emulator, as fractions of the bound 8 * 2^-24 * C + 8 * 2^-24 * |want| (C the case's largest coordinate): main case
(C = 56.4) ade 0.003, fde 0.022, mean_dev / max_dev / final_dev 0.118 (max |err| 3.2e-6 m), path_len 0.005, the deviation of every step
0.149 (4.0e-6 m); the stored samples 0.156 ulp(C) (6.0e-7 m; walked half 5.6e-8 m), their target half against the fp32 target 0.94 of
half an ulp of the value.  Cap case (C = 54.8): at most 0.047 for the records, 0.099 per step, samples 0.907 ulp(C) (3.5e-6 m, the
target half; walked half 6.0e-8 m), target half against the fp32 target 1.00 of half an ulp (a tie).
"""
import ctypes as C
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import emu
import track_cases as TC
from locoval_harness import _ptr, eval_state, track_state


def run_emu(case):
    """The scripted streams through step -> track -> finish; returns what `TC.check` takes."""
    from emloco_amd.learning.locoval_eval import RECORD_WORDS, TRACK_DTYPE, TRACK_WORDS
    lib = emu.lib()
    E, G, T = case["E"], case["G"], case["T"]
    st, b = eval_state(E, G)
    t, tb = track_state(case)
    records = np.zeros(E * G * RECORD_WORDS, np.int32)
    track = np.zeros(E * G * TRACK_WORDS, np.int32)
    samples = np.zeros((E, G, TC.TRACK_SAMPLES, 4), np.float32)
    value, rr = np.zeros(E, np.float32), np.ones((E, 2), np.float32)
    dev_now = np.zeros((T, E), np.float32)
    for k in range(T):
        verts, root, prog, dones = (np.ascontiguousarray(case[n][k]) for n in ("verts", "root", "progress", "dones"))
        t.root_pos, t.traj_verts, t.progress_buf = root.ctypes.data, verts.ctypes.data, prog.ctypes.data
        assert lib.emu_locoval_eval_step(C.byref(st), _ptr(rr), None, _ptr(dones), None, None) == 0
        assert lib.emu_locoval_eval_track(C.byref(st), C.byref(t), _ptr(track), _ptr(samples)) == 0
        assert lib.emu_locoval_eval_finish(C.byref(st), _ptr(value), _ptr(records)) == 0
        dev_now[k] = tb["dev_now"]
    return dict(track=track.view(TRACK_DTYPE).reshape(E, G), samples=samples, games=b["games"].copy(), dev_now=dev_now,
                steps=records.view(np.int32).reshape(E, G, RECORD_WORDS)[:, :, 9])


@pytest.fixture(scope="module")
def main_run():
    case = TC.main_case()
    return case, TC.restate(case), run_emu(case)


# ------------------------------------------------------------------------------------------------------------ the scripted cases
def test_the_main_case_holds_what_the_issue_asks_of_it():
    case = TC.main_case()
    want = TC.restate(case)
    n, L = want["rec"]["n_samples"], case["lengths"]
    assert case["E"] == 5 and case["G"] == 2 and case["stride"] == 12
    assert L[0][0] == 1 and n[0, 0] == 0 and want["rec"]["path_len"][0, 0] == 0            # ends at its first step
    assert L[0][1] == 12 and n[0, 1] == 1 and L[1][0] == 13 and n[1, 0] == 1                # on a sample step / one step after it
    assert L[1][1] == 168 and n[1, 1] == 14                                                 # a full game
    assert len(L[3]) > 2 and want["games"][3] == 2 and want["games"][2] == 1               # a third game after the quota; a game cut off
    assert len({tuple(np.cumsum(x)[:2]) for x in L}) == 5                                   # boundaries shifted between the envs
    # late steps clip at the last vertex
    i0, i1, lerp = TC.calc_pos32(case["verts"][0, 0], 160, case["dt"], case["traj_dur"])
    assert (i0, i1, float(lerp)) == (100, 100, 0.0)
    assert (want["rec"]["max_dev"] > 4.0).sum() == 1 and TC.coord_max(case) <= 64.0


def test_emulated_tracker_equals_the_float64_restatement(main_run):
    case, want, got = main_run
    worst = TC.check(case, want, got["track"], got["samples"], got["games"], got["dev_now"])
    assert max(worst.values()) <= 1.0
    # the tracker ran between the real step and finish kernels: the games they counted are the games it recorded
    done = np.arange(case["G"])[None, :] < got["games"][:, None]
    assert list(got["steps"][done]) == [1, 12, 13, 168, 168, 12, 13, 5, 90]
    assert got["track"]["path_len"][0, 0] == 0 and got["track"]["n_samples"][0, 0] == 0


def test_a_game_after_the_quota_leaves_the_records_and_samples_alone():
    """Env 3 plays its third and fourth game after its quota is met: cut the streams where its second game ends, and its slots hold the
    same bytes as after the whole run."""
    case = TC.main_case()
    full = run_emu(case)
    cut = dict(case, T=int(sum(case["lengths"][3][:2])))
    part = run_emu(cut)
    assert part["games"][3] == 2 and full["games"][3] == 2
    assert part["track"][3].tobytes() == full["track"][3].tobytes() and part["samples"][3].tobytes() == full["samples"][3].tobytes()


def test_samples_beyond_the_cap_are_dropped():
    case = TC.cap_case()
    want = TC.restate(case)
    got = run_emu(case)
    worst = TC.check(case, want, got["track"], got["samples"], got["games"], got["dev_now"])
    assert max(worst.values()) <= 1.0
    assert list(got["track"]["n_samples"][:, 0]) == [16, 16, 16] and case["lengths"] == [[20], [16], [17]]
    # fde is the deviation of the sixteenth sample, not of the game's last step
    assert got["track"]["fde"][0, 0] != got["track"]["final_dev"][0, 0] and got["track"]["fde"][1, 0] == got["track"]["final_dev"][1, 0]


# ------------------------------------------------------------------------------------------------------------ moments and report
def _records_of(case, got):
    """The recorded games as the evaluator's `track_records` lays them out (env-major)."""
    env, game = np.nonzero(np.arange(case["G"])[None, :] < got["games"][:, None])
    return got["track"][env, game]


def test_the_reduction_equals_track_moments_from_records(main_run):
    from emloco_amd.learning.locoval_eval import TRACK_MOMENT_NAMES, track_moments_from_records
    case, _, got = main_run
    mom = np.zeros(len(TRACK_MOMENT_NAMES))
    track = np.ascontiguousarray(got["track"])
    games = got["games"].astype(np.int32)
    assert emu.lib().emu_locoval_track_reduce(case["E"], case["G"], _ptr(track), _ptr(games), 4.0, _ptr(mom)) == 0
    ref = track_moments_from_records(_records_of(case, got))
    assert ref[0] == 9 and ref[1] == 7 and ref[10] == got["track"]["n_samples"].sum() and ref[11] == 1
    np.testing.assert_allclose(mom, ref, rtol=1e-12, atol=0)


def test_the_moments_of_two_shards_sum_to_the_moments_of_the_union(main_run):
    """The multi-rank contract: ranks all-reduce(sum) their moment vectors."""
    from emloco_amd.learning.locoval_eval import track_moments_from_records, tracking_from_moments
    case, _, got = main_run
    rec = _records_of(case, got)
    a, b, u = (track_moments_from_records(r) for r in (rec[:4], rec[4:], rec))
    np.testing.assert_allclose(a + b, u, rtol=1e-12, atol=0)
    assert list((a + b)[[0, 1, 10, 11]]) == list(u[[0, 1, 10, 11]])
    trk = tracking_from_moments(a + b)
    s = rec["n_samples"] > 0
    f8 = lambda k, sel=slice(None): rec[k][sel].astype(np.float64)
    assert trk["games"] == 9 and trk["games_sampled"] == 7 and trk["failed"] == 1 and abs(trk["fail_share"] - 1 / 9) < 1e-15
    for key, val in (("av_ade", f8("ade", s).mean()), ("std_ade", f8("ade", s).std()), ("av_fde", f8("fde", s).mean()),
                     ("std_fde", f8("fde", s).std()), ("av_mean_dev", f8("mean_dev").mean()), ("std_mean_dev", f8("mean_dev").std()),
                     ("av_final_dev", f8("final_dev").mean()), ("av_path_len", f8("path_len").mean())):
        assert abs(trk[key] - val) <= 1e-9 * max(1.0, abs(val)), key
    assert len(trk["lines"]) == 3 and trk["lines"][1].startswith("av_ade: ")
    assert tracking_from_moments(np.zeros(12))["games"] == 0


def test_tracking_from_records_correlates_the_value_with_ade_and_fde(main_run):
    from emloco_amd.learning.locoval_eval import tracking_from_records
    case, _, got = main_run
    rec = _records_of(case, got)
    s = rec["n_samples"] > 0
    v0 = -2.0 * rec["ade"].astype(np.float64) + 1.0                 # a value that falls with the error: r = -1 over the sampled games
    v1 = np.arange(len(rec), dtype=np.float64)
    out = tracking_from_records([v0, v1], rec)
    assert abs(out["corr_value_ade"][0] + 1.0) < 1e-12
    assert abs(out["corr_value_fde"][1] - np.corrcoef(v1[s], rec["fde"][s].astype(np.float64))[0, 1]) < 1e-12
    assert abs(out["std_final_dev"] - rec["final_dev"].astype(np.float64).std()) < 1e-15
    assert np.isnan(tracking_from_records([np.ones(len(rec))], rec)["corr_value_ade"][0])


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_library_exports_and_binds_the_two_entry_points():
    from emloco_amd import _abi, _lib as L
    lib = L.load()
    vp, ci = C.c_void_p, C.c_int
    assert lib.emloco_locoval_eval_track.argtypes == [vp, vp, vp, vp, vp] and lib.emloco_locoval_eval_track.restype is ci
    assert lib.emloco_locoval_track_reduce.argtypes == [ci, ci, vp, vp, C.c_float, vp, vp]
    assert {"emloco_locoval_eval_track", "emloco_locoval_track_reduce"} <= set(_abi.parse("emloco_predictor.h"))


def test_the_entry_points_refuse_bad_arguments(capfd):
    """The argument checks come before any launch: they answer without a device."""
    from emloco_amd import _lib as L
    lib = L.load()
    case = dict(E=4, stride=12, dt=1 / 30, traj_dur=5.0)
    st, _b = eval_state(4, 2)
    t, _tb = track_state(case)
    buf = np.zeros(4 * 2 * 16 * 4, np.float32)
    t.root_pos = t.traj_verts = t.progress_buf = buf.ctypes.data
    call = lambda s_=st, t_=t, r=buf, s=buf: lib.emloco_locoval_eval_track(None if s_ is None else C.byref(s_), None if t_ is None else C.byref(t_),
                                                                           _ptr(r), _ptr(s), None)
    assert call(s_=None) == -1 and call(t_=None) == -1 and call(r=None) == -1 and call(s=None) == -1
    for field, bad in (("stride", 0), ("stride", -3), ("root_stride", 1), ("dt", 0.0), ("dt", float("nan")), ("traj_dur", float("inf")),
                       ("traj_dur", -1.0), ("root_pos", None), ("traj_verts", None), ("progress_buf", None), ("sum_dev", None),
                       ("sum_sample_dev", None), ("path_len", None), ("max_dev", None), ("prev_xy", None), ("last_sample_dev", None),
                       ("n_samples", None)):
        keep = getattr(t, field)
        setattr(t, field, bad)
        assert call() == -1, (field, bad)
        setattr(t, field, keep)
    st.games_per_env = 0
    assert call() == -1
    st.games_per_env = 2
    assert b"emloco_locoval_eval_track" in lib.emloco_last_error()
    assert capfd.readouterr().err == ""                 # the text is returned, not printed
    mom = np.zeros(12)
    games = np.zeros(4, np.int32)
    red = lambda n=4, g=2, r=buf, gm=games, m=mom: lib.emloco_locoval_track_reduce(n, g, _ptr(r), _ptr(gm), 4.0, _ptr(m), None)
    assert red(n=0) == -1 and red(g=0) == -1 and red(r=None) == -1 and red(gm=None) == -1 and red(m=None) == -1


def test_the_track_mirror_follows_the_header(tmp_path):
    """EmlocoLocoValTrack / EmlocoLocoValTrackRecord against include/emloco_predictor.h: field names, order and kinds, the compiler's
    sizes and the two constants."""
    from emloco_amd import _abi, _lib as L
    from emloco_amd.learning import locoval_eval as LE
    src = _abi.source("emloco_predictor.h")

    def fields_of(name):
        body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{([^{}]*)\}\s*" + name + r"\s*;", src).group(1)
        out = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.replace("*", " * ").split(",")
            base, *first = [w_ for w_ in first.split() if w_ != "const"]
            for d in [first] + [m.split() for m in more]:
                out.append((d[-1], "ptr" if "*" in d else base))
        return out
    kinds = {C.c_int32: "int32_t", C.c_float: "float", C.c_void_p: "ptr"}
    assert fields_of("EmlocoLocoValTrack") == [(f, kinds[t]) for f, t in L.LocoValTrack._fields_]
    rec = [(f, {"<f4": "float", "<i4": "int32_t"}[LE.TRACK_DTYPE.fields[f][0].str]) for f in LE.TRACK_DTYPE.names]
    assert fields_of("EmlocoLocoValTrackRecord") == rec + [("_pad", "int32_t")]
    assert [LE.TRACK_DTYPE.fields[f][1] for f in LE.TRACK_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24] and LE.TRACK_DTYPE.itemsize == 32
    assert (L.TRACK_SAMPLES, L.TRACK_MOMENTS) == (16, 12) == (LE.TRACK_SAMPLES, len(LE.TRACK_MOMENT_NAMES)) == (TC.TRACK_SAMPLES, 12)
    if shutil.which("gcc") is None:
        pytest.skip("no gcc to ask for sizeof")
    (tmp_path / "sizes.c").write_text('#include "emloco_predictor.h"\n#include <stdio.h>\nint main(void) {\n'
                                      '    printf("%zu %zu %d %d\\n", sizeof(EmlocoLocoValTrack), sizeof(EmlocoLocoValTrackRecord), '
                                      'EMLOCO_TRACK_SAMPLES, EMLOCO_TRACK_MOMENTS);\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "sizes"), str(tmp_path / "sizes.c")])
    a, b, n, m = map(int, subprocess.check_output([str(tmp_path / "sizes")], text=True).split())
    assert (a, b, n, m) == (C.sizeof(L.LocoValTrack), 32, 16, 12)


# ------------------------------------------------------------------------------------------------------------ the host side
def test_run_test_parses_eval_tracks():
    from emloco_amd.run import pop_test_options
    argv = ["--test", "--num_envs", "8", "--eval_tracks", "--games_num", "16", "--eval_records", "games.npz"]
    opt = pop_test_options(argv)
    assert opt["eval_tracks"] is True and opt["games_num"] == "16" and opt["eval_records"] == "games.npz"
    assert argv == ["--test", "--num_envs", "8"]                      # nothing of --test's own is left for get_args
    assert pop_test_options(["--test"])["eval_tracks"] is False
    with pytest.raises(SystemExit, match="--eval_tracks"):
        pop_test_options(["--num_envs", "8", "--eval_tracks"])


def _fake_env(sample_dt, dt, episode):
    task = types.SimpleNamespace(_traj_sample_timestep=sample_dt, dt=dt, max_episode_length=episode, device="cpu", num_envs=4)
    return types.SimpleNamespace(env=types.SimpleNamespace(task=task))


def test_the_evaluator_refuses_an_incommensurate_stride_and_too_many_samples():
    from emloco_amd.learning.locoval_eval import LocoValEvaluator, track_stride
    assert track_stride(0.4, 2 * (1.0 / 60.0), 168) == 12 and track_stride(0.4, 1.0 / 30.0, 192) == 12
    with pytest.raises(ValueError, match="no whole number of control steps"):
        LocoValEvaluator(_fake_env(0.41, 1.0 / 30.0, 168), None, None, 8, track=True)
    with pytest.raises(ValueError, match="no whole number of control steps"):
        track_stride(0.4 + 2e-6, 1.0 / 30.0, 168)
    with pytest.raises(ValueError, match="holds 16"):
        LocoValEvaluator(_fake_env(0.4, 1.0 / 30.0, 193), None, None, 8, track=True)
    # without `track` the same task is not looked at: the evaluator goes on to its device check as before
    with pytest.raises(RuntimeError, match="gfx950"):
        LocoValEvaluator(_fake_env(0.41, 1.0 / 30.0, 168), None, None, 8)

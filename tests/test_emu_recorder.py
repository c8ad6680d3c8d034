"""CPU-only: the flight recorder's kernels (csrc/recorder_kernels.hip) on the emulator against the numpy restatement -- the case
tables of tests/recorder_cases.py, which tests/test_gpu_recorder.py runs on the device -- and the whole chain on the emulated
simulator: record, check, save, load and the oracle replay of every capture (tools/replay_capture.py)."""
import numpy as np
import pytest

import emu_recorder
import flight_recorder_ref as R
import recorder_cases as cases

make = emu_recorder.EmuBackend


@pytest.mark.parametrize("E", [5, 65])
def test_ring_wraps_and_stays_inside(E):
    cases.ring(make, E)


@pytest.mark.parametrize("mask", [31, 31 & ~(R.SPEED | R.EARLY_FALL), R.SPEED, 31 & ~R.REQUEST])
def test_causes(mask):
    cases.causes(make, mask)


def test_claim_does_not_depend_on_the_grid():
    got = [cases.claim(make, grid) for grid in (1, 2, 7, 0)]
    for d in got[1:]:
        assert all((d[k] == got[0][k]).all() for k in ("ring", "slots", "counters", "last", "request"))


def test_suppression_and_slot_content():
    cases.suppression(make)


def test_structure_mirror_has_the_compilers_layout(tmp_path):
    """EmlocoRecorderBufs carries a tag, so the header test of the untagged structures does not see it: size and every field offset
    against the compiler's"""
    import ctypes as C
    import subprocess
    from emloco_amd import _abi, _lib as L
    names = [f for f, _ in L.RecorderBufs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "emloco_task.h"\nint main(void) {\n    printf("%zu\\n", sizeof(EmlocoRecorderBufs));\n'
    src += "".join(f'    printf("%zu\\n", offsetof(EmlocoRecorderBufs, {n}));\n' for n in names) + "    return 0;\n}\n"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    assert out == [C.sizeof(L.RecorderBufs)] + [getattr(L.RecorderBufs, n).offset for n in names]
    assert (L.REC_WORDS, L.REC_POST_WORDS, L.rec_slot_words(8)) == (R.REC_WORDS, R.POST_WORDS, R.slot_words(8)) == (512, 892, 4992)


def test_whole_chain_on_the_emulated_simulator(tmp_path):
    """E = 6, 12 control steps on flat ground, self-collision on, depth 4: the emulated rigid-body step between the emulated record
    and check; the captures are the ones the oracle's run predicts and every one replays clean"""
    import emu
    import helpers
    from emloco_amd.learning import flight_recorder as FR
    sc = cases.chain_scene(6, 12)
    holder = helpers.oracle_sim(sc["models"], sc["root"], sc["dof"], sc["tgt"], self_collision=sc["sc"], **cases.SIM_PARAMS)
    st = cases.sim_state(holder, 0)
    b = make(sc["E"], cases.CHAIN_DEPTH, cases.CHAIN_SLOTS, cause_mask=R.NONFINITE | R.SPEED | R.REQUEST, speed2=sc["limit2"], state=st)
    for t in range(sc["steps"]):
        st["progress"][:] = t
        b.record(t)
        emu.sim_step(holder, 1)
        if t == sc["request"][1]:
            st["request"][sc["request"][0]] = 1
        b.check(t)
    d = b.pull()
    assert d["guards"] and (d["counters"][1:] == 0).all()
    captured = d["slots"][:int(d["counters"][0])]
    file_dict = FR.capture_file(captured, cases.CHAIN_DEPTH, sc["packed"], sc["sc"], holder.params, 1, None)
    cases.chain_verify(sc, captured, file_dict, tmp_path)


def test_command_line_options_and_file_names():
    from emloco_amd.learning.flight_recorder import rank_path
    from emloco_amd.run import capture_options
    argv = ["--num_envs", "64", "--capture", "out/cap.npz", "--capture_speed", "50", "--capture_early_fall", "10", "--stats"]
    opt = capture_options(argv)
    assert argv == ["--num_envs", "64", "--stats"]                 # what get_args does not know has left the list
    assert opt == dict(path="out/cap.npz", depth=8, slots=16, speed=50.0, ang_speed=None, early_fall=10)
    assert capture_options(["--stats"]) is None
    for bad in (["--capture_depth", "4"], ["--capture", "x.npz", "--capture_depth", "0"], ["--capture", "x.npz", "--capture_speed", "-1"],
                ["--capture", "x.npz", "--capture_slots", "many"]):
        with pytest.raises(SystemExit, match="--capture"):
            capture_options(list(bad))
    assert rank_path("out/cap.npz", 0, 1) == "out/cap.npz" and rank_path("out/cap.npz", 3, 4) == "out/cap_rank3.npz"
    assert rank_path("out.d/cap", 1, 2) == "out.d/cap_rank1"


def test_step_hook_runs_between_the_drive_input_and_the_launch():
    """BaseTask.step: before_physics_launch is the twin of after_physics_launch, and unset it is not there at all"""
    from emloco_amd.env.tasks.base_task import BaseTask
    order = []

    class T(BaseTask):
        def __init__(self):
            self.sim, self.gym = None, type("G", (), {"fetch_results": lambda self, sim, wait: order.append("fetch")})()

        def pre_physics_step(self, actions):
            order.append("pre")

        def _physics_step(self):
            order.append("launch")

        def post_physics_step(self):
            order.append("post")
    t = T()
    t.step(None)
    assert order == ["pre", "launch", "fetch", "post"]
    del order[:]
    t.before_physics_launch, t.after_physics_launch = (lambda: order.append("before")), (lambda: order.append("after"))
    t.step(None)
    assert order == ["pre", "before", "launch", "after", "fetch", "post"]


def test_refusals_reach_the_error_channel_without_a_device():
    """the refusals come ahead of any launch: the library says what is wrong with the structure on a machine without a GPU too"""
    import ctypes as C
    from emloco_amd import _lib as L
    lib = L.load()
    for entry in (lib.emloco_recorder_record, lib.emloco_recorder_check):
        assert entry(None, 0, None) == -1 and lib.emloco_last_error() == entry.__name__.encode() + b": null structure"
        bufs = L.RecorderBufs(n_env=4, depth=2, n_slots=1, speed2_limit=float("nan"))
        assert entry(C.byref(bufs), 0, None) == -1 and lib.emloco_last_error() == entry.__name__.encode() + b": speed2_limit negative or NaN"
        bufs.speed2_limit = 1.0
        assert entry(C.byref(bufs), 0, None) == -1 and lib.emloco_last_error() == entry.__name__.encode() + b": null root_state"
        bufs.t0 = 3
        assert entry(C.byref(bufs), 2, None) == -1 and b"t before t0" in lib.emloco_last_error()


def test_capture_log_fills_files_of_bounded_size(tmp_path):
    """CaptureLog on a stand-in recorder: a file holds at most per_file captures, the run goes on in _part files, and an epoch without
    captures writes nothing once a file exists"""
    from emloco_amd.learning import flight_recorder as FR
    W = FR.slot_words(2)

    class Rec:
        depth, saved = 2, []

        def __init__(self, epochs):
            self.epochs = list(epochs)

        def drain(self):
            k = self.epochs.pop(0)
            base = sum(r.shape[0] for r in self.given) if hasattr(self, "given") else 0
            caps = (np.arange(k, dtype=np.uint32)[:, None] + base) * np.ones((1, W), np.uint32)
            self.given = getattr(self, "given", []) + [caps]
            return caps, {c: (1 if c == "speed" and k else 0) for c in FR.CAUSES}

        def save(self, path, captures, missed):
            Rec.saved.append((path, captures[:, 0].tolist(), dict(missed)))
    Rec.saved = []
    log = FR.CaptureLog(Rec([0, 3, 0, 4, 2]), str(tmp_path / "c.npz"), per_file=4)
    got = [log.end_epoch() for _ in range(5)]
    assert [g["captures"] for g in got] == [0, 3, 0, 4, 2] and log.total == 9 and log.missed["speed"] == 3
    names = [p.rsplit("/", 1)[1] for p, _, _ in Rec.saved]
    assert names == ["c.npz", "c.npz", "c.npz", "c_part1.npz", "c_part1.npz", "c_part2.npz"]        # (the third epoch wrote nothing)
    assert [ids for _, ids, _ in Rec.saved] == [[], [0, 1, 2], [0, 1, 2, 3], [4, 5, 6], [4, 5, 6, 7], [8]]
    assert [p.rsplit("/", 1)[1] for p in log.paths] == ["c.npz", "c_part1.npz", "c_part2.npz"] and log.captures.shape[0] == 1
    assert FR.part_path("out.d/cap", 2) == "out.d/cap_part2"

"""CPU-only: the crowd-aware terrain sensor (emloco_amd/csrc/crowd_kernels.hip on the emulator, tests/emu_crowd.py) against the
reference's fixtures (tests/golden/crowd_sensor.npz, tests/golden/gen_golden_crowd.py), against the post-physics kernel's sensor block,
and against the float64 restatement tests/crowd_ref.py where the reference is silent or undefined; the refusals of
emloco_task_crowd_sensor; the CrowdBufs mirror against the header.

The task itself is not constructed here: HumanoidPedestrianTerrain builds its simulator on the device (gymapi.create_sim has no host
path), so the task-level checks live in tests/test_gpu_crowd.py only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crowd_ref
import emu_crowd
from emloco_amd import _abi, _lib as L, crowd_sensor as S

TOL = 2e-5            # the bar of tests/test_gpu_task.py for observation rows against reference fixtures (clipped and scaled row)
HS, VS = 0.1, 0.005


def check_against_ref(rows, flip, ref_rows, ref_flip, channels):
    assert np.abs(rows - ref_rows).max() <= TOL and np.abs(flip - ref_flip).max() <= TOL


def case_args(z, name):
    res, stamps, vel = (int(v) for v in z[name + "_cfg"])
    ids = z[name + "_env_ids"]
    return dict(res=res, extent=float(z[name + "_extent"]), stamps=bool(stamps), channels=3 if vel else 1), (ids if ids.size else None)


def run_case(backend_cls, z, name, **kw):
    a, ids = case_args(z, name)
    rb = z[name + "_rb"]
    gs = int(z["group_size"]) if a["stamps"] else len(rb)
    b = backend_cls(len(rb), z["heightfield"], HS, VS, a["res"], a["extent"], a["channels"], a["stamps"], gs, head_body=int(z["head_body"]))
    rows, flip = b.run(rb, ids, **kw)
    assert b.guards()
    return b, a, ids, rb, gs, rows, flip


def fixture_case(B, name):
    """every scenario below: `B` is the backend class (emulator here, the device in tests/test_gpu_crowd.py); returns what it computed"""
    z, _ = emu_crowd.fixtures()
    b, a, ids, rb, gs, rows, flip = run_case(B, z, name)
    sel = np.arange(len(rb)) if ids is None else ids
    C_ = a["channels"]
    got, ref = rows[sel].reshape(len(sel), -1, C_), z[name + "_rows"].reshape(len(sel), -1, C_)
    assert np.array_equal(got[..., 0], ref[..., 0])                          # the height channel: equal, not close
    assert np.abs(got - ref).max() <= TOL
    gotf, reff = flip[sel].reshape(len(sel), -1, C_), z[name + "_flip"].reshape(len(sel), -1, C_)
    assert np.array_equal(gotf[..., 0], reff[..., 0]) and np.abs(gotf - reff).max() <= TOL
    if ids is not None:                                                      # the rows of the other envs are not written
        rest = np.setdiff1d(np.arange(len(rb)), ids)
        assert not rows[rest].any() and not flip[rest].any()
    if a["stamps"]:
        plain = B(len(rb), z["heightfield"], HS, VS, a["res"], a["extent"], 1, False, len(rb), head_body=int(z["head_body"]))
        assert (plain.run(rb)[0][sel] != got[..., 0]).mean() > 0.01           # the stamps are seen
    # the restatement agrees with the reference: it is the yardstick of the tests below
    rr, rf = crowd_ref.sensor(rb, z["heightfield"], HS, VS, int(z["head_body"]), a["res"], a["extent"], C_, a["stamps"], gs, ids)
    check_against_ref(z[name + "_rows"], z[name + "_flip"], rr, rf, C_)
    return [rows, flip]


@pytest.mark.parametrize("name", emu_crowd.fixtures()[1])
def test_fixture_case(name):
    fixture_case(emu_crowd.EmuBackend, name)


def test_grid_stride():
    """fewer workgroups than envs give the same bytes"""
    z, _ = emu_crowd.fixtures()
    _, _, _, rb, _, rows, flip = run_case(emu_crowd.EmuBackend, z, "a")
    _, _, _, _, _, rows3, flip3 = run_case(emu_crowd.EmuBackend, z, "a", grid=3)
    assert np.array_equal(rows, rows3) and np.array_equal(flip, flip3)


def padded_ids_case(B):
    """-1 entries of an id list are skipped"""
    z, _ = emu_crowd.fixtures()
    _, _, _, rb, _, rows, flip = run_case(B, z, "a")
    b = B(8, z["heightfield"], HS, VS, 8, 2.0, 3, True, 4)
    part, pflip = b.run(rb, [6, -1, 1, -1, -1])
    assert np.array_equal(part[[1, 6]], rows[[1, 6]]) and not part[[0, 2, 3, 4, 5, 7]].any() and b.guards()
    return [part, pflip]


def test_padded_ids():
    padded_ids_case(emu_crowd.EmuBackend)


def default_case(B):
    """stamps off, one channel, 32 x 32, +-2 m: the bytes post_physics_env writes today, and the copied columns beside them"""
    import emu
    rng = np.random.default_rng(5)
    E = 5
    hf = (rng.integers(-3, 4, size=(96, 80)) * 30).astype(np.int16)
    rb = emu_crowd.rb_states(E, rng, [(4.0, 4.0)] * 3 + [(0.3, 7.8), (9.4, 0.2)])
    rb[:, :, :3] += rng.uniform(-0.3, 0.3, (E, 24, 3)).astype(np.float32) * (np.arange(24)[None, :, None] != 0)
    th = emu.TaskHost(E, hf)
    th.rb_state[:] = rb
    th.traj_verts[:] = rng.uniform(0, 9, th.traj_verts.shape)
    th.post_physics(L.POST_OBS)
    n_copy = L.SELF_OBS + 2 * L.TRAJ_SAMPLES
    b = B(E, hf, HS, VS, 32, 2.0, 1, False, E, src_width=L.OBS, n_copy=n_copy)
    b.src[:], b.src_flip[:] = th.obs, th.flip_obs
    b.run(rb)
    assert th.obs[:, n_copy:].any()
    assert np.array_equal(b.obs, th.obs) and np.array_equal(b.flip, th.flip_obs) and b.guards()
    return [b.obs.copy(), b.flip.copy()]


def test_default_sensor_equals_post_physics_block():
    default_case(emu_crowd.EmuBackend)


def two_on_one_spot(order):
    """members 1 and 2 of group 0 at the identical place, different velocities"""
    rng = np.random.default_rng(11)
    rb = emu_crowd.rb_states(8, rng, [(4.03, 4.07)] * 4 + [(6.51, 3.52)] * 4, clear=(16, 1.0))
    a, b = order
    rb[b, 0, :7] = rb[a, 0, :7]
    rb[a, 0, 7:10], rb[b, 0, 7:10] = [1.0, -0.5, 0.1], [-0.7, 0.9, 0.0]
    return rb


def duplicate_case(B, order):
    z, _ = emu_crowd.fixtures()
    rb = two_on_one_spot(order)
    b = B(8, z["heightfield"], HS, VS, 16, 1.0, 3, True, 4)
    rows, flip = b.run(rb)
    rr, rf = crowd_ref.sensor(rb, z["heightfield"], HS, VS, 13, 16, 1.0, 3, True, 4)
    check_against_ref(rows, flip, rr, rf, 3)
    # env 0 looks at the pair: every stamped probe that reads one of the two reads member 2's velocity
    own = crowd_ref.owners(rb, z["heightfield"].shape, HS, 4)[0]
    assert 1 not in own.values() and 2 in own.values()
    return [rows, flip]


@pytest.mark.parametrize("order", [(1, 2), (2, 1)])
def test_duplicate_cell_goes_to_the_higher_index(order):
    duplicate_case(emu_crowd.EmuBackend, order)


def moved(rb, rng, res, extent):
    """every member somewhere else: 0.6 .. 0.9 m further in x and in y, clear of the cell boundaries again"""
    out = rb.copy()
    for e in range(len(rb)):
        while True:
            out[e, [0, 13], :2] = rb[e, [0, 13], :2] + rng.uniform(0.6, 0.9, (1, 2)).astype(np.float32)
            if crowd_ref.clear_of_boundaries(out[e], 13, res, extent, HS):
                break
    return out


def three_calls_case(B):
    z, _ = emu_crowd.fixtures()
    rng = np.random.default_rng(3)
    rb = emu_crowd.rb_states(8, rng, [(3.0, 3.0)] * 4 + [(5.0, 3.5)] * 4, clear=(16, 1.5))
    b = B(8, z["heightfield"], HS, VS, 16, 1.5, 3, True, 4)
    out = []
    for call in range(3):
        rows, flip = b.run(rb)
        out += [rows, flip]
        rr, rf = crowd_ref.sensor(rb, z["heightfield"], HS, VS, 13, 16, 1.5, 3, True, 4)
        check_against_ref(rows, flip, rr, rf, 3)
        rb = moved(rb, rng, 16, 1.5)
    assert b.guards() and b.epoch.tag == 3
    return out


def test_no_stamp_survives_a_call():
    three_calls_case(emu_crowd.EmuBackend)


def wrap_case(B):
    """the call that uses the last tag, and the one after it (the map is cleared, the tag starts over)"""
    z, _ = emu_crowd.fixtures()
    rng = np.random.default_rng(4)
    rb = emu_crowd.rb_states(8, rng, [(3.0, 3.0)] * 4 + [(5.0, 3.5)] * 4, clear=(16, 1.5))
    b = B(8, z["heightfield"], HS, VS, 16, 1.5, 3, True, 4)
    assert b.epoch.shift == 10 and b.epoch.last == (1 << 22) - 1             # 4 * 200 = 800 < 1024
    b.run(rb)
    b.epoch.tag = b.epoch.last - 1
    tags, out = [], []
    for call in range(3):
        rb = moved(rb, rng, 16, 1.5)
        rows, flip = b.run(rb)
        out += [rows, flip]
        tags.append(b.epoch.tag)
        rr, rf = crowd_ref.sensor(rb, z["heightfield"], HS, VS, 13, 16, 1.5, 3, True, 4)
        check_against_ref(rows, flip, rr, rf, 3)
    assert tags == [b.epoch.last, 1, 2] and b.guards()
    return out


def test_epoch_tag_wrap():
    wrap_case(emu_crowd.EmuBackend)


BAD = [np.nan, 1e30, -1e30]


def blown_up_case(B, bad):
    z, _ = emu_crowd.fixtures()
    rng = np.random.default_rng(6)
    rb = emu_crowd.rb_states(8, rng, [(3.0, 3.0)] * 4 + [(5.0, 3.5)] * 4, clear=(16, 1.5))
    b = B(8, z["heightfield"], HS, VS, 16, 1.5, 3, True, 4)
    good, good_flip = b.run(rb)
    rb2 = rb.copy()
    rb2[2, 0, :3] = bad
    rb2[2, 13, :3] = bad
    rows, flip = b.run(rb2)
    assert b.guards()
    rows_, cols_ = z["heightfield"].shape
    cell = (rows_ - 2) * cols_ + cols_ - 2 if bad > 0 else 0                  # map_index1: NaN and below -> 0, above -> shape - 2
    assert b.owner[cell] >> b.epoch.shift == b.epoch.tag and (int(b.owner[cell]) & 1023) - 1 in range(400, 600)     # env 2's
    # the members of the other group see nothing of it; in its own group only the probes that read env 2's old or new cells change
    assert np.array_equal(rows[4:], good[4:]) and np.array_equal(flip[4:], good_flip[4:])
    rr, rf = crowd_ref.sensor(rb2, z["heightfield"], HS, VS, 13, 16, 1.5, 3, True, 4, env_ids=[0, 1, 3])
    check_against_ref(rows[[0, 1, 3]], flip[[0, 1, 3]], rr, rf, 3)
    return [rows[[0, 1, 3, 4, 5, 6, 7]], flip[[0, 1, 3, 4, 5, 6, 7]]]


@pytest.mark.parametrize("bad", BAD)
def test_blown_up_member_faults_nowhere(bad):
    blown_up_case(emu_crowd.EmuBackend, bad)


# ------------------------------------------------------------------ the C ABI
def good_bufs():
    keep = [np.zeros(4096, np.float32) for _ in range(4)]
    b = L.CrowdBufs(8, 4, 96, 80, 13, 8, 3, 1, 340, 0, 192, 0, 10, 1, 0.1, 0.005, *([keep[0].ctypes.data] * 6), None, None,
                    keep[1].ctypes.data, keep[2].ctypes.data)
    return b, keep


REFUSALS = [("n_env", 0, "n_env"), ("group_size", 3, "group_size"), ("res", 0, "res"), ("res", 65, "res"), ("channels", 2, "channels"),
            ("rb_state", None, "rb_state"), ("heightfield", None, "heightfield"), ("probe_xy", None, "probe_xy"), ("obs", None, "obs"),
            ("flip_obs", None, "flip_obs"), ("owner", None, "owner"), ("root_x", None, "root_x"), ("root_y", None, "root_y"),
            ("dst_width", 191, "dst_width"), ("tag", 0, "tag"), ("tag_shift", 9, "tag_shift"), ("hf_rows", 1, "height map")]


@pytest.mark.parametrize("field,value,word", REFUSALS)
def test_refusals(field, value, word, capfd):
    lib = L.load()
    b, keep = good_bufs()
    setattr(b, field, value)
    rc = lib.emloco_task_crowd_sensor(C.byref(b), None, 0, None)
    msg = lib.emloco_last_error().decode()
    assert rc == -1 and msg.startswith("emloco_task_crowd_sensor: ") and word in msg
    with pytest.raises(L.EmlocoError, match="emloco_task_crowd_sensor"):
        L.check(rc, "emloco_task_crowd_sensor")
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_refuses_null_structure_and_negative_n(capfd):
    lib = L.load()
    assert lib.emloco_task_crowd_sensor(None, None, 0, None) == -1 and b"null structure" in lib.emloco_last_error()
    b, keep = good_bufs()
    assert lib.emloco_task_crowd_sensor(C.byref(b), keep[0].ctypes.data, -1, None) == -1 and b"n < 0" in lib.emloco_last_error()
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_python_refusals():
    with pytest.raises(S.CrowdSensorError, match="multiple"):
        S.group_layout(10, 4)
    assert S.group_layout(8, 512) == (8, 1) and S.group_layout(2048, 512) == (512, 4)
    assert S.stamp_units(0.005) == 340 and crowd_ref.stamp_units(0.005) == 340
    assert S.stamp_units(1.7 / 40000.0) == 40000 - 65536                      # .short() wraps


def test_crowd_bufs_mirror_follows_the_header(tmp_path):
    m = re.search(r"typedef\s+struct\s+EmlocoCrowdBufs\s*\{([^{}]*)\}\s*EmlocoCrowdBufs\s*;", _abi.source("emloco_task.h"))
    fields = []
    for decl in filter(str.strip, m.group(1).split(";")):
        first, *more = decl.replace("*", " * ").split(",")
        base, *first = [w for w in first.split() if w != "const"]
        for d in [first] + [x.split() for x in more]:
            assert len(d) == 1 + ("*" in d) and re.fullmatch(r"\w+", d[-1]), decl
            fields.append((d[-1], "ptr" if "*" in d else _abi.SCALARS[base]))
    assert [(f, "ptr" if t is C.c_void_p else t) for f, t in L.CrowdBufs._fields_] == fields
    if shutil.which("gcc") is None:
        pytest.skip("no gcc to ask for sizeof")
    (tmp_path / "size.c").write_text('#include "emloco_task.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(EmlocoCrowdBufs)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "size"), str(tmp_path / "size.c")])
    assert int(subprocess.check_output([str(tmp_path / "size")], text=True)) == C.sizeof(L.CrowdBufs)
    assert (L.CROWD_ROOT_X, L.CROWD_ROOT_Y, L.CROWD_MAX_RES) == (10, 20, 64)


def test_run_refuses_a_policy_on_a_crowd_configuration():
    import emloco_amd
    from emloco_amd import run
    cfg_env = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg", "pacer_group.yaml")
    for extra in (["--policy_random_init"], ["--train_policy"], ["--policy_checkpoint", "nowhere.pth"],
                  ["--test", "--valuenet_path", "nowhere.pth", "--policy_random_init"]):
        with pytest.raises(SystemExit, match="amp_network_sept_cnn_builder"):
            run.main(["--cfg_env", cfg_env, "--num_envs", "64"] + extra)

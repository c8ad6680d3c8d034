"""CPU-only: the crowd policy's convolution trunk (emloco_amd/csrc/cnn_kernels.hip on the emulator, tests/emu_cnn.py) against its
float64 restatement (tests/cnn_ref.py), and the refusals of emloco_cnn_trunk.

The bar, emulator against float64: max|err| <= 2e-6 * max|ref| + 1e-7.  Stock torch fp32 against float64 for the same tower and input
scale differs by 1.5e-7 to 3.0e-7 of the output scale on the build machine (2.4e-7 at (16, 3), 4.1e-7 at (64, 3)); the bar is five times
that, for a different but fixed summation order.  tests/test_gpu_cnn_policy.py runs the same cases on the device, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import cnn_ref
import emu_cnn
from emloco_amd import _lib as L

NAMES = list(emu_cnn.CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, features float64, every layer's activations): computed once, shared, never written"""
    c = emu_cnn.draw_case(name)
    width = c["ch"] * c["res"] ** 2
    maps = c["obs"][:, c["lead"]:c["lead"] + width]
    feat, acts = cnn_ref.trunk(maps, c["res"], c["ch"], c["weights"], c["biases"], c["mean"], c["var"], emu_cnn.EPS, emu_cnn.CLIP)
    feat.setflags(write=False)
    return c, feat, acts


def check_case(B, name, **kw):
    """every back end: the features against float64, the columns around them and the guards untouched; returns the features"""
    c, ref, _ = reference(name)
    got, untouched, guards = B(c).run(**kw)
    assert untouched and guards
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{name}: max|err| {err:.3e}, max|ref| {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= 2e-6 * scale + 1e-7
    return got


@pytest.mark.parametrize("name", NAMES)
def test_reference_has_clamped_inputs_and_a_share_of_zeros(name):
    c, _, acts = reference(name)
    width = c["ch"] * c["res"] ** 2
    maps = c["obs"][:, c["lead"]:c["lead"] + width]
    n = cnn_ref.normalize(maps, c["mean"], c["var"], emu_cnn.EPS, emu_cnn.CLIP)
    assert (n == 5.0).any() and (n == -5.0).any()
    for a in acts:
        share = float((a == 0).mean())
        assert 0.10 <= share <= 0.90, share
    assert all(np.abs(b).min() > 0 for b in c["biases"])


@pytest.mark.parametrize("name", NAMES)
def test_emulator_against_float64_and_any_grid(name):
    c, _, _ = reference(name)
    one = check_case(emu_cnn.EmuBackend, name, grid=1)
    for grid in (2, c["rows"]):
        got, untouched, guards = emu_cnn.EmuBackend(c).run(grid=grid)
        assert untouched and guards and np.array_equal(got.view(np.uint32), one.view(np.uint32))


def test_flatten_order_is_channel_major():
    c = dict(emu_cnn.draw_case("r16c3"))
    keep = 5
    w3 = np.zeros_like(c["weights"][2])
    w3[keep] = np.abs(c["weights"][2][keep]) + 0.05
    b3 = np.zeros_like(c["biases"][2])
    c["weights"], c["biases"] = c["weights"][:2] + [w3], c["biases"][:2] + [b3]
    got, untouched, guards = emu_cnn.EmuBackend(c).run()
    assert untouched and guards
    side = 16 >> 3
    blocks = got.reshape(c["rows"], 16, side * side)
    assert (blocks[:, keep] > 0).all()
    assert (np.delete(blocks, keep, axis=1) == 0).all()


@pytest.mark.parametrize("name", ["r16c3", "r32c1"])
def test_normalisation_off_equals_the_prenormalised_map(name):
    c, _, _ = reference(name)
    b = emu_cnn.EmuBackend(c)
    on, _, _ = b.run()
    pre = c["obs"].copy()
    width = c["ch"] * c["res"] ** 2
    m = pre[:, c["lead"]:c["lead"] + width]
    y = (m - c["mean"]) / np.sqrt(c["var"] + np.float32(emu_cnn.EPS))                 # float32 throughout, the kernel's operation order
    pre[:, c["lead"]:c["lead"] + width] = np.minimum(np.maximum(y, np.float32(-emu_cnn.CLIP)), np.float32(emu_cnn.CLIP))
    assert pre.dtype == np.float32
    off, untouched, guards = b.run(normalize=False, obs=pre)
    assert untouched and guards and np.array_equal(on.view(np.uint32), off.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- refusals of the C ABI
def good_args():
    keep = [np.zeros(8 * 8 * 3 + 4, np.float32), np.zeros(192, np.float32), np.ones(192, np.float32), np.zeros(4096, np.float32),
            np.zeros(64, np.float32)]
    p = [a.ctypes.data for a in keep]
    args = dict(rows=1, res=8, channels=3, layers=2, f0=4, f1=4, f2=0, f3=0, x=p[0], ldx=196, mean=p[1], var=p[2], eps=1e-5, clip=5.0,
                normalize=1, params=p[3], out=p[4], ldo=20, out_off=2, stream=None)
    return args, keep


REFUSALS = [("x", None, "x"), ("mean", None, "mean"), ("var", None, "var"), ("params", None, "params"), ("out", None, "out"),
            ("res", 12, "res"), ("res", 72, "res"), ("res", 0, "res"), ("channels", 2, "channels"), ("layers", 0, "layers"),
            ("layers", 5, "layers"), ("f1", 17, "filters"), ("f0", 0, "filters"), ("ldx", 191, "ldx"), ("ldo", 17, "ldo"),
            ("rows", 0, "rows"), ("out_off", -1, "out_off")]


@pytest.mark.parametrize("field,value,word", REFUSALS)
def test_refusals(field, value, word, capfd):
    lib = L.load()
    args, keep = good_args()
    args[field] = value
    a = dict(args, eps=C.c_float(args["eps"]), clip=C.c_float(args["clip"]))
    rc = lib.emloco_cnn_trunk(*a.values())
    msg = lib.emloco_last_error().decode()
    assert rc == -1 and msg.startswith("emloco_cnn_trunk: ") and word in msg, (rc, msg)
    with pytest.raises(L.EmlocoError, match="emloco_cnn_trunk"):
        L.check(rc, "emloco_cnn_trunk")
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_a_side_that_does_not_halve_through_every_layer_is_refused():
    lib = L.load()
    args, keep = good_args()
    args.update(layers=4, f2=4, f3=4, eps=C.c_float(1e-5), clip=C.c_float(5.0))
    assert lib.emloco_cnn_trunk(*args.values()) == -1 and b"halve" in lib.emloco_last_error()

"""CPU-only: the backward of the crowd policy's convolution trunk (emloco_amd/csrc/cnn_backward_kernels.hip on the emulator,
tests/emu_cnn_bwd.py) against float64 autograd (tests/cnn_bwd_ref.py); the refusals of emloco_cnn_trunk_backward and of its workspace
query; the --cnn_backward gate of run.py; the kernel's scratch and LDS from the compiler's own remarks.

The bar, emulator against float64, per gradient tensor (every layer's dW and db): max|err| <= K * max|ref| + 1e-7 with K = 3.4e-6.
How K was set: stock torch fp32 autograd on the CPU (cnn_bwd_ref.backward(dtype=torch.float32)) against the same float64 reference on
the same cases differs by 2.3e-8 .. 6.84e-7 of a tensor's largest value on the build machine -- the largest per case: r16c3 2.8e-7,
r32c1 4.3e-7, r64c3 6.84e-7 (first layer's dW), r16c1_two_layers 1.7e-7, r8c3_one_layer 7.0e-8, r16c1_four_layers 5.2e-7,
r16c3_f5_16_7 2.4e-7, r16c1_two_layers_many_rows (259 rows) 5.7e-7 -- and K is five times the largest, for a different but fixed
summation order (the rule of tests/test_cnn_trunk_cpu.py).  The emulator itself: 2.3e-8 .. 3.7e-7.  The ReLU masks cannot differ
between fp32 and float64 on these inputs: test_reference_inputs holds every float64 pre-activation at least 2e-6 of its layer's largest
away from zero, five times the forward's measured fp32 error.  tests/test_gpu_cnn_backward.py runs the same cases on the device, bit for
bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import cnn_bwd_ref
import cnn_ref
import emu_cnn_bwd as E
import test_build_resources as B
from emloco_amd import _lib as L

NAMES = list(E.CASES)
K_BAR, TINY = 3.4e-6, 1e-7


def maps_of(c):
    width = c["ch"] * c["res"] ** 2
    return c["obs"][:, c["lead"]:c["lead"] + width]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, [(dW, db) per layer] float64, every layer's pre-activation float64): computed once, shared, never written"""
    c = E.draw_case(name)
    grads, pre, _ = cnn_bwd_ref.backward(maps_of(c), c["res"], c["ch"], c["weights"], c["biases"], c["dout"], c["mean"], c["var"], E.EPS, E.CLIP)
    for w, b in grads:
        w.setflags(write=False), b.setflags(write=False)
    return c, grads, pre


def within_bar(name, dparams):
    """every gradient tensor of a packed result against float64; prints each figure before it asserts"""
    c, ref, _ = reference(name)
    for l, ((gw, gb), (rw, rb)) in enumerate(zip(E.split_params(dparams, c["ch"], c["filters"]), ref)):
        for what, got, want in (("dW", gw, rw), ("db", gb, rb)):
            assert np.isfinite(got).all(), (name, l, what)
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            print(f"{name} layer {l + 1} {what}: max|err| {err:.3e}, max|ref| {scale:.3e}, ratio {err / scale:.3e}")
            assert err <= K_BAR * scale + TINY, (name, l, what, err, scale)


def check_case(Backend, name, **kw):
    """every back end: dparams within the bar, guards intact, the workspace written only in its first grid * P floats"""
    c, _, _ = reference(name)
    got, guards, tail = Backend(c).run(**kw)
    assert guards and tail
    within_bar(name, got)
    return got


def bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_reference_inputs(name):
    c, grads, pre = reference(name)
    n = cnn_ref.normalize(maps_of(c), c["mean"], c["var"], E.EPS, E.CLIP)
    assert (n == 5.0).any() and (n == -5.0).any()
    assert all(np.abs(b).min() > 0 for b in c["biases"])
    for p in pre:
        share = float((p <= 0).mean())
        assert 0.10 <= share <= 0.90, share
        margin = np.abs(p).min() / np.abs(p).max()
        print(f"{name}: zero share {share:.2f}, nearest pre-activation {margin:.3e} of the layer's largest")
        assert margin > 2e-6, margin
    assert all(np.abs(w).max() > 0 and np.abs(b).max() > 0 for w, b in grads)
    if name.endswith("many_rows"):
        assert c["rows"] == E.grid_of(c["rows"], c["res"], c["ch"], c["filters"]) + 3       # one workgroup takes two rows, most take one


@pytest.mark.parametrize("name", NAMES)
def test_emulator_against_float64(name):
    check_case(E.EmuBackend, name)


@pytest.mark.parametrize("name", NAMES)
def test_emulator_twice_gives_the_same_bits(name):
    c, _, _ = reference(name)
    b = E.EmuBackend(c)
    one, two = b.run(), b.run()
    assert one[1] and one[2] and two[1] and two[2] and np.array_equal(bits(one[0]), bits(two[0]))


@pytest.mark.parametrize("name", NAMES)
def test_emulator_at_any_grid(name):
    c, _, _ = reference(name)
    for grid in (1, 2, c["rows"]):
        check_case(E.EmuBackend, name, grid=grid)


@pytest.mark.parametrize("name", ["r16c3", "r32c1"])
def test_normalisation_off_equals_the_prenormalised_map(name):
    c, _, _ = reference(name)
    b = E.EmuBackend(c)
    on, g_on, t_on = b.run()
    pre = c["obs"].copy()
    width = c["ch"] * c["res"] ** 2
    m = pre[:, c["lead"]:c["lead"] + width]
    y = (m - c["mean"]) / np.sqrt(c["var"] + np.float32(E.EPS))                          # float32 throughout, the kernel's operation order
    pre[:, c["lead"]:c["lead"] + width] = np.minimum(np.maximum(y, np.float32(-E.CLIP)), np.float32(E.CLIP))
    assert pre.dtype == np.float32
    off, g_off, t_off = b.run(normalize=False, obs=pre)
    assert g_on and t_on and g_off and t_off and np.array_equal(bits(on), bits(off))


@pytest.mark.parametrize("name", ["r16c3", "r16c1_four_layers", "r8c3_one_layer"])
def test_a_zero_dout_gives_exactly_zero(name):
    c, _, _ = reference(name)
    got, guards, tail = E.EmuBackend(c).run(dout=np.zeros_like(c["dout"]))
    assert guards and tail and (got == 0).all()


# ---------------------------------------------------------------------------------------------------------------- refusals of the C ABI
def good_args():
    keep = [np.zeros(8 * 8 * 3 + 4, np.float32), np.zeros(192, np.float32), np.ones(192, np.float32), np.zeros(4096, np.float32),
            np.zeros(64, np.float32), np.zeros(456, np.float32), np.zeros(456, np.float32)]
    p = [a.ctypes.data for a in keep]
    args = dict(rows=1, res=8, channels=3, layers=2, f0=4, f1=4, f2=0, f3=0, x=p[0], ldx=196, mean=p[1], var=p[2], eps=1e-5, clip=5.0,
                normalize=1, params=p[3], dout=p[4], lddo=20, dout_off=2, dparams=p[5], workspace=p[6], workspace_floats=456, stream=None)
    return args, keep


REFUSALS = [("x", None, "x"), ("mean", None, "mean"), ("var", None, "var"), ("params", None, "params"), ("dout", None, "dout"),
            ("dparams", None, "dparams"), ("workspace", None, "workspace"), ("res", 12, "res"), ("res", 72, "res"), ("res", 0, "res"),
            ("channels", 2, "channels"), ("layers", 0, "layers"), ("layers", 5, "layers"), ("f1", 17, "filters"), ("f0", 0, "filters"),
            ("ldx", 191, "ldx"), ("lddo", 17, "lddo"), ("rows", 0, "rows"), ("dout_off", -1, "dout_off"),
            ("workspace_floats", 455, "workspace_floats")]


@pytest.mark.parametrize("field,value,word", REFUSALS)
def test_refusals(field, value, word, capfd):
    lib = L.load()
    args, keep = good_args()
    args[field] = value
    a = dict(args, eps=C.c_float(args["eps"]), clip=C.c_float(args["clip"]))
    rc = lib.emloco_cnn_trunk_backward(*a.values())
    msg = lib.emloco_last_error().decode()
    assert rc == -1 and msg.startswith("emloco_cnn_trunk_backward: ") and word in msg, (rc, msg)
    with pytest.raises(L.EmlocoError, match="emloco_cnn_trunk_backward"):
        L.check(rc, "emloco_cnn_trunk_backward")
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_workspace_query(capfd):
    lib = L.load()
    shape = dict(rows=1, res=8, channels=3, layers=2, f0=4, f1=4, f2=0, f3=0)
    assert lib.emloco_cnn_trunk_backward_workspace(*shape.values()) == 456                      # one workgroup, P = 196 + 260
    limit = E.grid_of(1 << 20, 8, 3, (4, 4))
    assert limit >= 1 and E.grid_of(limit, 8, 3, (4, 4)) == limit == E.grid_of(limit + 3, 8, 3, (4, 4)) and E.grid_of(2, 8, 3, (4, 4)) == min(2, limit)
    for field, value, word in [("res", 12, "res"), ("res", 72, "res"), ("channels", 2, "channels"), ("layers", 5, "layers"),
                               ("layers", 0, "layers"), ("f1", 17, "filters"), ("f0", 0, "filters"), ("rows", 0, "rows"), ("layers", 4, "halve")]:
        a = dict(shape, **{field: value})
        if word == "halve":
            a.update(f2=4, f3=4)
        n = lib.emloco_cnn_trunk_backward_workspace(*a.values())
        msg = lib.emloco_last_error().decode()
        assert n == -1 and msg.startswith("emloco_cnn_trunk_backward_workspace: ") and word in msg, (n, msg)
    out = capfd.readouterr()
    assert out.out == "" and out.err == ""


def test_a_side_that_does_not_halve_through_every_layer_is_refused():
    lib = L.load()
    args, keep = good_args()
    args.update(layers=4, f2=4, f3=4, eps=C.c_float(1e-5), clip=C.c_float(5.0))
    assert lib.emloco_cnn_trunk_backward(*args.values()) == -1 and b"halve" in lib.emloco_last_error()


# ---------------------------------------------------------------------------------------------------------------- the gate of run.py
def _env_cfgs():
    import os

    import yaml

    import emloco_amd
    cfg = os.path.join(os.path.dirname(emloco_amd.__file__), "data", "cfg")
    crowd_path = os.path.join(cfg, "pacer_group.yaml")
    return crowd_path, yaml.safe_load(open(crowd_path))["env"], yaml.safe_load(open(os.path.join(cfg, "pacer.yaml")))["env"]


def test_cnn_backward_opens_the_gate_for_the_cnn_network_only():
    from emloco_amd import run
    _, crowd, plain = _env_cfgs()
    f = dict(use_policy=False, train_policy=True, test=False)
    assert run.crowd_policy_refusal(crowd, "amp_sept_cnn", cnn_backward=True, **f) is None
    assert run.crowd_policy_refusal(plain, "amp_sept_cnn", cnn_backward=True, **f) is None
    for sept in ("amp_sept", "amp_sept_value"):
        text = run.crowd_policy_refusal(crowd, sept, cnn_backward=True, **f)
        assert text and "amp_network_sept_cnn_builder" in text
        assert run.crowd_policy_refusal(plain, sept, cnn_backward=True, **f) is None            # (run.main refuses the flag itself, below)
    text = run.crowd_policy_refusal(crowd, "amp_sept_cnn", **f)                                  # the default: today's refusal, naming the flag
    assert "backward is not built" in text and "amp_network_sept_cnn_builder" in text and "--cnn_backward" in text
    assert "--cnn_backward" in run.crowd_policy_refusal(plain, "amp_sept_cnn", cnn_backward=False, **f)


def test_run_refuses_cnn_backward_where_it_means_nothing():
    from emloco_amd import run
    from emloco_amd.learning.amp_policy import CNN_CFG
    crowd_path, _, _ = _env_cfgs()
    with pytest.raises(SystemExit, match="--cnn_backward.*--train_policy"):
        run.main(["--cfg_env", crowd_path, "--num_envs", "64", "--cfg_train", CNN_CFG, "--policy_random_init", "--cnn_backward"])
    with pytest.raises(SystemExit, match="--cnn_backward.*amp_sept_value.*no CNN trunk"):
        run.main(["--num_envs", "64", "--train_policy", "--cnn_backward"])                       # the default task, the sept network
    with pytest.raises(SystemExit, match="amp_network_sept_cnn_builder"):
        run.main(["--cfg_env", crowd_path, "--num_envs", "64", "--train_policy", "--cnn_backward"])      # sept network, crowd configuration


# ---------------------------------------------------------------------------------------------------------------- the compiler's remarks
def test_backward_kernel_has_no_scratch_and_fits_the_lds():
    from emloco_amd import build
    flags = {src: extra for src, extra in build.UNITS}
    p = B._remarks("cnn_capi.hip", flags["cnn_capi.hip"])
    text, _ = p.communicate()
    assert p.returncode == 0, text[-2000:]
    res = B._parse(text)
    ks = [k for k in res if "cnn_trunk_backward_kernel" in k]
    assert len(ks) == 1, list(res)
    r = res[ks[0]]
    print("cnn_trunk_backward_kernel:", r)
    assert r["ScratchSize"] == 0 and 0 < r["LDS"] <= 163840, r
    red = [res[k] for k in res if "cnn_grad_reduce_kernel" in k]
    assert len(red) == 1 and red[0]["ScratchSize"] == 0

"""Device conformance matrix of the normalisation, loss-head and optimiser kernels against float64 (tests/kernel_refs.py).

Companion of tests/test_gpu_kernel_matrix.py: every case calls a C entry point of include/emloco_predictor.h directly through ctypes
with explicit arguments, so the case decides which kernel and which branch runs.  Every output is a guarded buffer (sentinel before,
behind and -- where a leading dimension is loose -- between the rows, which must survive; NaN in the logical output before the launch,
so an element never written fails); inputs carry large garbage outside their logical extent.

Covered here: emloco_layernorm_fwd / _fwd_save / _bwd / _bwd2, emloco_softmax_fwd / _bwd, emloco_act_bwd (= the dz of
emloco_act_bwd_colsum), emloco_colsum (= emloco_colsum_ex with flags 0), emloco_gather_flat, emloco_obs_normalize, emloco_disc_reward,
emloco_rms_update / _chunked, emloco_ffn_fwd / _fwd_norm / _bwd_input / _bwd_input_colsum (F = 64 .. 2048, the mask decoded bit by bit),
emloco_locoval_fwd / _fwd_rows / _bwd / _bwd_rows, emloco_locoval_fit_grad, emloco_adamw_gated, emloco_adam_clip_flat / _counted,
emloco_ppo_actor_head_fwd / _bwd, emloco_ppo_critic_head_fwd / _bwd, emloco_ppo_disc_head_fwd / _bwd, emloco_ppo_gather_rows, and the
host-side refusals (d > 1024, F > 2048 in all four feed-forward entry points, steps_in == steps_out, count_in == count_out).

The chained feed-forward is bf16-operand only: it is checked against float64 on the bf16-rounded operands stage by stage -- the hidden
layer / dz1 as ONE bf16 rounding (half a spacing, 2^-8 of the value) of an fp32 accumulation (BAR_FP32 of sum |a b|, the header's figure
for fp32 accumulation), then the second product from the hidden layer / dz1 AS STORED, where only the fp32 accumulation is left -- and
asserted to be visibly reduced precision against the unrounded float64 (error > 1e-4 of scale).

Bars.  Copies, masks, counts, slots, step counters and "left as it is" regions: exact (bit for bit).  Single-rounding element-wise
results: 2^-22 of the result's magnitude.  Fixed-order fp32 sums: COLSUM_C x sum |terms| (the bar of test_gpu_kernel_matrix).  Every
other output: the same operation is evaluated in float32 with stock torch on the CPU (kernel_refs with dtype=float32) on the case's own
inputs; the family's bar is 8 x the largest float32-vs-float64 error over its cases, in the measure the test uses (max error over the
tensor's max, or over sum |terms| for means and sums).  A different but legitimate summation order or expf / logf moves the error by a
small factor, a wrong element or a dropped term by orders of magnitude.  The bar is one per family and output (the largest float32
error over the family's cases), not one per case: a tiny case whose float32 evaluation happens to be exact would otherwise get a bar of
0; the price is that a small case is judged against the tall case's error -- still orders of magnitude below a wrong element.

Measured (MI355X, the run that accompanied this file; figures are printed by every run, `pytest -s`):

    family / output                float32 reference     bar (8 x)     device
    layernorm y                    1.69e-07              1.35e-06      1.51e-07
    layernorm mean                 1.17e-07              9.37e-07      1.51e-07
    layernorm rstd                 1.19e-07              9.50e-07      1.22e-07
    layernorm dxr                  1.31e-07              1.05e-06      1.31e-07
    softmax P                      3.67e-07              2.94e-06      2.39e-07
    softmax dS                     1.80e-07              1.44e-06      1.80e-07
    disc_reward                    4.75e-06              3.80e-05      4.83e-06
    adamw_gated params             2.42e-07              1.94e-06      1.64e-07
    adamw_gated exp_avg            8.74e-08              6.99e-07      8.74e-08
    adamw_gated exp_avg_sq         1.20e-07              9.59e-07      1.20e-07
    adam_clip_flat params          1.07e-07              8.53e-07      1.07e-07
    adam_clip_flat exp_avg         1.29e-07              1.03e-06      1.08e-07
    adam_clip_flat exp_avg_sq      2.84e-07              2.27e-06      2.54e-07
    ppo_actor_head surrogate       1.61e-06              1.29e-05      2.79e-06
    ppo_actor_head entropy         1.08e-07              8.60e-07      1.37e-07
    ppo_actor_head bound           7.06e-08              5.65e-07      9.33e-08
    ppo_actor_head kl              8.22e-06              6.58e-05      8.22e-06
    ppo_actor_head dmu             8.11e-06              6.49e-05      8.87e-06
    ppo_actor_head dlogstd         8.74e-06              6.99e-05      1.03e-05
    ppo_critic_head loss           1.73e-07              1.39e-06      1.13e-07
    ppo_critic_head dvalues        9.18e-08              7.34e-07      9.18e-08
    ppo_disc_head bce_agent        8.48e-08              6.78e-07      7.77e-08
    ppo_disc_head bce_demo         3.52e-08              2.82e-07      3.52e-08
    ppo_disc_head d_agent          1.29e-07              1.03e-06      1.29e-07
    ppo_disc_head d_demo           1.13e-07              9.01e-07      1.13e-07
    ffn norm y                     1.61e-07              1.29e-06      1.88e-07
    ffn norm y (2 launches)        1.61e-07              1.29e-06      1.98e-07
    ffn norm mean                  1.71e-07              1.37e-06      2.01e-07
    ffn norm rstd                  1.32e-07              1.06e-06      1.25e-07
    locoval value                  6.84e-07              5.47e-06      7.04e-07
    locoval x100                   9.35e-08              7.48e-07      8.46e-08
    locoval h1                     4.97e-07              3.97e-06      5.02e-07
    locoval h2                     4.00e-07              3.20e-06      4.40e-07
    locoval angle                  5.38e-08              4.31e-07      7.28e-08
    locoval dparams                8.91e-05              7.13e-04      4.60e-05
    locoval d traj                 5.40e-07              4.32e-06      4.76e-07
    obs_normalize (derived bar)    --                    4.77e-07      1.82e-07

(locoval dparams: over sum |terms| of the batch sum, where a product with a nearly dead hidden unit's activation carries that activation's
own float32 cancellation error -- the float32 reference shows the same 1e-5 class.  The feed-forward's hidden / out / dz1 / dx bars are
derived, see above.)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R                                                          # noqa: E402
from test_gpu_kernel_matrix import DEV, GARBAGE, SENT, TAIL, _bits, _Guarded, _ptr, _stream          # noqa: E402
from test_kernel_refs_cpu import (ACTOR_SHAPES, CRITIC_SIZES, E_CLIP, OBS_CASES, SHARE_CAP, constructed_actor,   # noqa: E402
                                  constructed_critic)

F32, F64 = torch.float32, torch.float64
COLSUM_C = 1e-5                         # fixed-order fp32 sums: c x sum |x| (test_gpu_kernel_matrix._colsum_bar)
ULP4 = 2.0 ** -22                       # single-rounding element-wise results
OBS_BAR = 4 * 2.0 ** -23                # obs_normalize away from the clamp: a subtraction, an addition, a square root and a division, one ulp each
NORM_BAR = COLSUM_C + ULP4              # clip norm: a fixed-order sum of (positive) squares, COLSUM_C x sum, then sqrt, a cast and a division (a few
                                        # roundings); the squared norm, the coefficient (half the sum's relative error) and g x coefficient all stay below it
ROW_BAR = 2.0 ** -19                    # constructed actor rows: neglogp is a sum of <= 4 terms of magnitude <= 4.5, each addition rounding at 2^-24: <= 2^-20
                                        # absolute in the exponent, which expf turns into a relative error of the ratio, plus expf's own 2 ulp (2^-22)
MARGIN, Table = R.MARGIN, R.Table      # device bar = MARGIN x the float32 reference's own error (kernel_refs.Table, shared with the task matrix)


def _lib():
    from emloco_amd.predictor import ops
    return ops._lib()


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


_KEEP = []      # device tensors handed to a launch as a bare pointer: kept alive until the test ends (a launch is asynchronous, and a freed
                # block may be handed to the next allocation, whose upload would then run ahead of the kernel that still reads it)


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _dev(t):
    if t is None:
        return None
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


def _out(rows, cols, ld=None, off=4):
    """a guarded [rows][cols] fp32 output holding NaN (leading dimension ld, element offset off: the default of 4 floats keeps 16-byte
    alignment and leaves a sentinel band ahead of the output as well as behind it)"""
    o = _Guarded(1, rows, cols, cols if ld is None else ld, 0, off)
    o.fill()
    return o


def _vec_out(n, off=4):
    return _out(1, n, off=off)


def _loose(val, ld, off=0):
    """val [rows][cols] placed with leading dimension ld at element offset off inside a buffer of GARBAGE"""
    rows, cols = val.shape
    buf = torch.randn(off + rows * ld + TAIL, generator=_gen(rows * 31 + cols)) * GARBAGE
    buf.as_strided((rows, cols), (ld, 1), off).copy_(val)
    return _dev(buf)


def _unaligned(t):
    """a device copy of t that starts 4 bytes past a 16-byte boundary"""
    buf = torch.full((t.numel() + 5,), GARBAGE, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    _KEEP.append(v)
    return v


def _got(o):
    torch.cuda.synchronize()
    return o.got()[0].reshape(o.shape[1:]).cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm

# (rows, d, aligned, res, dy2): d = 128 aligned = the two-rows-per-wave kernels; everything else the generic one.  rows: % 8 and % 64
# tails, one / two / three fold levels of dgamma | dbeta (row blocks of 64: <= 32 blocks, <= 1024, above)
LN_CASES = [(1, 128, 1, 1, 1), (7, 128, 1, 0, 0), (8, 128, 1, 1, 0), (9, 128, 1, 1, 1), (63, 128, 1, 1, 1), (65, 128, 1, 1, 1),
            (2048, 128, 1, 1, 1), (2049, 128, 1, 1, 0), (65537 + 64, 128, 1, 1, 1), (65, 128, 0, 1, 1), (9, 128, 0, 0, 0),
            (1, 1, 0, 1, 1), (5, 63, 0, 1, 1), (66, 64, 0, 0, 1), (67, 65, 0, 1, 0), (130, 300, 0, 1, 1), (5, 1024, 0, 1, 1),
            (2049, 33, 0, 1, 1)]


def _ln_inputs(rows, d, res, dy2, seed):
    g = _gen(seed)
    sc = 0.5 + torch.rand(rows, 1, generator=g) * 3.0                    # row variance >= 0.1 (x + res: >= 0.25 + ...)
    x = torch.randn(rows, d, generator=g) * sc + torch.randn(rows, 1, generator=g)
    r = torch.randn(rows, d, generator=g) * sc if res else None
    if d < 8:                                                             # a narrow row's sample variance can be anything: spread it
        x = x + torch.arange(d) * 1.0
    return dict(x=x, res=r, gamma=1.0 + 0.3 * torch.randn(d, generator=g), beta=0.3 * torch.randn(d, generator=g),
                dy=torch.randn(rows, d, generator=g), dy2=torch.randn(rows, d, generator=g) if dy2 else None)


def _ln_case(lib, tab, rows, d, aligned, res, dy2, fails):
    case = (rows, d, aligned, res, dy2)
    c = _ln_inputs(rows, d, res, dy2, 17 * rows + d)
    eps = 1e-5
    put = _dev if aligned else _unaligned
    x, rs, gamma, beta = put(c["x"]), (put(c["res"]) if res else None), put(c["gamma"]), put(c["beta"])
    off = 4 if aligned else 1
    if d > 1:
        xr64 = (c["x"].double() + (c["res"].double() if res else 0.0))
        assert xr64.var(dim=1, unbiased=False).min() >= 0.1
    y, mean, rstd = _out(rows, d, off=off), _vec_out(rows), _vec_out(rows)
    assert lib.emloco_layernorm_fwd(rows, d, eps, _ptr(x), _ptr(rs), _ptr(gamma), _ptr(beta), y.ptr(), mean.ptr(), rstd.ptr(), _stream()) == 0
    y2, mean2, rstd2, xr = _out(rows, d, off=off), _vec_out(rows), _vec_out(rows), _out(rows, d, off=off)
    assert lib.emloco_layernorm_fwd_save(rows, d, eps, _ptr(x), _ptr(rs), _ptr(gamma), _ptr(beta), y2.ptr(), mean2.ptr(), rstd2.ptr(),
                                         xr.ptr(), _stream()) == 0
    gy, gm, gr, gxr = _got(y), _got(mean).reshape(-1), _got(rstd).reshape(-1), _got(xr)
    if not (torch.equal(gy, _got(y2)) and torch.equal(gm, _got(mean2).reshape(-1)) and torch.equal(gr, _got(rstd2).reshape(-1))):
        fails.append((case, "fwd_save's y / mean / rstd differ from fwd's"))
    xr32 = c["x"] + c["res"] if res else c["x"]
    if not torch.equal(gxr.float(), xr32):
        fails.append((case, "xr is not the fp32 sum x + res"))
    ref = R.layernorm_fwd(c["x"], c["res"], c["gamma"], c["beta"], eps)
    r32 = R.layernorm_fwd(c["x"], c["res"], c["gamma"], c["beta"], eps, dtype=F32)
    for name, got, k in (("y", gy, 0), ("mean", gm, 1), ("rstd", gr, 2)):
        tab.add(case, name, R.err_max(got, ref[k]), R.err_max(r32[k], ref[k]))
    # backward on the device's own mean / rstd / xr (fp32 inputs of the backward; the reference takes the same values)
    dxr, dg, db = _out(rows, d, off=off), _vec_out(d), _vec_out(d)
    ws = torch.empty(lib.emloco_layernorm_bwd_workspace(rows, d) + TAIL, device=DEV)
    xr_d, dy_d, dy2_d = put(xr32), put(c["dy"]), (put(c["dy2"]) if dy2 else None)
    mean_d, rstd_d = _dev(gm.float()), _dev(gr.float())
    assert lib.emloco_layernorm_bwd2(rows, d, _ptr(xr_d), _ptr(gamma), _ptr(mean_d), _ptr(rstd_d), _ptr(dy_d), _ptr(dy2_d), dxr.ptr(),
                                     dg.ptr(), db.ptr(), _ptr(ws), _stream()) == 0
    gdx, gdg, gdb = _got(dxr), _got(dg).reshape(-1), _got(db).reshape(-1)
    dxr1, dg1, db1 = _out(rows, d, off=off), _vec_out(d), _vec_out(d)
    dsum = put(c["dy"] + c["dy2"]) if dy2 else dy_d
    assert lib.emloco_layernorm_bwd(rows, d, _ptr(xr_d), _ptr(gamma), _ptr(mean_d), _ptr(rstd_d), _ptr(dsum), dxr1.ptr(), dg1.ptr(),
                                    db1.ptr(), _ptr(ws), _stream()) == 0
    if not (torch.equal(gdx, _got(dxr1)) and torch.equal(gdg, _got(dg1).reshape(-1)) and torch.equal(gdb, _got(db1).reshape(-1))):
        fails.append((case, "layernorm_bwd2(dy, dy2) is not bit-equal to layernorm_bwd(dy + dy2)"))
    bref = R.layernorm_bwd(xr32, c["gamma"], gm, gr, c["dy"], c["dy2"])
    b32 = R.layernorm_bwd(xr32, c["gamma"], gm, gr, c["dy"], c["dy2"], dtype=F32)
    if d > 1:                                                              # (d = 1: dxr is exactly 0, nothing to scale an error by)
        tab.add(case, "dxr", R.err_max(gdx, bref[0]), R.err_max(b32[0], bref[0]))
    elif not (gdx == 0).all():                                             # xhat = 0 and g - mean(g) = 0, both exactly
        fails.append((case, "dxr of a one-element row is not 0"))
    tg, tb = R.layernorm_bwd_terms(xr32, c["gamma"], gm, gr, c["dy"], c["dy2"])
    eg, eb = R.err_terms(gdg, bref[1], tg), R.err_terms(gdb, bref[2], tb)
    if eg > COLSUM_C or eb > COLSUM_C:
        fails.append((case, "dgamma / dbeta vs float64 over sum |terms|", eg, eb))


def test_layernorm_matrix_against_float64():
    lib = _lib()
    tab, fails = Table("layernorm"), []
    for case in LN_CASES:
        _ln_case(lib, tab, *case, fails)
    assert not fails, (len(fails), fails[:10])
    tab.check()


def test_layernorm_constant_row_gives_beta():
    """a constant row has variance 0: y = beta up to the mean's rounding scaled by 1 / sqrt(eps); finite"""
    lib = _lib()
    eps = 1e-5
    for d, aligned in ((128, True), (128, False), (300, False)):
        g = _gen(d)
        x = torch.randn(9, d, generator=g)
        x[4] = 1.5
        gamma, beta = 1.0 + 0.3 * torch.randn(d, generator=g), torch.randn(d, generator=g)
        put = _dev if aligned else _unaligned
        y, mean, rstd = _out(9, d, off=4 if aligned else 1), _vec_out(9), _vec_out(9)
        assert lib.emloco_layernorm_fwd(9, d, eps, _ptr(put(x)), None, _ptr(put(gamma)), _ptr(put(beta)), y.ptr(), mean.ptr(), rstd.ptr(), _stream()) == 0
        gy = _got(y)
        assert torch.isfinite(gy).all()
        # the mean of d equal values carries <= 2^-23 of relative rounding; times rstd = 1 / sqrt(eps), times gamma
        bar = gamma.abs().double() * 2.0 ** -23 * 1.5 / eps ** 0.5 + ULP4 * beta.abs().double()
        assert ((gy[4] - beta.double()).abs() <= bar).all(), (d, aligned, (gy[4] - beta.double()).abs().max().item())
        # 1.5 d and its mean are exact, so the variance is exactly 0: rstd = 1 / sqrt(eps), three roundings (eps as float, sqrt, division)
        assert abs(_got(rstd).reshape(-1)[4].item() - eps ** -0.5) <= ULP4 * eps ** -0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax

# (n_seq, rows_per_seq, cols, bias): bias none / finite / partial -inf / one sequence fully masked; cols <= 1024 the register path
SM_CASES = [(1, 1, 1, "none"), (1, 3, 63, "finite"), (2, 2, 64, "inf"), (1, 5, 65, "none"), (3, 3, 453, "dead"), (1, 4, 1024, "inf"),
            (1, 5, 1025, "finite"), (2, 3, 1025, "dead"), (1, 2, 2500, "inf"), (3, 1, 7, "dead")]


def test_softmax_matrix_against_float64():
    lib = _lib()
    tab, fails = Table("softmax"), []
    for n_seq, rps, cols, bias in SM_CASES:
        case = (n_seq, rps, cols, bias)
        g = _gen(n_seq * 7 + rps * 3 + cols)
        rows, scale = n_seq * rps, 0.37
        S = torch.randn(rows, cols, generator=g) * 4.0
        kb = None
        if bias != "none":
            kb = torch.randn(n_seq, cols, generator=g)
            if bias in ("inf", "dead"):
                kb[0, cols // 2:] = float("-inf")
            if bias == "dead":
                kb[n_seq - 1, :] = float("-inf")
        dP = torch.randn(rows, cols, generator=g)
        ref = R.softmax_fwd(S, scale, kb, rps)
        r32 = R.softmax_fwd(S, scale, kb, rps, dtype=F32)
        for inplace in (False, True):
            P = _out(rows, cols)
            if inplace:
                P.view().copy_(_dev(S).reshape(P.shape))
                P.before = P.buf.clone()
            src = P.ptr() if inplace else _ptr(_dev(S))
            assert lib.emloco_softmax_fwd(n_seq, rps, cols, scale, src, _ptr(_dev(kb)), P.ptr(), _stream()) == 0
            gP = _got(P)
            if inplace:
                if not torch.equal(gP, gP0):
                    fails.append((case, "in-place softmax differs from out of place"))
            else:
                gP0 = gP
                tab.add(case, "P", R.err_max(gP, ref), R.err_max(r32, ref))
                if bias == "dead" and not (gP[-rps:] == 0).all():
                    fails.append((case, "a fully masked row is not all zero"))
                if bias in ("inf", "dead") and not (gP[:rps, cols // 2:] == 0).all():
                    fails.append((case, "a -inf key got probability"))
        Pd = _dev(gP0.float())
        bref = R.softmax_bwd(gP0, dP, scale)
        b32 = R.softmax_bwd(gP0.float(), dP, scale, dtype=F32)
        for inplace in (False, True):
            dS = _out(rows, cols)
            if inplace:
                dS.view().copy_(_dev(dP).reshape(dS.shape))
                dS.before = dS.buf.clone()
            src = dS.ptr() if inplace else _ptr(_dev(dP))
            assert lib.emloco_softmax_bwd(rows, cols, scale, _ptr(Pd), src, dS.ptr(), _stream()) == 0
            gS = _got(dS)
            if inplace:
                if not torch.equal(gS, gS0):
                    fails.append((case, "in-place softmax backward differs"))
            else:
                gS0 = gS
                if cols > 1:
                    tab.add(case, "dS", R.err_max(gS, bref), R.err_max(b32, bref))
                elif not (gS == 0).all():                                  # P = 1, dP - dP P = 0 exactly
                    fails.append((case, "dS of a one-key row is not 0"))
    assert not fails, (len(fails), fails[:10])
    tab.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# act_bwd, colsum, gather_flat

def test_act_bwd_equals_the_dz_of_act_bwd_colsum_and_float64():
    lib = _lib()
    for m, n, relu, p in ((1, 1, 1, 0.0), (33, 65, 1, 0.1), (257, 128, 0, 0.1), (300, 31, 1, 0.0), (1000, 7, 0, 0.25)):
        g = _gen(m + n)
        dy, y = torch.randn(m, n, generator=g), torch.randn(m, n, generator=g)
        y[::3] = 0.0
        seed = 0xABCD + m
        keep = np.zeros(m * n, np.uint8)
        assert lib.emloco_dropout_keep_mask(seed, 0, m * n, float(p), keep.ctypes.data_as(C.c_void_p)) == 0
        keep = torch.from_numpy(keep.reshape(m, n)).double()
        dz = _out(m, n)
        assert lib.emloco_act_bwd(m * n, _ptr(_dev(dy)), _ptr(_dev(y)), relu, float(p), seed, dz.ptr(), _stream()) == 0
        got = _got(dz)
        ref = R.act_bwd(dy, y, relu, keep, p)
        assert ((got - ref).abs() <= ULP4 * ref.abs()).all(), (m, n, relu, p)
        dz2, cs = _out(m, n), _vec_out(n)
        ws = torch.empty(lib.emloco_colsum_workspace(m, n) + TAIL, device=DEV)
        assert lib.emloco_act_bwd_colsum(m, n, _ptr(_dev(dy)), _ptr(_dev(y)), relu, float(p), seed, dz2.ptr(), cs.ptr(), _ptr(ws), _stream()) == 0
        assert torch.equal(_got(dz2), got), ("act_bwd differs from act_bwd_colsum's dz", m, n)
        assert R.err_terms(_got(cs).reshape(-1), got.sum(0), got.abs().sum(0)) <= COLSUM_C


def test_colsum_equals_colsum_ex_and_float64():
    lib = _lib()
    for m, n, aligned in ((1, 1, 1), (31, 64, 1), (33, 65, 1), (1025, 128, 0), (1025, 128, 1), (32769, 12, 1), (40000, 7, 1)):
        X = torch.randn(m, n, generator=_gen(m + n))
        Xd = _dev(X) if aligned else _unaligned(X)
        ws = torch.empty(lib.emloco_colsum_workspace(m, n) + TAIL, device=DEV)
        a, b = _vec_out(n), _vec_out(n)
        assert lib.emloco_colsum(m, n, _ptr(Xd), a.ptr(), _ptr(ws), _stream()) == 0
        assert lib.emloco_colsum_ex(m, n, _ptr(Xd), b.ptr(), _ptr(ws), 0, _stream()) == 0
        ga = _got(a).reshape(-1)
        assert torch.equal(ga, _got(b).reshape(-1))
        assert R.err_terms(ga, R.colsum(X), X.double().abs().sum(0)) <= COLSUM_C, (m, n, aligned)


@pytest.mark.parametrize("sizes,src_skew,dst_skew", [
    ([1, 2, 3, 4, 5, 0, 7, 1023, 1024, 1025], 0, 0), ([5, 0, 16, 33, 4099], 1, 0), ([5, 0, 16, 33, 4099], 0, 1),
    ([7] * 96 + [9], 1, 2), ([(i * 37) % 50 for i in range(200)], 3, 1), ([3, 300000, 5, 0, 64], 0, 0), ([3, 300001, 5], 1, 3)])
def test_gather_flat_copies_every_slice_and_nothing_else(sizes, src_skew, dst_skew):
    lib = _lib()
    g = _gen(len(sizes))
    pool = torch.full((sum(sizes) + 8 * len(sizes) + 16,), GARBAGE, device=DEV)
    assert pool.data_ptr() % 16 == 0
    ptrs, offs, srcs = [], [], []
    o, d = 0, dst_skew
    for i, n in enumerate(sizes):
        o = (o + 3) // 4 * 4 + (src_skew * i) % 4
        v = pool[o:o + n]
        v.copy_(torch.randn(n, generator=g) + 10.0 * (i + 1))
        srcs.append(v.clone())
        ptrs.append(pool.data_ptr() + 4 * o)
        o += n
        offs.append(d)
        d += n + 3 + (dst_skew * i) % 4
    flat = torch.full((d + TAIL,), SENT, device=DEV)
    want = flat.clone()
    for v, off in zip(srcs, offs):
        want[off:off + v.numel()] = v
    arr = (C.c_void_p * len(sizes))(*ptrs)
    numel, off_a = np.asarray(sizes, np.int64), np.asarray(offs, np.int64)
    assert lib.emloco_gather_flat(len(sizes), arr, numel.ctypes.data_as(C.c_void_p), off_a.ctypes.data_as(C.c_void_p), _ptr(flat), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(flat), _bits(want)), "a slice differs, or a gap / the tail was written"
    assert lib.emloco_gather_flat(0, None, None, None, None, _stream()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# observation normaliser, style reward, running moments

def test_obs_normalize_matrix_against_float64():
    lib = _lib()
    eps, clip = 1e-5, 5.0
    worst = 0.0
    for rows, cols, seed in OBS_CASES + [(70000, 3, 6)]:                   # (70 000 rows: above one launch's grid.y, the row stride)
        c = R.case_obs(rows, cols, seed)
        ref = R.obs_normalize(c["x"], c["mean"], c["var"], eps, clip)
        raw = (c["x"].double() - c["mean"].double()) / torch.sqrt(c["var"].double() + eps)
        near = (raw.abs() - clip).abs() < 1e-5 * clip
        assert near.double().mean().item() <= SHARE_CAP
        for split in sorted({0, cols // 3, cols}):
            ldx, ld0, ld1 = cols + 5, split + 3, cols - split + 2
            x = _loose(c["x"], ldx, off=1)
            o0, o1 = _out(rows, max(split, 1), ld=max(ld0, 1)), _out(rows, max(cols - split, 1), ld=max(ld1, 1))
            if split == 0:
                o0.view().fill_(SENT); o0.before = o0.buf.clone()
            if split == cols:
                o1.view().fill_(SENT); o1.before = o1.buf.clone()
            assert lib.emloco_obs_normalize(rows, cols, _ptr(x, 1), ldx, _ptr(_dev(c["mean"])), _ptr(_dev(c["var"])), eps, clip, split,
                                            o0.ptr(), max(ld0, 1), o1.ptr() if split < cols else None, max(ld1, 1), _stream()) == 0
            g0, g1 = _got(o0), _got(o1)
            if split == 0:
                assert (g0 == SENT).all()
            if split == cols:
                assert (g1 == SENT).all()
            got = torch.cat([g0[:, :split] if split else g0[:, :0], g1[:, :cols - split] if split < cols else g1[:, :0]], dim=1)
            assert torch.isfinite(got).all()
            err = ((got - ref).abs() / raw.abs().clamp_min(1e-30))[~near]
            worst = max(worst, err.max().item())
            assert (err <= OBS_BAR).all(), (rows, cols, split, err.max().item())
            assert ((got == clip) | (got == -clip))[(raw.abs() > clip) & ~near].all()
    print(f"\n  [obs_normalize] device error {worst:.3e} of the unclamped value (bar {OBS_BAR:.3e})")
    # an observation exactly at the clamp: (11 - 1) / sqrt(3 + 1) = 5
    o0 = _out(1, 3)
    x, mean, var = torch.tensor([[11.0, -9.0, 10.5]]), torch.ones(3), torch.full((3,), 3.0)
    assert lib.emloco_obs_normalize(1, 3, _ptr(_dev(x)), 3, _ptr(_dev(mean)), _ptr(_dev(var)), 1.0, 5.0, 3, o0.ptr(), 3, None, 0, _stream()) == 0
    assert _got(o0).tolist() == [[5.0, -5.0, 4.75]]


def test_disc_reward_against_float64():
    lib = _lib()
    tab = Table("disc_reward")
    for n in (1, 255, 256, 257, 5000):
        x = torch.rand(n, generator=_gen(n)) * 18.0 - 12.0                 # 1 - sigmoid >= 1e-3 for logits <= 6.9
        x = torch.where(x > 6.5, x - 6.0, x)
        assert (R.disc_one_minus_sigmoid(x) >= 1e-3).all()
        out = _vec_out(n, off=1)
        assert lib.emloco_disc_reward(n, _ptr(_dev(x)), 2.0, out.ptr(), _stream()) == 0
        ref, r32 = R.disc_reward(x, 2.0), R.disc_reward(x, 2.0, dtype=F32)
        tab.add(n, "reward", R.err_max(_got(out).reshape(-1), ref), R.err_max(r32, ref))
    tab.check()
    x = torch.tensor([12.0, 13.5, 20.0, 80.0, 1e30])
    out = _vec_out(5)
    assert lib.emloco_disc_reward(5, _ptr(_dev(x)), 2.0, out.ptr(), _stream()) == 0
    floor = -np.log(1e-4) * 2.0
    assert ((_got(out).reshape(-1) - floor).abs() <= ULP4 * floor).all()


RMS_ROWS = [1, 2, 3, 4, 5, 255, 256, 257, 2048, 25600]


def test_rms_update_matrix_against_float64():
    lib = _lib()
    fails = []
    for rows in RMS_ROWS:
        for cols, first_col, count in ((1, 0, 0.0), (64, 64, 5.0), (65, 7, 1.0e6), (130, 0, 300.0)):
            case = (rows, cols, first_col, count)
            g = _gen(rows * 3 + cols)
            xv = torch.randn(rows, cols, generator=g) * 3.0 + 1.0
            ldx = cols + 3
            x = _loose(xv, ldx, off=2)
            mean0, var0 = torch.randn(cols, generator=g, dtype=F64), torch.rand(cols, generator=g, dtype=F64) + 0.1
            rm, rv, rn = R.rms_update(xv, mean0, var0, count, first_col)
            outs = []
            for chunked in (False, True):
                mean, var = mean0.clone().to(DEV), var0.clone().to(DEV)
                cin, cout = torch.tensor([count], dtype=F64, device=DEV), torch.full((3,), float(SENT), dtype=F64, device=DEV)
                if chunked:
                    ws = torch.empty(lib.emloco_rms_update_workspace(rows, cols) + 64, dtype=torch.uint8, device=DEV)
                    rc = lib.emloco_rms_update_chunked(rows, cols, _ptr(x, 2), ldx, _ptr(mean), _ptr(var), _ptr(cin), _ptr(cout, 1), first_col,
                                                       _ptr(ws), _stream())
                else:
                    rc = lib.emloco_rms_update(rows, cols, _ptr(x, 2), ldx, _ptr(mean), _ptr(var), _ptr(cin), _ptr(cout, 1), first_col, _stream())
                assert rc == 0
                torch.cuda.synchronize()
                m, v, n = mean.cpu(), var.cpu(), cout.cpu()
                outs.append((m, v))
                if not (n[0] == SENT and n[2] == SENT and n[1] == rn and cin.item() == count):
                    fails.append((case, chunked, "count"))
                if not (torch.equal(m[:first_col], mean0[:first_col]) and torch.equal(v[:first_col], var0[:first_col])):
                    fails.append((case, chunked, "moments below first_col changed"))
                if first_col < cols:
                    # float64 arithmetic throughout: both are rounding-level restatements of one rule (1e-12 relative, as the header's
                    # "equal to float64 rounding"; worst-case linear growth for the tall cases: 2^-53 per addition over `rows` positive terms, for
                    # the sum of squared deviations itself and for the mean, whose error enters every deviation twice: 3 rows 2^-53)
                    em = ((m - rm).abs() / (rm.abs() + mean0.abs() + 1.0))[first_col:].max().item()
                    if rows == 1:
                        ok = torch.isnan(v[first_col:]).all().item() and em <= 1e-12
                    else:
                        ok = em <= 1e-12 and ((v - rv).abs() / rv.abs())[first_col:].max().item() <= max(1e-12, 3 * rows * 2.0 ** -53)
                    if not ok:
                        fails.append((case, chunked, "moments vs float64", em))
            if rows > 1 and first_col < cols:
                ev = ((outs[0][1] - outs[1][1]).abs() / outs[0][1].abs())[first_col:].max().item()
                if ev > 1e-12:
                    fails.append((case, "chunked vs one launch", ev))
    assert not fails, (len(fails), fails[:10])


def test_refused_calls_write_nothing():
    """host-side argument checks: a refused call returns non-zero and leaves every output as it was"""
    lib = _lib()
    z = torch.zeros(4096, device=DEV)
    # rms_update*: count_in == count_out
    mean, var, cnt = torch.ones(8, dtype=F64, device=DEV), torch.ones(8, dtype=F64, device=DEV), torch.tensor([3.0], dtype=F64, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    assert lib.emloco_rms_update(4, 8, _ptr(z), 8, _ptr(mean), _ptr(var), _ptr(cnt), _ptr(cnt), 0, _stream()) != 0
    assert lib.emloco_rms_update_chunked(4, 8, _ptr(z), 8, _ptr(mean), _ptr(var), _ptr(cnt), _ptr(cnt), 0, _ptr(ws), _stream()) != 0
    torch.cuda.synchronize()
    assert (mean == 1).all() and (var == 1).all() and cnt.item() == 3.0
    # adamw_gated: steps_in == steps_out
    p, g, m, v, st = (torch.full((16,), 2.0, device=DEV) for _ in range(5))
    assert lib.emloco_adamw_gated(16, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(st), _ptr(st), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, _stream()) != 0
    torch.cuda.synchronize()
    assert all((t == 2.0).all() for t in (p, g, m, v, st))
    # layernorm: d <= 1024 in all four entry points; 1024 itself is served (test_layernorm_matrix)
    d = 1025
    outs = [_out(2, d), _vec_out(2), _vec_out(2), _out(2, d), _vec_out(d), _vec_out(d)]
    x = torch.ones(2 * d + d, device=DEV)
    big = torch.empty(16 * d, device=DEV)
    y, mean, rstd, xr, dg, db = outs
    assert lib.emloco_layernorm_fwd(2, d, 1e-5, _ptr(x), None, _ptr(x), _ptr(x), y.ptr(), mean.ptr(), rstd.ptr(), _stream()) != 0
    assert lib.emloco_layernorm_fwd_save(2, d, 1e-5, _ptr(x), None, _ptr(x), _ptr(x), y.ptr(), mean.ptr(), rstd.ptr(), xr.ptr(), _stream()) != 0
    assert lib.emloco_layernorm_bwd(2, d, _ptr(x), _ptr(x), _ptr(x), _ptr(x), _ptr(x), y.ptr(), dg.ptr(), db.ptr(), _ptr(big), _stream()) != 0
    assert lib.emloco_layernorm_bwd2(2, d, _ptr(x), _ptr(x), _ptr(x), _ptr(x), _ptr(x), _ptr(x), y.ptr(), dg.ptr(), db.ptr(), _ptr(big), _stream()) != 0
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(_bits(o.buf), _bits(o.before))
    # chained feed-forward: F <= 2048 in the forward AND the input-gradient pass (2048 itself is served)
    M, F = 4, 2112
    w = torch.zeros(F * 128, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(F, device=DEV)
    xin = torch.zeros(M * 128, device=DEV)
    hid = torch.full((M * F,), 0x1234, dtype=torch.int16, device=DEV)
    mask = torch.full((M * F // 32,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = torch.full((M * 128,), SENT, device=DEV)
    vecs = [torch.full((M,), SENT, device=DEV) for _ in range(2)]
    colp = torch.full((8 * F,), SENT, device=DEV)
    assert lib.emloco_ffn_fwd(M, F, _ptr(xin), _ptr(w), _ptr(w), _ptr(b), _ptr(b), _ptr(hid), _ptr(mask), _ptr(out), 0.0, 1, 2, _stream()) != 0
    assert lib.emloco_ffn_fwd_norm(M, F, _ptr(xin), _ptr(w), _ptr(w), _ptr(b), _ptr(b), _ptr(hid), _ptr(mask), _ptr(xin), _ptr(b), _ptr(b), 1e-5,
                                   _ptr(out), _ptr(out), _ptr(vecs[0]), _ptr(vecs[1]), 0.0, 1, 2, _stream()) != 0
    assert lib.emloco_ffn_bwd_input(M, F, _ptr(xin), _ptr(w), _ptr(w), _ptr(mask), _ptr(hid), _ptr(out), 0.0, _stream()) != 0
    assert lib.emloco_ffn_bwd_input_colsum(M, F, _ptr(xin), _ptr(w), _ptr(w), _ptr(mask), _ptr(hid), _ptr(out), 0.0, _ptr(colp), _stream()) != 0
    torch.cuda.synchronize()
    assert (hid == 0x1234).all() and (mask == 0x5A5A5A5A).all() and (out == SENT).all() and (colp == SENT).all()
    assert all((t == SENT).all() for t in vecs)


# ---------------------------------------------------------------------------------------------------------------------------------
# LocoVal fit gradient, AdamW, clip + Adam

def test_locoval_fit_grad_matrix():
    lib = _lib()
    for n, live in ((1, 1), (1, 0), (1023, 7), (1024, 8), (1025, 9), (4096, 300), (4096, 4096), (3000, 0), (5000, 1)):
        g = _gen(n + live)
        value, target = torch.rand(n, generator=g), torch.rand(n, generator=g)
        w = torch.zeros(n)
        w[torch.randperm(n, generator=g)[:live]] = 1.0
        value[w == 0] = float("nan")                                       # a weight-0 row's value is never read into the result
        dv, tail, slot = _vec_out(n, off=1), _vec_out(2), torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
        assert lib.emloco_locoval_fit_grad(n, _ptr(_dev(value)), _ptr(_dev(target)), _ptr(_dev(w)), dv.ptr(), tail.ptr(), _ptr(slot, 4), _stream()) == 0
        rdv, rloss, rcnt, rslot = R.fit_grad(value, target, w)
        gdv, gt = _got(dv).reshape(-1), _got(tail).reshape(-1)
        s = slot.cpu()
        assert (s[:4] == -7).all() and (s[4 + n:] == -7).all() and torch.equal(s[4:4 + n], rslot), ("slot", n, live)
        assert gt[1].item() == rcnt
        assert ((gdv - rdv).abs() <= ULP4 * rdv.abs()).all() and (gdv[w == 0] == 0).all()
        terms = (w.double() * (torch.nan_to_num(value.double()) - target.double()) ** 2).sum()
        assert abs(gt[0].item() - rloss.item()) <= COLSUM_C * max(terms.item(), 1e-30), ("loss", n, live)
        tail0 = _vec_out(2)                                                # slot == NULL
        assert lib.emloco_locoval_fit_grad(n, _ptr(_dev(value)), _ptr(_dev(target)), _ptr(_dev(w)), dv.ptr(), tail0.ptr(), None, _stream()) == 0
        assert torch.equal(_got(tail0), _got(tail))


def test_adamw_gated_matrix():
    lib = _lib()
    tab = Table("adamw_gated")
    # the entry point takes float arguments: the reference gets the values the kernel receives
    lr, b1, b2, eps, wd = (float(np.float32(t)) for t in (1e-3, 0.9, 0.999, 1e-8, 1e-4))
    for n in (1, 255, 257, 6174):
        g = _gen(n)
        p0 = torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g) * (0.01 if k % 2 else 3.0) for k in range(4)]
        for gate in ("null", "open", "closed_mid"):
            P, M, V = _vec_out(n, off=1), _vec_out(n), _vec_out(n)
            P.view().copy_(_dev(p0).reshape(1, 1, n)); M.view().zero_(); V.view().zero_()
            steps = [torch.zeros(1, device=DEV), torch.full((1,), SENT, device=DEV)]
            stats = torch.zeros(5, dtype=F64, device=DEV)
            rp, rm, rv = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
            fp, fm, fv = p0.clone(), torch.zeros(n), torch.zeros(n)
            t, fits, tot = 0, 0, 0.0
            for k, gk in enumerate(grads):
                closed = gate == "closed_mid" and k in (1, 2)
                tail = None if gate == "null" else torch.tensor([0.5 + k, 0.0 if closed else 3.0], device=DEV)
                for o in (P, M, V):
                    o.before = o.buf.clone()
                assert lib.emloco_adamw_gated(n, P.ptr(), _ptr(_dev(gk)), M.ptr(), V.ptr(), _ptr(steps[k % 2]), _ptr(steps[1 - k % 2]), _ptr(tail),
                                              lr, b1, b2, eps, wd, _ptr(stats), _stream()) == 0
                torch.cuda.synchronize()
                if closed:                                                 # behind a closed gate nothing moves, bit for bit
                    assert all(torch.equal(_bits(o.buf), _bits(o.before)) for o in (P, M, V)), "a closed gate let a write through"
                else:
                    t += 1
                    rp, rm, rv = R.adamw_step(rp, gk, rm, rv, t, lr, b1, b2, eps, wd)
                    fp, fm, fv = R.adamw_step(fp, gk, fm, fv, t, lr, b1, b2, eps, wd, dtype=F32)
                    if tail is not None:
                        fits += 1; tot += 0.5 + k
                assert steps[1 - k % 2].item() == t
            st = stats.cpu()
            if gate == "null":
                assert (st == 0).all()
            else:
                assert st[4].item() == fits and st[3].item() == 3.0 * fits and st[2].item() == tot and st[1].item() == 3.0
            for name, o, ref, r32 in (("params", P, rp, fp), ("exp_avg", M, rm, fm), ("exp_avg_sq", V, rv, fv)):
                tab.add((n, gate), name, R.err_max(_got(o).reshape(-1), ref), R.err_max(r32, ref))
    tab.check()


def test_adam_clip_flat_matrix():
    lib = _lib()
    tab, fails = Table("adam_clip_flat"), []
    lr, eps = float(np.float32(1e-3)), float(np.float32(1e-8))          # float arguments; the betas travel as doubles
    b1, b2 = 0.9, 0.999
    for n, wd, max_norm, gscale in ((1, 0.0, 1.0, 3.0), (4095, float(np.float32(1e-2)), 1.0, 1.0), (4096, 0.0, 1.0, 1e-4), (4097, float(np.float32(1e-2)), 0.0, 1.0),
                                    (257 * 4096 + 5, 0.0, 1.0, 1.0), (5000, 0.0, -1.0, 1.0)):
        case = (n, wd, max_norm, gscale)
        g = _gen(n % 100000)
        p0 = torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g) * gscale for _ in range(3)]
        nws = lib.emloco_adam_clip_flat_workspace(n)
        runs = {}
        for counted in (False, True):
            P, M, V = _vec_out(n, off=1), _vec_out(n), _vec_out(n)
            P.view().copy_(_dev(p0).reshape(1, 1, n)); M.view().zero_(); V.view().zero_()
            cnt = torch.zeros(1, device=DEV)
            rp, rm, rv = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
            fp, fm, fv = p0.clone(), torch.zeros(n), torch.zeros(n)
            for t, gk in enumerate(grads, 1):
                G = _vec_out(n)
                G.view().copy_(_dev(gk).reshape(1, 1, n)); G.before = G.buf.clone()
                ws = torch.full((nws + TAIL,), SENT, device=DEV)
                if counted:
                    rc = lib.emloco_adam_clip_flat_counted(n, P.ptr(), G.ptr(), M.ptr(), V.ptr(), lr, b1, b2, eps, wd, max_norm, _ptr(ws), _ptr(cnt), _stream())
                else:
                    rc = lib.emloco_adam_clip_flat(n, P.ptr(), G.ptr(), M.ptr(), V.ptr(), lr, b1, b2, eps, wd, float(np.float32(1 - b1 ** t)),
                                                   float(np.float32(np.sqrt(1 - b2 ** t))), max_norm, _ptr(ws), _stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert (ws[nws:] == SENT).all(), "the workspace was overrun"
                rp, rg, rm, rv, norm, coef = R.adam_clip_step(rp, gk, rm, rv, t, lr, b1, b2, eps, wd, max_norm)
                fp, _, fm, fv, _, _ = R.adam_clip_step(fp, gk, fm, fv, t, lr, b1, b2, eps, wd, max_norm, dtype=F32)
                gg = _got(G).reshape(-1)
                if max_norm > 0:
                    w = ws[:2].cpu().double()
                    ss = gk.double().pow(2).sum()                      # the norm: a fixed-order sum of squares, then one sqrt
                    if abs(w[0].item() ** 2 - ss.item()) > NORM_BAR * ss.item() or abs(w[1].item() - coef.item()) > NORM_BAR * coef.item():
                        fails.append((case, counted, t, "workspace norm / coefficient", w.tolist(), norm.item(), coef.item()))
                    if coef.item() == 1.0 and not (w[1].item() == 1.0 and torch.equal(gg.float(), gk)):
                        fails.append((case, counted, t, "a coefficient of exactly 1 must leave the gradient as it is"))
                    if not ((gg - rg).abs() <= (NORM_BAR + ULP4) * rg.abs()).all():
                        fails.append((case, counted, t, "clipped gradient"))
                elif not torch.equal(gg.float(), gk):
                    fails.append((case, counted, t, "max_norm <= 0 must not touch the gradient"))
                if counted and cnt.item() != t:
                    fails.append((case, t, "step counter", cnt.item()))
            runs[counted] = [_got(o).reshape(-1) for o in (P, M, V)]
            for name, got, ref, r32 in zip(("params", "exp_avg", "exp_avg_sq"), runs[counted], (rp, rm, rv), (fp, fm, fv)):
                tab.add((case, counted), name, R.err_max(got, ref), R.err_max(r32, ref))
        # the counted variant after t calls = the plain one with the host's corrections for t (the same float32 corrections: bit-equal
        # moments; parameters within the bias corrections' own rounding, checked by the table above)
        if not (torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])):
            fails.append((case, "counted and host-corrected moments differ"))
    assert not fails, (len(fails), fails[:10])
    tab.check()
    # a NaN gradient poisons every element when clipping is on
    n = 9000
    P, M, V, G = (torch.ones(n, device=DEV) for _ in range(4))
    G[4500] = float("nan")
    ws = torch.zeros(lib.emloco_adam_clip_flat_workspace(n), device=DEV)
    assert lib.emloco_adam_clip_flat(n, _ptr(P), _ptr(G), _ptr(M), _ptr(V), lr, b1, b2, eps, 0.0, 0.1, 0.03, 1.0, _ptr(ws), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(P).all() and torch.isnan(G).all() and torch.isnan(ws[:2]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# PPO heads

def _actor_launch(lib, c, B, A, e_clip, g3, kl=True, dls=True):
    d = {k: _dev(v) for k, v in c.items()}
    rows, out5 = _out(B, 5), _vec_out(5)
    assert lib.emloco_ppo_actor_head_fwd(B, A, _ptr(d["mu"]), _ptr(d["logstd"]), _ptr(d["actions"]), _ptr(d["old_neglogp"]), _ptr(d["adv"]),
                                         _ptr(d["old_mu"]) if kl else None, _ptr(d["old_sigma"]) if kl else None, e_clip, rows.ptr(), out5.ptr(),
                                         _stream()) == 0
    dmu, dl = _out(B, A, off=1), _out(B, A, off=1)
    assert lib.emloco_ppo_actor_head_bwd(B, A, _ptr(d["mu"]), _ptr(d["logstd"]), _ptr(d["actions"]), _ptr(d["old_neglogp"]), _ptr(d["adv"]), e_clip,
                                         _ptr(_dev(g3)), dmu.ptr(), dl.ptr() if dls else None, _stream()) == 0
    torch.cuda.synchronize()
    if not dls:
        assert torch.equal(_bits(dl.buf), _bits(dl.before)), "dlogstd == NULL still wrote"
    return _got(out5).reshape(-1), _got(rows), _got(dmu), (_got(dl) if dls else None)


def test_ppo_actor_head_matrix_against_float64():
    lib = _lib()
    tab, fails = Table("ppo_actor_head"), []
    g3 = torch.tensor([1.0, -0.01, 10.0])
    for B, A in ACTOR_SHAPES + [(25600, 69), (3, 69)]:
        case = (B, A)
        c = R.case_actor(B, A, 100 + B + A)
        edge, bound = R.actor_branch_distances(c, E_CLIP)
        near = edge < 1e-5
        assert near.double().mean().item() <= SHARE_CAP and R.near_share(bound, 1.0) <= SHARE_CAP
        out5, rows, dmu, dl = _actor_launch(lib, c, B, A, E_CLIP, g3)
        ref5, rrows, _ = R.actor_head_fwd(c["mu"], c["logstd"], c["actions"], c["old_neglogp"], c["adv"], c["old_mu"], c["old_sigma"], E_CLIP)
        f5, frows, _ = R.actor_head_fwd(c["mu"], c["logstd"], c["actions"], c["old_neglogp"], c["adv"], c["old_mu"], c["old_sigma"], E_CLIP, dtype=F32)
        terms = rrows.abs().mean(dim=0)
        for k, name in ((0, "surrogate"), (1, "entropy"), (2, "bound"), (4, "kl")):
            if terms[k] > 0:
                tab.add(case, name, abs(out5[k].item() - ref5[k].item()) / terms[k].item(), abs(f5[k].item() - ref5[k].item()) / terms[k].item())
        if not torch.equal(rows[:, 3][~near], rrows[:, 3][~near]):
            fails.append((case, "clipped flags"))
        if abs(out5[3].item() - ref5[3].item()) > near.double().sum().item() / B + 2.0 ** -22:
            fails.append((case, "clipped fraction", out5[3].item(), ref5[3].item()))
        rdm, rdl = R.actor_head_bwd(c["mu"], c["logstd"], c["actions"], c["old_neglogp"], c["adv"], E_CLIP, g3)
        fdm, fdl = R.actor_head_bwd(c["mu"], c["logstd"], c["actions"], c["old_neglogp"], c["adv"], E_CLIP, g3, dtype=F32)
        keep = ~near
        tab.add(case, "dmu", R.err_max(dmu[keep], rdm[keep]), R.err_max(fdm[keep], rdm[keep]))
        tab.add(case, "dlogstd", R.err_max(dl[keep], rdl[keep]), R.err_max(fdl[keep], rdl[keep]))
        if B in (5, 257):                                                   # old_mu == NULL: KL 0; dlogstd == NULL: not written
            o5, _, dm2, _ = _actor_launch(lib, c, B, A, E_CLIP, g3, kl=False, dls=False)
            if not (o5[4] == 0 and torch.equal(o5[:4], out5[:4]) and torch.equal(dm2, dmu)):
                fails.append((case, "NULL old statistics / NULL dlogstd change the other outputs"))
    assert not fails, (len(fails), fails[:10])
    tab.check()


def test_ppo_heads_constructed_ties_and_boundaries():
    """exactly representable inputs: the device must give torch's tie and closed-interval results (kernel_refs, pinned against torch
    autograd on the same numbers by tests/test_kernel_refs_cpu.py)"""
    lib = _lib()
    a = constructed_actor()
    g3 = torch.tensor([1.0, -0.5, 2.0])
    out5, rows, dmu, dl = _actor_launch(lib, a, 6, 2, 0.25, g3)
    ref5, rrows, ratio = R.actor_head_fwd(a["mu"], a["logstd"], a["actions"], a["old_neglogp"], a["adv"], a["old_mu"], a["old_sigma"], 0.25)
    rdm, rdl = R.actor_head_bwd(a["mu"], a["logstd"], a["actions"], a["old_neglogp"], a["adv"], 0.25, g3)
    assert torch.equal(rows[:, 2:4], rrows[:, 2:4]), "bound loss / clipped flag of the constructed rows"
    # exp(+-1) and 0.5 log(2 pi) are not representable: a few float32 roundings of O(1) quantities
    assert ((rows - rrows).abs() <= ROW_BAR * rrows.abs().clamp_min(1.0)).all()
    assert ((dmu - rdm).abs() <= ROW_BAR * rdm.abs().max()).all() and ((dl - rdl).abs() <= ROW_BAR * rdl.abs().max()).all()
    # rows whose ratio is far outside the range on the side the clamp cuts carry no surrogate gradient at all
    cut = ((ratio > 1.25) & (a["adv"] > 0)) | ((ratio < 0.75) & (a["adv"] < 0))
    assert cut.any() and ((rdl - g3[1].double() / 6)[cut].abs() <= 1e-15).all() and ((dl - g3[1].double() / 6)[cut].abs() <= ULP4).all()

    c = constructed_critic()
    B = 8
    for clip_value in (0, 1):
        d = {k: _dev(v) for k, v in c.items()}
        rows, out1, dv = _vec_out(B), _vec_out(1), _vec_out(B, off=1)
        assert lib.emloco_ppo_critic_head_fwd(B, _ptr(d["v"]), _ptr(d["v_old"]), _ptr(d["ret"]), 0.25, clip_value, rows.ptr(), out1.ptr(), _stream()) == 0
        assert lib.emloco_ppo_critic_head_bwd(B, _ptr(d["v"]), _ptr(d["v_old"]), _ptr(d["ret"]), 0.25, clip_value, _ptr(_dev(torch.ones(1))), dv.ptr(),
                                              _stream()) == 0
        rl, rr = R.critic_head_fwd(c["v"], c["v_old"], c["ret"], 0.25, clip_value)
        rg = R.critic_head_bwd(c["v"], c["v_old"], c["ret"], 0.25, clip_value, torch.ones(1))
        assert torch.equal(_got(rows).reshape(-1), rr) and _got(out1).item() == rl.item(), ("critic rows / loss", clip_value)
        assert torch.equal(_got(dv).reshape(-1), rg), ("critic gradient: tie and closed-interval rules", clip_value, _got(dv), rg)

    z = torch.tensor([0.0, 0.0, -1.0, 2.0])
    rows, out4 = _out(8, 2), _vec_out(4)
    assert lib.emloco_ppo_disc_head_fwd(4, 4, _ptr(_dev(z)), _ptr(_dev(z)), rows.ptr(), out4.ptr(), _stream()) == 0
    o = _got(out4).reshape(-1)
    assert o[1] == 0.25 and o[3] == 0.25, "a logit of exactly 0 is neither < 0 nor > 0"


def test_ppo_critic_head_matrix_against_float64():
    lib = _lib()
    tab = Table("ppo_critic_head")
    for B in CRITIC_SIZES + [3, 1026]:
        c = R.case_critic(B, 200 + B)
        edge, tie = R.critic_branch_distances(c, E_CLIP)
        near = (edge < 1e-5) | (tie < 1e-5)
        assert near.double().mean().item() <= SHARE_CAP
        d = {k: _dev(v) for k, v in c.items()}
        g1 = torch.tensor([1.7])
        for clip_value in (0, 1):
            rows, out1, dv = _vec_out(B), _vec_out(1), _vec_out(B, off=1)
            vo = _ptr(d["v_old"]) if clip_value else None
            assert lib.emloco_ppo_critic_head_fwd(B, _ptr(d["v"]), vo, _ptr(d["ret"]), E_CLIP, clip_value, rows.ptr(), out1.ptr(), _stream()) == 0
            assert lib.emloco_ppo_critic_head_bwd(B, _ptr(d["v"]), vo, _ptr(d["ret"]), E_CLIP, clip_value, _ptr(_dev(g1)), dv.ptr(), _stream()) == 0
            rl, rr = R.critic_head_fwd(c["v"], c["v_old"], c["ret"], E_CLIP, clip_value)
            fl, _ = R.critic_head_fwd(c["v"], c["v_old"], c["ret"], E_CLIP, clip_value, dtype=F32)
            tab.add((B, clip_value), "loss", abs(_got(out1).item() - rl.item()) / rr.abs().mean().item(), abs(fl.item() - rl.item()) / rr.abs().mean().item())
            rg = R.critic_head_bwd(c["v"], c["v_old"], c["ret"], E_CLIP, clip_value, g1)
            fg = R.critic_head_bwd(c["v"], c["v_old"], c["ret"], E_CLIP, clip_value, g1, dtype=F32)
            keep = ~near if clip_value else torch.ones(B, dtype=torch.bool)
            if keep.any():
                tab.add((B, clip_value), "dvalues", R.err_max(_got(dv).reshape(-1)[keep], rg[keep]), R.err_max(fg[keep], rg[keep]))
    tab.check()


def test_ppo_disc_head_matrix_against_float64():
    lib = _lib()
    tab = Table("ppo_disc_head")
    for na, nd in ((1, 1), (255, 257), (256, 3), (257, 1024), (25600, 2048)):
        g = _gen(na + nd)
        a, d = torch.randn(na, generator=g) * 3, torch.randn(nd, generator=g) * 3 + 0.5
        g2 = torch.tensor([0.5, 0.25])
        rows, out4 = _out(na + nd, 2), _vec_out(4)
        assert lib.emloco_ppo_disc_head_fwd(na, nd, _ptr(_dev(a)), _ptr(_dev(d)), rows.ptr(), out4.ptr(), _stream()) == 0
        da, dd = _vec_out(na, off=1), _vec_out(nd, off=1)
        assert lib.emloco_ppo_disc_head_bwd(na, nd, _ptr(_dev(a)), _ptr(_dev(d)), _ptr(_dev(g2)), da.ptr(), dd.ptr(), _stream()) == 0
        o = _got(out4).reshape(-1)
        r4, ra, rd = R.disc_head_fwd(a, d)
        f4, _, _ = R.disc_head_fwd(a, d, dtype=F32)
        assert abs(o[1].item() - r4[1].item()) <= ULP4 and abs(o[3].item() - r4[3].item()) <= ULP4, "accuracies: counts over n, one rounding"
        for k, name, terms in ((0, "bce_agent", ra.mean()), (2, "bce_demo", rd.mean())):
            tab.add((na, nd), name, abs(o[k].item() - r4[k].item()) / terms.item(), abs(f4[k].item() - r4[k].item()) / terms.item())
        rda, rdd = R.disc_head_bwd(a, d, g2)
        fda, fdd = R.disc_head_bwd(a, d, g2, dtype=F32)
        tab.add((na, nd), "d_agent", R.err_max(_got(da).reshape(-1), rda), R.err_max(fda, rda))
        tab.add((na, nd), "d_demo", R.err_max(_got(dd).reshape(-1), rdd), R.err_max(fdd, rdd))
    tab.check()


@pytest.mark.parametrize("n_tables,n_rows", [(1, 1), (3, 5), (16, 257), (2, 5000)])
def test_ppo_gather_rows_matrix(n_tables, n_rows):
    lib = _lib()
    g = _gen(n_tables + n_rows)
    n_src = 37
    idx = torch.randint(0, n_src, (n_rows,), generator=g)
    idx[: min(n_rows, 4)] = idx[0]                                         # repeated row ids
    widths = [(1, 4, 7, 128, 69, 8, 3, 12)[t % 8] for t in range(n_tables)]
    srcs, dsts, want = [], [], []
    for t, w in enumerate(widths):
        s = torch.randn(n_src, w, generator=g)
        sd = _unaligned(s) if t % 2 else _dev(s)                           # odd tables start off 16-byte alignment
        o = _out(n_rows, w, off=(4, 1, 2)[t % 3])
        srcs.append(sd); dsts.append(o); want.append(s[idx])
    sp = (C.c_void_p * n_tables)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * n_tables)(*[o.ptr().value for o in dsts])
    cols = np.asarray(widths, np.int32)
    assert lib.emloco_ppo_gather_rows(n_tables, n_rows, _ptr(_dev(idx)), sp, dp, cols.ctypes.data_as(C.c_void_p), _stream()) == 0
    for o, w in zip(dsts, want):
        assert torch.equal(_got(o).float(), w)
    assert lib.emloco_ppo_gather_rows(17, n_rows, _ptr(_dev(idx)), sp, dp, cols.ctypes.data_as(C.c_void_p), _stream()) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# chained feed-forward (bf16 operands, fp32 accumulation; hidden and dz1 stored as bf16 once)

from test_gpu_kernel_matrix import BAR_FP32                              # noqa: E402  (fp32 accumulation: 2e-6 of sum |a b|, the header's figure)
from test_kernel_refs_cpu import FFN_CASES, LOCOVAL_CASES                  # noqa: E402

BF16_HALF_ULP = 2.0 ** -8               # round-to-nearest to 8 significant bits: at most half a spacing, <= 2^-8 of the value


def _bf16_dev(t):
    return _dev(t.to(torch.bfloat16))


def _bf16_out(rows, cols):
    """a guarded bf16 [rows][cols] output (NaN bits inside, sentinel bits in a 16-byte-aligned band ahead and behind)"""
    o = _Guarded(1, rows, cols, cols, 0, 8, bf16=True)
    o.fill()
    return o


def _decode_mask(words, M, F):
    """include/emloco_predictor.h: word (row, chunk c, h) at [row][2 c + h], bit 16 t + 4 q + e = unit 64 c + 32 t + 8 q + 4 h + e"""
    w = words.cpu().numpy().astype(np.uint32).reshape(M, F // 32)
    unit = np.zeros((M, F), bool)
    for c in range(F // 64):
        for h in range(2):
            for t in range(2):
                for q in range(4):
                    for e in range(4):
                        unit[:, 64 * c + 32 * t + 8 * q + 4 * h + e] = (w[:, 2 * c + h] >> (16 * t + 4 * q + e)) & 1
    return torch.from_numpy(unit)


def _ffn_case(lib, tab, M, F, seed, p, fails):
    case = (M, F, p)
    c = R.case_ffn(M, F, seed)
    s_h, s_o = 0x1357 + seed, 0x2468 + seed
    keep_h = keep_o = None
    if p > 0:
        kh, ko = np.zeros((M, F), np.uint8), np.zeros(M * 128, np.uint8)
        assert lib.emloco_ffn_keep_mask(s_h, 0, M, F, float(p), kh.ctypes.data_as(C.c_void_p)) == 0
        assert lib.emloco_dropout_keep_mask(s_o, 0, M * 128, float(p), ko.ctypes.data_as(C.c_void_p)) == 0
        keep_h, keep_o = torch.from_numpy(kh).double(), torch.from_numpy(ko.reshape(M, 128)).double()
    inv = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(float(p))))
    x, b1, b2 = _dev(c["x"]), _dev(c["b1"]), _dev(c["b2"])
    w1, w2 = _bf16_dev(c["w1"]), _bf16_dev(c["w2"])
    hid, out = _bf16_out(M, F), _out(M, 128)
    mask = torch.full((M * F // 32 + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    assert lib.emloco_ffn_fwd(M, F, _ptr(x), _ptr(w1), _ptr(w2), _ptr(b1), _ptr(b2), hid.ptr(), _ptr(mask, 4), out.ptr(), float(p), s_h, s_o, _stream()) == 0
    g_hid, g_out = _got(hid), _got(out)
    mw = mask.cpu()
    if not ((mw[:4] == 0x5A5A5A5A).all() and (mw[4 + M * F // 32:] == 0x5A5A5A5A).all()):
        fails.append((case, "a mask word landed outside the mask"))
    units = _decode_mask(mw[4:4 + M * F // 32], M, F)
    r_hid, r_act, _, z1 = R.ffn_fwd(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], keep_h, keep_o, p)
    xb, w1b, w2b = R.bf16_round(c["x"]), R.bf16_round(c["w1"]), R.bf16_round(c["w2"])
    mag1 = (xb.abs() @ w1b.abs().T + c["b1"].double().abs()) * inv
    # the mask against the hidden layer the same launch stored (exact), and against float64 away from the ReLU's branch point
    if not torch.equal(units, g_hid > 0):
        fails.append((case, "mask bits (header's layout) differ from (hidden > 0)"))
    near = z1.abs() < 1e-5 * z1.abs().max()
    if near.double().mean().item() > SHARE_CAP:
        fails.append((case, "too many pre-activations near 0", near.double().mean().item()))
    if not torch.equal(units[~near], r_act[~near]):
        fails.append((case, "mask differs from relu-active AND kept (float64)", (units != r_act)[~near].sum().item()))
    h_unr = z1.clamp_min(0.0) * (keep_h * inv if p > 0 else 1.0)
    if not ((g_hid - h_unr).abs() <= BF16_HALF_ULP * h_unr.abs() + (1 + BF16_HALF_ULP) * BAR_FP32 * mag1 + 1e-30)[~near].all():
        fails.append((case, "hidden is not the bf16 rounding of the float64 value (one rounding of an fp32 accumulation)"))
    # the output from the hidden layer as stored: only the fp32 accumulation of the second product is left
    r_out = (g_hid @ w2b.T + c["b2"].double()) * (keep_o * inv if p > 0 else 1.0)
    mag2 = (g_hid.abs() @ w2b.abs().T + c["b2"].double().abs()) * inv
    e_out = ((g_out - r_out).abs() / mag2.clamp_min(1e-30)).max().item()
    if not (torch.isfinite(g_out).all() and e_out <= BAR_FP32):
        fails.append((case, "out vs float64 on the rounded operands", e_out))
    if M >= 31:                                                             # (a maximum over >= 31 x 128 outputs)
        _, _, full, _ = R.ffn_fwd(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], keep_h, keep_o, p, rounded=False)
        e_full = ((g_out - full).abs() / mag2.clamp_min(1e-30)).max().item()
        if not e_full > 1e-4:
            fails.append((case, "the bf16 path is not visibly reduced precision", e_full))
    # ---- the same with the post-norm tail: xr = fp32(out + res) bit for bit (the same accumulators, one more addition); y / mean / rstd
    # against float64 LayerNorm of that xr (the row sums run in another order than emloco_layernorm_fwd_save's: not bit-equal to it)
    res, gamma, beta = _dev(c["res"]), _dev(c["gamma"]), _dev(c["beta"])
    hid2, y, xr, mean, rstd = _bf16_out(M, F), _out(M, 128), _out(M, 128), _vec_out(M), _vec_out(M)
    mask2 = torch.full_like(mask, 0x5A5A5A5A)
    assert lib.emloco_ffn_fwd_norm(M, F, _ptr(x), _ptr(w1), _ptr(w2), _ptr(b1), _ptr(b2), hid2.ptr(), _ptr(mask2, 4), _ptr(res), _ptr(gamma), _ptr(beta),
                                   1e-5, y.ptr(), xr.ptr(), mean.ptr(), rstd.ptr(), float(p), s_h, s_o, _stream()) == 0
    g_xr = _got(xr)
    if not (torch.equal(_got(hid2), g_hid) and torch.equal(mask2.cpu(), mw)):
        fails.append((case, "ffn_fwd_norm's hidden / mask differ from ffn_fwd's"))
    if not torch.equal(g_xr.float(), g_out.float() + c["res"]):
        fails.append((case, "ffn_fwd_norm's xr is not fp32(ffn_fwd's out + res)"))
    ln = R.layernorm_fwd(g_xr, None, c["gamma"], c["beta"], 1e-5)
    l32 = R.layernorm_fwd(g_xr.float(), None, c["gamma"], c["beta"], 1e-5, dtype=F32)
    for name, got, k in (("norm y", _got(y), 0), ("norm mean", _got(mean).reshape(-1), 1), ("norm rstd", _got(rstd).reshape(-1), 2)):
        tab.add(case, name, R.err_max(got, ln[k]), R.err_max(l32[k], ln[k]))
    ysave, ms, rs_, xs = _out(M, 128), _vec_out(M), _vec_out(M), _out(M, 128)
    assert lib.emloco_layernorm_fwd_save(M, 128, 1e-5, out.ptr(), _ptr(res), _ptr(gamma), _ptr(beta), ysave.ptr(), ms.ptr(), rs_.ptr(), xs.ptr(), _stream()) == 0
    if not torch.equal(_got(xs), g_xr):
        fails.append((case, "ffn_fwd -> layernorm_fwd_save gives another xr than ffn_fwd_norm"))
    tab.add(case, "norm y (2 launches)", R.err_max(_got(ysave), ln[0]), R.err_max(l32[0], ln[0]))
    # ---- input-gradient pass on the forward's mask
    dz2 = _dev(c["dz2"])
    w2t, w1t = _bf16_dev(c["w2"].T.contiguous()), _bf16_dev(c["w1"].T.contiguous())
    dz1, dx = _bf16_out(M, F), _out(M, 128)
    assert lib.emloco_ffn_bwd_input(M, F, _ptr(dz2), _ptr(w2t), _ptr(w1t), _ptr(mask, 4), dz1.ptr(), dx.ptr(), float(p), _stream()) == 0
    g_dz1, g_dx = _got(dz1), _got(dx)
    d_unr = (R.bf16_round(c["dz2"]) @ w2b) * units.double() * inv
    magd = (R.bf16_round(c["dz2"]).abs() @ w2b.abs()) * inv
    if not ((g_dz1 - d_unr).abs() <= BF16_HALF_ULP * d_unr.abs() + (1 + BF16_HALF_ULP) * BAR_FP32 * magd + 1e-30).all():
        fails.append((case, "dz1 is not the bf16 rounding of (dz2 w2) o mask / (1 - p)"))
    if not (g_dz1[~units] == 0).all():
        fails.append((case, "dz1 is not 0 where the mask is clear"))
    r_dx, magx = g_dz1 @ w1b, g_dz1.abs() @ w1b.abs()
    e_dx = ((g_dx - r_dx).abs() / magx.clamp_min(1e-30)).max().item()
    if not (torch.isfinite(g_dx).all() and e_dx <= BAR_FP32):
        fails.append((case, "dx vs float64 on dz1 as stored", e_dx))
    nrows = lib.emloco_ffn_bwd_colsum_rows(M)
    dz1c, dxc, colp = _bf16_out(M, F), _out(M, 128), _out(nrows, F)
    assert lib.emloco_ffn_bwd_input_colsum(M, F, _ptr(dz2), _ptr(w2t), _ptr(w1t), _ptr(mask, 4), dz1c.ptr(), dxc.ptr(), float(p), colp.ptr(), _stream()) == 0
    if not (torch.equal(_got(dz1c), g_dz1) and torch.equal(_got(dxc), g_dx)):
        fails.append((case, "bwd_input_colsum's dz1 / dx differ from bwd_input's"))
    g_cp = _got(colp)
    live = (M + 31) // 32
    if not (g_cp[live:] == 0).all():
        fails.append((case, "colpart rows of waves past the last row are not exactly zero"))
    for wv in range(live):                                                  # every wave's row: the column sums of its own 32 rows
        blk = g_dz1[32 * wv:32 * wv + 32]
        if R.err_terms(g_cp[wv], blk.sum(0), blk.abs().sum(0).clamp_min(1e-30)) > COLSUM_C:
            fails.append((case, "colpart row vs float64 column sum of dz1 as stored", wv))
            break
    if R.err_terms(g_cp.sum(0), g_dz1.sum(0), g_dz1.abs().sum(0).clamp_min(1e-30)) > COLSUM_C:
        fails.append((case, "colpart summed over rows vs float64 column sum of dz1 as stored"))


def test_ffn_matrix_against_float64():
    """F = 64 (one chunk) .. 2048 (the limit, served), M over the wave and workgroup tails, with and without dropout"""
    lib = _lib()
    tab, fails = Table("ffn"), []
    for M, F, seed in FFN_CASES:
        for p in ((0.0, 0.1) if M in (33, 255, 257) else (0.0,)):
            _ffn_case(lib, tab, M, F, seed, p, fails)
    assert not fails, (len(fails), fails[:10])
    tab.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# LocoVal MLP with yaw normalisation

def _locoval_inputs(B, stride, seed):
    """case_locoval plus the constructed guard rows: x of waypoint 1 exactly 0, and +-5e-11 (inside |x| < 1e-10)"""
    c = R.case_locoval(B, stride, seed)
    for row, xv in ((0, 0.0), (1, 5e-11), (2, -5e-11)):
        if row < B:
            c["traj"][row, 1, 0] = xv
    return c


def _lv_fwd(lib, d, B, stride, weight=None, prefill=None, rows_entry=True):
    outs = [_vec_out(B), _out(B, 100), _out(B, 49), _out(B, 24), _vec_out(B)]
    if prefill is not None:
        for o, v in zip(outs, prefill):
            o.view().copy_(_dev(v).reshape(o.shape)); o.before = o.buf.clone()
    args = [B, _ptr(d["traj"]), stride, _ptr(d["pose"]), _ptr(d["vel"])] + [_ptr(t) for t in d["params"]] + [o.ptr() for o in outs]
    if rows_entry:
        assert lib.emloco_locoval_fwd_rows(*args, _ptr(weight), _stream()) == 0
    else:
        assert lib.emloco_locoval_fwd(*args, _stream()) == 0
    return [_got(o) for o in outs]


def _lv_bwd(lib, d, B, stride, fwd, dvalue, slot=None, count=None, prefill_dtraj=None):
    dp, dt = _vec_out(6174), _out(B, 13 * stride)
    if prefill_dtraj is not None:
        dt.view().copy_(_dev(prefill_dtraj).reshape(dt.shape)); dt.before = dt.buf.clone()
    ws = torch.full((B * 6174 + TAIL,), float("nan"), device=DEV)
    _KEEP.append(ws)
    f = [_dev(t.float().contiguous()) for t in fwd]
    head = [B, _ptr(d["traj"]), stride, _ptr(d["pose"]), _ptr(d["vel"]), _ptr(d["params"][0]), _ptr(d["params"][2]), _ptr(d["params"][4])]
    mid = [_ptr(f[0]), _ptr(f[1]), _ptr(f[2]), _ptr(f[3]), _ptr(f[4]), _ptr(_dev(dvalue))]
    if slot is None:
        assert lib.emloco_locoval_bwd(*head, *mid, dp.ptr(), dt.ptr(), _ptr(ws), _stream()) == 0
    else:
        assert lib.emloco_locoval_bwd_rows(*head, *mid, _ptr(_dev(slot)), _ptr(_dev(count)), dp.ptr(), dt.ptr(), _ptr(ws), _stream()) == 0
    return _got(dp).reshape(-1), _got(dt).reshape(B, 13, stride)


def test_locoval_matrix_against_float64():
    lib = _lib()
    tab, fails = Table("locoval"), []
    for B, stride, seed in LOCOVAL_CASES:
        case = (B, stride)
        c = _locoval_inputs(B, stride, seed)
        z1, z2 = R.locoval_branch_distances(c)
        # the backward sums every row into dparams, so no row may sit on a ReLU's branch point at all (the seeds are chosen for it)
        assert not (z1.abs() < 1e-5 * z1.abs().max()).any() and not (z2.abs() < 1e-5 * z2.abs().max()).any()
        d = dict(traj=_dev(c["traj"]), pose=_dev(c["pose"]), vel=_dev(c["vel"]), params=[_dev(t) for t in c["params"]])
        ref = R.locoval_fwd(c["traj"], c["pose"], c["vel"], c["params"])
        r32 = R.locoval_fwd(c["traj"], c["pose"], c["vel"], c["params"], dtype=F32)
        fwd = _lv_fwd(lib, d, B, stride, rows_entry=False)
        got = [fwd[0].reshape(-1), fwd[1], fwd[2], fwd[3], fwd[4].reshape(-1)]
        for name, g_, k in (("value", got[0], 0), ("x100", got[1], 1), ("h1", got[2], 2), ("h2", got[3], 3), ("angle", got[4], 4)):
            tab.add(case, name, R.err_max(g_, ref[k]), R.err_max(r32[k], ref[k]))
        hidden_cols = [26 + 3 * j + k for j in R.LV_HIDDEN_JOINTS for k in range(3)]
        if not (got[1][:, hidden_cols] == 0).all():
            fails.append((case, "hidden joints are not zero in x100"))
        same = _lv_fwd(lib, d, B, stride, weight=None)
        if not all(torch.equal(a, b) for a, b in zip(same, fwd)):
            fails.append((case, "fwd_rows(NULL weights) differs from fwd"))
        # sparse forward: rows with weight 0 keep what they held, bit for bit; the others are fwd's
        g = _gen(seed + 50)
        for live in sorted({0, 1, min(B, 7), min(B, 8), min(B, 9), B}):
            w = torch.zeros(B)
            w[torch.randperm(B, generator=g)[:live]] = torch.rand(live, generator=g) + 0.5
            pre = [torch.randn(t.shape, generator=g) for t in fwd]
            sp = _lv_fwd(lib, d, B, stride, weight=_dev(w), prefill=pre)
            on = w != 0
            for k in range(4):                                               # value, x100, h1, h2 (angle is scratch for the backward)
                a, b_, p_ = sp[k].reshape(B, -1), fwd[k].reshape(B, -1), pre[k].reshape(B, -1).double()
                if not (torch.equal(a[on], b_[on]) and torch.equal(a[~on], p_[~on])):
                    fails.append((case, live, "sparse forward: live rows differ from fwd, or a weight-0 row was written", k))
        # backward on the device's own forward results
        bref = R.locoval_bwd(c["traj"], c["pose"], c["vel"], c["params"], c["dvalue"])
        b32 = R.locoval_bwd(c["traj"], c["pose"], c["vel"], c["params"], c["dvalue"], dtype=F32)
        terms = R.locoval_bwd_terms(c["traj"], c["pose"], c["vel"], c["params"], c["dvalue"])
        dp, dt = _lv_bwd(lib, d, B, stride, got, c["dvalue"])
        tab.add(case, "dparams", R.err_terms(dp, bref[0], terms), R.err_terms(b32[0], bref[0], terms))
        tab.add(case, "dtraj", R.err_max(dt, bref[1]), R.err_max(b32[1], bref[1]))
        if stride > 2 and not (dt[:, :, 2:] == 0).all():
            fails.append((case, "d traj beyond (x, y) is not zero"))
        # the guard of waypoint 1: the guarded x gets the rotation's gradient only (float64 autograd of where(|x| < 1e-10, 1e-10, x))
        for row in range(min(B, 3)):
            if abs(dt[row, 1, 0].item() - bref[1][row, 1, 0].item()) > MARGIN * max(R.err_max(b32[1], bref[1]), ULP4) * bref[1].abs().max().item():
                fails.append((case, "gradient at the guarded x of waypoint 1", row, dt[row, 1, 0].item(), bref[1][row, 1, 0].item()))
        full_slot, full_cnt = torch.arange(B, dtype=torch.int32), torch.tensor([float(B)])
        dp2, dt2 = _lv_bwd(lib, d, B, stride, got, c["dvalue"], slot=full_slot, count=full_cnt)
        if not (torch.equal(dp2, dp) and torch.equal(dt2, dt)):
            fails.append((case, "bwd_rows with every row live differs from bwd"))
        for live in sorted({0, 1, min(B, 7), min(B, 8), min(B, 9)}):
            w = torch.zeros(B)
            w[torch.randperm(B, generator=g)[:live]] = 1.0
            on = w != 0
            dv = c["dvalue"] * w
            slot = R.fit_grad(torch.zeros(B), torch.zeros(B), w)[3]
            pre = torch.randn(B, 13, stride, generator=g)
            dp3, dt3 = _lv_bwd(lib, d, B, stride, got, dv, slot=slot, count=torch.tensor([float(live)]), prefill_dtraj=pre)
            if not (torch.equal(dt3[on], dt[on]) and torch.equal(dt3[~on], pre[~on].double())):
                fails.append((case, live, "sparse backward: d traj of a live row differs from bwd's, or a row without a slot was written"))
            if live == 0:
                if not (dp3 == 0).all():
                    fails.append((case, live, "no live row: dparams must be exactly 0"))
                continue
            sref = R.locoval_bwd(c["traj"], c["pose"], c["vel"], c["params"], dv)
            s32 = R.locoval_bwd(c["traj"], c["pose"], c["vel"], c["params"], dv, dtype=F32)
            sterms = R.locoval_bwd_terms(c["traj"][on], c["pose"][on], c["vel"][on], c["params"], dv[on])
            tab.add((case, live), "dparams", R.err_terms(dp3, sref[0], sterms), R.err_terms(s32[0], sref[0], sterms))
    assert not fails, (len(fails), fails[:10])
    tab.check()

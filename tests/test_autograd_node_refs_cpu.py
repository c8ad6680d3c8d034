"""CPU companion of tests/test_gpu_autograd_nodes.py: the references, the case table and the bars of tests/autograd_node_cases.py,
without a device.

1. The closed-form float64 references equal stock torch in float64 autograd (F.linear + F.relu + an explicit mask, F.layer_norm on
   x + res, softmax attention with an additive key bias and a given keep mask, the two-layer feed-forward).
2. Every case's advertised branch follows from the pure predicates of ops.py (_ksplit_for, _ffn_chain_ok, the two padding conditions,
   the chunk sizes for a MAX_SEQ_HEADS), evaluated on the host.
3. Every bar is met with margin (half of it) by a float32 stock-torch evaluation of the same case: a case whose own float32 evaluation
   would not meet its bar is a badly chosen input, not a finding about the device.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F                                                  # noqa: E402

import autograd_node_cases as A                                                  # noqa: E402
import kernel_refs as R                                                          # noqa: E402
from kernel_matrix_cases import BAR_FP32, _attn_reference, _key_bias, _p8, attn_bar_ratios, attn_mags      # noqa: E402

MARGIN = 0.5


def _margin(rounded):
    """half the bar for the fp32 classes; the whole bar where operands or stores are rounded to bf16 -- half a bf16 spacing, 2^-8 of the
    value, is a bound that single elements attain, not a statistical figure that leaves room"""
    return 1.0 if rounded else MARGIN
NO_RND = {k: False for k in ("fwd", "dx", "dw", "h", "f", "dw2", "dz1", "dw1")}
ALL_RND = {k: True for k in NO_RND}


def _keep(shape, p, seed):
    if p == 0.0:
        return None
    return (torch.rand(shape, generator=A.gen(seed)) >= p).double() / (1.0 - p)


def _close(got, want, tol, what):
    err = (got - want).abs()
    assert (err <= tol).all(), (what, err.max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the references

def test_linear_reference_equals_float64_autograd():
    for c in A.linear_cases():
        if c.name not in ("base", "kpad", "narrow"):
            continue
        inp = {k: (v.double() if v is not None else None) for k, v in c.inputs().items()}
        keep_s = _keep((c.M, c.N), c.p, c.M + c.N)
        leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "W", "b") if inp[k] is not None]
        y = F.linear(*leaves)
        if c.relu:
            y = F.relu(y)
        if keep_s is not None:
            y = y * keep_s
        grads = torch.autograd.grad(y, leaves, inp["dy"])
        ref = A.linear_reference(inp, c.relu, keep_s, y.detach() > 0, c.p, NO_RND, BAR_FP32, BAR_FP32)
        _close(ref["y"][0], y.detach(), 1e-12 * c.x_scale, (c, "y"))
        for name, g in zip(("dx", "dW", "db"), grads):
            # (the reference scales by the float32 value of 1 / (1 - p), as the kernels do: 2^-24 of the value away from float64's)
            tol = 1e-12 * c.x_scale + (A.MASK_PASS * g.abs().max() if keep_s is not None else 0.0)
            _close(ref[name][0], g, tol, (c, name))


def test_feed_forward_reference_equals_float64_autograd():
    for c in A.ffn_cases():
        if c.M > 200:
            continue
        inp = {k: v.double() for k, v in c.inputs().items()}
        k1s, k2s = _keep((c.M, c.F), c.p, 1), _keep((c.M, c.N), c.p, 2)
        leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "W1", "b1", "W2", "b2")]
        h = F.relu(F.linear(leaves[0], leaves[1], leaves[2]))
        h = h * k1s if k1s is not None else h
        f = F.linear(h, leaves[3], leaves[4])
        f = f * k2s if k2s is not None else f
        grads = torch.autograd.grad(f, leaves, inp["df"])
        ref = A.ffn_reference(inp, k1s, k2s, h.detach(), c.p, NO_RND, False, BAR_FP32, BAR_FP32)
        _close(ref["h"][0], h.detach(), 1e-12, (c, "h"))
        _close(ref["f"][0], f.detach(), 1e-12, (c, "f"))
        for name, g in zip(("dx", "dW1", "db1", "dW2", "db2"), grads):
            _close(ref[name][0], g, 1e-12 + (2 * A.MASK_PASS * g.abs().max() if c.p > 0 else 0.0), (c, name))


def test_layer_norm_reference_equals_float64_autograd():
    for rows, d in ((1, 128), (257, 20), (5, 1024)):
        c = {k: v.double() for k, v in A.ln_inputs(rows, d).items()}
        x, res, gamma, beta = (c[k].clone().requires_grad_(True) for k in ("x", "res", "gamma", "beta"))
        y = F.layer_norm(x + res, (d,), gamma, beta, 1e-5)
        gx, gr, gg, gb = torch.autograd.grad(y, [x, res, gamma, beta], c["dy"] + c["dy2"])
        ry, mean, rstd, xr = R.layernorm_fwd(c["x"], c["res"], c["gamma"], c["beta"], 1e-5)
        dxr, dg, db = R.layernorm_bwd(xr, c["gamma"], mean, rstd, c["dy"], c["dy2"])
        _close(ry, y.detach(), 1e-12, "y")
        for got, want, what in ((dxr, gx, "dx"), (dxr, gr, "dres"), (dg, gg, "dgamma"), (db, gb, "dbeta")):
            _close(got, want, 1e-11, (rows, d, what))
        # the same tensor as x and res: autograd hands it both edges' gradients
        t = c["x"].clone().requires_grad_(True)
        (g2,) = torch.autograd.grad(F.layer_norm(t + t, (d,), c["gamma"], c["beta"], 1e-5), [t], c["dy"])
        _, m2, r2, xr2 = R.layernorm_fwd(c["x"], c["x"], c["gamma"], c["beta"], 1e-5)
        _close(2.0 * R.layernorm_bwd(xr2, c["gamma"], m2, r2, c["dy"])[0], g2, 1e-11, "x twice")


def _stock_attention(qkv, kb, H, dh, nq, keepm, dout):
    """softmax attention with stock torch ops on a leaf qkv -> (out, dqkv)"""
    Bn, S, _ = qkv.shape
    d = H * dh
    leaf = qkv.clone().requires_grad_(True)
    q, k, v = (leaf[..., i * d:(i + 1) * d].reshape(Bn, S, H, dh).transpose(1, 2) for i in range(3))
    s = q[:, :, :nq] @ k.transpose(-1, -2) / dh ** 0.5
    if kb is not None:
        s = s + kb.to(s.dtype)[:, None, None, :]
    dead = torch.isneginf(s).all(-1, keepdim=True)
    P = torch.where(dead, torch.zeros_like(s), torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1))
    if keepm is not None:
        P = P * keepm.to(s.dtype)
    out = (P @ v).transpose(1, 2).reshape(Bn, nq, d)
    (g,) = torch.autograd.grad(out, [leaf], dout)
    return out.detach(), g


@pytest.mark.parametrize("kind", A.ATTN_BIAS)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_reference_equals_float64_autograd(kind, p):
    Bn, S, H = 3, 33, 4
    for nq in (1, 21, 33):
        g = A.gen(S + nq + len(kind))
        qkv = (torch.randn(Bn, S, 3 * 32 * H, generator=g) * 0.6).double()
        dout = torch.randn(Bn, nq, 32 * H, generator=g).double()
        kb = _key_bias(kind, Bn, S, 17, "cpu")
        keep = (torch.rand(Bn, H, nq, S, generator=g) >= p).double() if p > 0 else None
        out, dqkv = _stock_attention(qkv, kb, H, 32, nq, keep / (1.0 - _p8(p)) if keep is not None else None, dout)
        r_out, _, r_dqkv, _ = _attn_reference(qkv, kb, H, nq, keep, p, dout)
        _close(r_out, out, 1e-12, ("out", kind, nq))
        _close(r_dqkv, dqkv, 1e-11, ("dqkv", kind, nq))


@pytest.mark.parametrize("H,dh", [(4, 16), (2, 20)])
def test_embedded_attention_reference_equals_float64_autograd_at_other_head_dims(H, dh):
    Bn, S = 3, 21
    g = A.gen(H + dh)
    qkv = (torch.randn(Bn, S, 3 * H * dh, generator=g) * 0.6).double()
    dout = torch.randn(Bn, S, H * dh, generator=g).double()
    out, dqkv = _stock_attention(qkv, None, H, dh, S, None, dout)
    q32, do32, c = A.embed32(qkv, dout, H, dh)
    r_out, _, r_dqkv, _ = _attn_reference(q32, None, H, S, None, 0.0, do32)
    e_out, e_dqkv = A.unembed32(r_out, r_dqkv, H, dh, c)
    _close(e_out, out, 1e-12, "out")
    _close(e_dqkv, dqkv, 1e-11, "dqkv")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the case table against the predicates of ops.py

def test_the_predicates_restated_for_the_case_table_are_those_of_ops():
    from emloco_amd.predictor import ops
    for red in (1, 20, 255, 256, 511, 512, 515, 1030, 4096, 300000):
        for out_elems in (1, 320, 720, 16384, 16385, 10 ** 6, 10 ** 8):
            assert A.ksplit_for(red, out_elems) == ops._ksplit_for(red, out_elems)
    before = ops.get_matmul_precision()
    try:
        for mode in A.MODES:
            ops.set_matmul_precision({"split3": "fp32_split", "split2": "fp32_split"}.get(mode, mode))
            for K, F_, N in ((128, 64, 128), (128, 2048, 128), (128, 96, 128), (128, 2112, 128), (20, 36, 20), (64, 72, 64), (128, 32, 128), (128, 64, 64)):
                assert bool(ops._ffn_chain_ok(1, K, F_, N)) == A.ffn_chain_ok(mode, K, F_, N), (mode, K, F_, N)
    finally:
        ops.set_matmul_precision(before)
    assert ops.FusedAttentionFn.MAX_SEQ_HEADS == 65535
    assert (ops.GEMM_ACC, ops.GEMM_SPLIT2) == (A.GEMM_ACC, A.GEMM_SPLIT2)


def test_every_linear_case_reaches_the_branch_it_names():
    cases = A.linear_cases()
    seen = set()
    for c in cases:
        kf, kx, kw = c.ksplits()
        e = c.expect
        if "ksplit" in e:
            assert {"fwd": kf, "dx": kx, "dw": kw}[e["ksplit"]] > 1, c
            seen.add((e["ksplit"], {"fwd": kf, "dx": kx, "dw": kw}[e["ksplit"]]))
        if "kpad" in e:
            assert A.pads_k(c.K) == e["kpad"] and (c.Kp != c.K) == e["kpad"] and c.Kp % 4 == 0 or not e["kpad"], c
        if "npad" in e:
            assert A.pads_n(c.N, c.M) == e["npad"] and (c.Np == 36) == e["npad"], c
        if "narrow" in e:
            assert c.N <= 32
        if "act" in e:
            seen.add(e["act"])
    assert {("fwd", 2), ("fwd", 4), ("dx", 2), ("dw", 2), ("dw", 4)} <= seen
    assert {"emloco_act_bwd_colsum", "emloco_act_bwd", "emloco_colsum_ex", None} <= seen        # the four mask / bias branches of the backward
    assert [A.pads_k(K) for K in (255, 256, 257, 258)] == [False, False, True, True]
    # the base grid: relu x dropout x bias x every subset of needs_input_grad
    base = {(c.relu, c.p, c.bias, c.needs) for c in cases if c.name == "base"}
    assert len(base) == 4 * (5 + 3)


def test_every_feed_forward_case_reaches_the_branch_it_names():
    for c in A.ffn_cases():
        for mode in c.modes:
            if "chain" in c.expect:
                assert c.chained(mode) == c.expect["chain"], (c, mode)
            if c.expect.get("dw_ksplit"):
                assert A.ksplit_for(c.M, c.F * c.K) > 1 and A.ksplit_for(c.M, c.N * c.F) > 1, c
    small = A.FfnCase("plain", 33, 20, 36, 20)
    assert not small.h16("bf16") and not small.chained("bf16")                  # the small model keeps an fp32 hidden layer
    assert A.FfnCase("plain", 130, 64, 72, 64).h16("bf16") and A.FfnCase("plain", 515, 128, 64, 128).chained("bf16")
    assert not A.ffn_chain_ok("bf16", 128, 96, 128) and not A.ffn_chain_ok("bf16", 128, 2112, 128) and A.ffn_chain_ok("bf16", 128, 2048, 128)


def test_the_attention_chunks_of_the_cases():
    assert A.chunks(5, 4, 9) == [(0, 2), (2, 2), (4, 1)]
    assert A.chunks(16384, 4, 65535) == [(0, 16383), (16383, 1)]
    assert A.chunks(3, 4, 65535) == [(0, 3)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the bars against a float32 evaluation of the same cases

@pytest.mark.parametrize("rounded", [False, True])
def test_a_float32_linear_meets_every_bar_with_margin(rounded):
    rat = A.Ratios("linear float32" + (" on bf16 operands" if rounded else ""))
    rnd = ALL_RND if rounded else NO_RND
    for c in A.linear_cases():
        if c.out_bf16 and not rounded:
            continue
        inp = c.inputs()
        keep_s = _keep((c.M, c.N), c.p, c.M + c.N)
        got, act = A.linear_float32(inp, c.relu, keep_s, c.p, rnd, y16=c.out_bf16)
        ref = A.linear_reference({k: (v.double() if v is not None else None) for k, v in inp.items()}, c.relu, keep_s, act, c.p, rnd, BAR_FP32, BAR_FP32,
                                 y16=c.out_bf16)
        for name in ("y", "dx", "dW", "db"):
            rat.add(c, name, got[name], ref[name][0], ref[name][1] * _margin(rounded))
    rat.check()


@pytest.mark.parametrize("rounded", [False, True])
def test_a_float32_feed_forward_meets_every_bar_with_margin(rounded):
    rat = A.Ratios("ffn float32" + (" on bf16 operands" if rounded else ""))
    rnd = ALL_RND if rounded else NO_RND
    for c in A.ffn_cases():
        inp = c.inputs()
        k1s, k2s = _keep((c.M, c.F), c.p, 1), _keep((c.M, c.N), c.p, 2)
        h16 = rounded and c.h16("bf16")
        got = A.ffn_float32(inp, k1s, k2s, c.p, rnd, h16)
        ref = A.ffn_reference({k: v.double() for k, v in inp.items()}, k1s, k2s, got["h"].double(), c.p, rnd, h16, BAR_FP32, BAR_FP32)
        for name in ("h", "f", "dx", "dW1", "db1", "dW2", "db2"):
            rat.add(c, name, got[name], ref[name][0], ref[name][1] * _margin(rounded))
    rat.check()


def test_a_float32_attention_meets_every_bar_with_margin():
    Bn, S, H = 3, 33, 4
    worst = {}
    for kind in A.ATTN_BIAS:
        for nq in (1, 21, 33):
            for p in (0.0, 0.1):
                g = A.gen(S + nq + len(kind))
                qkv = torch.randn(Bn, S, 3 * 32 * H, generator=g) * 0.6
                dout = torch.randn(Bn, nq, 32 * H, generator=g)
                kb = _key_bias(kind, Bn, S, 17, "cpu")
                keep = (torch.rand(Bn, H, nq, S, generator=g) >= p).double() if p > 0 else None
                out, dqkv = _stock_attention(qkv, kb, H, 32, nq, keep / (1.0 - _p8(p)) if keep is not None else None, dout)
                ref = _attn_reference(qkv.double(), kb, H, nq, keep, p, dout.double())
                mags = attn_mags(qkv.double(), kb, H, nq, keep, p, dout.double())
                el = attn_bar_ratios((out.double(), ref[3], dqkv.double()), (ref[0], ref[3], ref[2]), mags, 32 * H, BAR_FP32)
                for k_, v in el.items():
                    worst[k_] = max(worst.get(k_, 0.0), v)
    print("\n  [attention float32]", {k_: round(v, 3) for k_, v in worst.items()})
    assert all(v <= MARGIN for v in worst.values()), worst


def test_a_float32_layer_norm_has_a_measurable_error_on_every_case():
    """the layer norm's bars are MARGIN x the float32 evaluation's own error (kernel_refs.Table): that error must not vanish"""
    for d in A.LN_D:
        for rows in A.LN_ROWS:
            c = A.ln_inputs(rows, d)
            ref = R.layernorm_fwd(c["x"], c["res"], c["gamma"], c["beta"], 1e-5)
            r32 = R.layernorm_fwd(c["x"], c["res"], c["gamma"], c["beta"], 1e-5, dtype=torch.float32)
            assert 0 < R.err_max(r32[0], ref[0]) < 1e-5, (rows, d)
            xr = c["x"] + c["res"]
            assert xr.double().var(dim=1, unbiased=False).min() >= 0.1 if d > 1 else True

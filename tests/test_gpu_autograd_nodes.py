"""Device matrix of the predictor's autograd nodes (emloco_amd/predictor/ops.py) against float64 (tests/autograd_node_cases.py).

The kernel matrices call the C entry points; this one drives the layer above them -- `linear`, `relu_mask`, `feed_forward`,
`feed_forward_norm`, `layer_norm`, `attention` and the direct-gradient path of `mark_direct_grad` -- through the public wrappers (or
`Fn.apply` where a seed must be explicit), with torch.autograd.grad / .backward on a random dy, and judges every output and every
requested gradient element by element: |got - ref| <= eps x mag + carried (the cases module derives the bars).  Every case also takes
a census of the launches the node made and asserts the branch it was written for (reduction split, padded K / N, GEMM_ACC, which mask
launch, chained launch or two GEMMs, the number of attention launches), so a case that stops reaching its branch fails.

Modes: fp32, fp32_split with three and with two backward pieces, bf16 (the fused attention's backward pieces are a load-time knob of
the library, not of ops.py: it runs in fp32, split and bf16, the split bar following what the library reports).

Measured worst error / bar (MI355X, the run that accompanied this file; printed by every run, `pytest -s`):

    family                     mode     y / h    f        dx       dW / dW1   dW2      db / db1   db2
    linear                     fp32     0.154    --       0.162    0.130      --       0.009      --
    linear                     split3   0.112    --       0.162    0.099      --       0.009      --
    linear                     split2   0.105    --       0.173    0.429      --       0.009      --
    linear                     bf16     0.993    --       0.162    0.092      --       0.009      --
    direct gradient (a)-(h)    all      --       --       --       <= 0.096   --       <= 0.005   --
    feed_forward               fp32     0.115    0.129    0.019    0.023      0.111    0.006      0.007
    feed_forward               split3   0.103    0.154    0.019    0.020      0.100    0.006      0.006
    feed_forward               split2   0.103    0.130    0.030    0.041      0.172    0.025      0.004
    feed_forward               bf16     0.993    0.082    0.501    0.940      0.074    0.939      0.007
    fall-back vs chained       bf16     --       0.186    0.208    0.236      0.270    0.230      0.000
    feed_forward_norm          bf16     0.956    0.063    0.489    0.872      0.033    0.870      0.008

    layer_norm / feed_forward_norm's norm (8 x the float32 evaluation's error):  y 1.6e-7 of a bar of 1.7e-6, dxr 1.1e-7 of 9.0e-7

    attention                  mode     out      dq       dk       dv
    fused                      fp32     0.034    0.015    0.026    0.091
    fused                      split    0.028    0.012    0.036    0.127
    fused                      bf16     0.172    0.069    0.053    0.148
    chunks 2 + 2 + 1           fp32     0.027    0.010    0.008    0.039
    chunks 2 + 2 + 1           split    0.030    0.011    0.006    0.026
    chunks 2 + 2 + 1           bf16     0.120    0.032    0.041    0.076
    at the limit, 16383 + 1    split    0.019    0.021    0.018    0.091
    composed, head dim 16      all      0.025    0.006    0.006    0.018
    composed, head dim 20      all      0.021    0.005    0.004    0.023

(0.99 / 0.94: a tensor stored as bf16 is allowed half a bf16 spacing, 2^-8 of its value, which single elements attain.  relu_mask is
bit-exact.  torch.autograd.grad on a weight marked for the direct path raises in every mode.)
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import autograd_node_cases as A                                                  # noqa: E402
import kernel_refs as R                                                          # noqa: E402
from kernel_matrix_cases import (BAR_FP32, _attn_reference, _bf16_round, _colsum_bar, _key_bias, attn_bar_ratios,   # noqa: E402
                                 attn_eps_bwd, attn_mags)

DEV = "cuda:0"
F32 = torch.float32


@pytest.fixture
def ops():
    from emloco_amd.predictor import ops as o
    return o


def _real_lib():
    from emloco_amd import _lib as L
    return L.require_device()


def _tap_seeds(ops, mp):
    seeds, real = [], ops.next_dropout_seed

    def tapped():
        seeds.append(real())
        return seeds[-1]
    mp.setattr(ops, "next_dropout_seed", tapped)
    return seeds


def _gemm_keep(seed, rows, cols, p):
    """keep mask of a GEMM epilogue's dropout over a dense rows x cols output (the flat element index is hashed)"""
    h = np.zeros(rows * cols, np.uint8)
    assert _real_lib().emloco_dropout_keep_mask(seed & 0xFFFFFFFF, 0, rows * cols, C.c_float(p), h.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(h.reshape(rows, cols)).double()


def _ffn_keep(seed, rows, F_, p):
    h = np.zeros((rows, F_), np.uint8)
    assert _real_lib().emloco_ffn_keep_mask(seed & 0xFFFFFFFF, 0, rows, F_, C.c_float(p), h.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(h).double()


def _attn_keep(seed, n_seq, H, S, p):
    h = np.zeros(n_seq * H * S * S, np.uint8)
    assert _real_lib().emloco_attention_keep_mask(seed & 0xFFFFFFFF, n_seq * H, S, C.c_float(p), h.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(h.reshape(n_seq, H, S, S)).double()


def _offset_copy(t):
    """a device copy of t whose storage starts one float past a 16-byte boundary (contiguous, storage offset 1)"""
    buf = torch.zeros(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.storage_offset() == 1
    return v


def _d64(t):
    return None if t is None else t.detach().double().cpu()


def _split2(rec):
    return bool(rec["flags"] & A.GEMM_SPLIT2)


# ---------------------------------------------------------------------------------------------------------------------------------
# linear

def _linear_leaves(c, inp):
    M, K, N = c.M, c.K, c.N
    x = inp["x"].to(DEV)
    if c.x_kind == "transposed":
        x = x.t().contiguous().t()
        assert not x.is_contiguous()
    elif c.x_kind == "offset":
        x = _offset_copy(x)
    else:
        x = x.view(*c.lead, K)
    W = inp["W"].to(DEV)
    if c.w_kind == "t_view":
        W = W.t().contiguous().t()
        assert not W.is_contiguous()
    b = inp["b"].to(DEV) if c.bias else None
    for t, need in zip((x, W, b), c.need()):
        if need:
            t.requires_grad_(True)
    dy = inp["dy"].to(DEV)
    if c.dy_kind == "strided":
        wide = torch.zeros(M, 2 * N, device=DEV)
        wide[:, ::2] = dy
        dy = wide[:, ::2]
        assert not dy.is_contiguous()
    else:
        dy = dy.view(*c.lead, N)
    return x, W, b, dy


def _linear_case(ops, c, mode, rat, mp):
    inp = c.inputs()
    x, W, b, dy = _linear_leaves(c, inp)
    census, seeds = A.Census(ops, mp), _tap_seeds(ops, mp)
    with A.precision(ops, mode, mp):
        y = ops.linear(x, W, b, relu=bool(c.relu), drop_p=c.p, out_bf16=c.out_bf16)
        fwd_end = census.mark()
        leaves = [t for t, need in zip((x, W, b), c.need()) if need]
        if c.dy_kind == "expanded":
            grads = torch.autograd.grad(y.sum(), leaves)
        else:
            grads = torch.autograd.grad(y, leaves, dy.to(y.dtype))
    torch.cuda.synchronize()
    got = dict(zip([n for n, need in zip(("dx", "dW", "db"), c.need()) if need], grads))
    for name, leaf in (("dx", x), ("dW", W), ("db", b)):
        if name in got and got[name].shape != leaf.shape:
            rat.fail(c, f"{name} has shape {tuple(got[name].shape)}, the leaf {tuple(leaf.shape)}")
            return
    # ---- the census: the branch the case was written for
    fwd = census.gemms()[:1]
    bwd = {"dx": census.gemms(fwd_end, ta=0, tb=1), "dW": census.gemms(fwd_end, ta=1, tb=1)}
    names = census.names(fwd_end)
    ok = len(fwd) == 1 and len(census.gemms()) == 1 + sum(name in got for name in ("dx", "dW"))
    ok = ok and all(len(bwd[name]) == (name in got) for name in bwd)
    if not ok:
        rat.fail(c, ("launches", [(r["m"], r["n"], r["k"]) for r in census.gemms()]))
        return
    fwd = fwd[0]
    y16 = y.dtype == torch.bfloat16
    kf, kx, kw = c.ksplits()
    checks = [("forward shape", (fwd["m"], fwd["n"], fwd["k"]) == (c.M, c.Np, c.Kp)),
              ("forward ksplit", fwd["ksplit"] == (1 if y16 else kf)),
              ("no accumulation outside the direct path", not any(r["flags"] & A.GEMM_ACC for r in census.gemms())),
              ("mask launch", [n for n in names if n in ("emloco_act_bwd", "emloco_act_bwd_colsum", "emloco_colsum_ex")] == ([c.act_launch()] if c.act_launch() else [])),
              ("bf16 output only in the bf16 mode", y16 == (c.out_bf16 and mode == "bf16"))]
    if "dx" in got:
        checks += [("dx ksplit", bwd["dx"][0]["ksplit"] == (1 if y16 else kx)), ("dx pieces", _split2(bwd["dx"][0]) == (mode == "split2"))]
    if "dW" in got:
        checks += [("dW ksplit", bwd["dW"][0]["ksplit"] == kw), ("dW pieces", _split2(bwd["dW"][0]) == (mode == "split2"))]
    e = c.expect
    if "ksplit" in e and not y16:
        rec = {"fwd": fwd, "dx": bwd["dx"][0], "dw": bwd["dW"][0]}[e["ksplit"]]
        checks.append(("the split reduction is reached", rec["ksplit"] > 1))
    if "kpad" in e:
        checks.append(("K padding", (fwd["k"] != c.K) == e["kpad"] and fwd["k"] % 4 == (0 if e["kpad"] else fwd["k"] % 4)))
    if "npad" in e:
        checks.append(("N padding", (fwd["n"] == 36) == e["npad"] and (fwd["n"] == 33) != e["npad"]))
    if "narrow" in e:
        checks.append(("narrow output", fwd["n"] <= 32 and not fwd["image"]))
    if e.get("unaligned_x"):
        checks.append(("unaligned x", not fwd["vec"] and not fwd["image"]))
    for what, good in checks:
        if not good:
            rat.fail(c, ("census", what, mode))
    # ---- the numbers
    keep_s = None
    if c.p > 0:
        if len(seeds) != 1:
            rat.fail(c, ("dropout seeds drawn", len(seeds)))
            return
        keep_s = _gemm_keep(seeds[0], c.M, c.Np, c.p)[:, :c.N] / (1.0 - c.p)
    yd = _d64(y).reshape(c.M, c.N)
    rnd = {"fwd": fwd["bf16"], "dx": bool(bwd["dx"]) and bwd["dx"][0]["bf16"], "dw": bool(bwd["dW"]) and bwd["dW"][0]["bf16"]}
    i64 = {k: _d64(v) for k, v in inp.items()}
    if y16:
        i64["dy"] = _bf16_round(inp["dy"])                  # (the gradient of a bf16 output arrives as bf16: an exact operand)
    ref = A.linear_reference(i64, c.relu, keep_s, yd > 0, c.p, rnd, A.eps_bwd(mode), A.eps_bwd(mode), y16=y16)
    rat.add(c, "y", yd, *ref["y"])
    for name, g in got.items():
        rat.add(c, name, _d64(g).reshape(ref[name][0].shape), *ref[name])


@pytest.mark.parametrize("mode", A.MODES)
def test_linear_matrix_against_float64(ops, mode, monkeypatch):
    rat = A.Ratios(f"linear {mode}")
    for c in A.linear_cases():
        if mode in c.modes:
            with monkeypatch.context() as mp:
                _linear_case(ops, c, mode, rat, mp)
    rat.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# the direct-gradient path

def _direct_inputs(M, K, N):
    g = A.gen(M + K + N)
    return dict(x=torch.randn(M, K, generator=g), W=torch.randn(N, K, generator=g) / K ** 0.5, b=torch.randn(N, generator=g) * 0.3,
                dy=torch.randn(M, N, generator=g), V=torch.randn(N, K, generator=g) / K ** 0.5, vb=torch.randn(N, generator=g) * 0.3,
                dz=torch.randn(M, N, generator=g), x2=torch.randn(M, K, generator=g), dy2=torch.randn(M, N, generator=g))


def _plain_ref(x, W, b, dy, census_rec, mode):
    rnd = {"fwd": False, "dx": False, "dw": census_rec["bf16"]}
    return A.linear_reference(dict(x=x, W=W, b=b, dy=dy), 0, None, None, 0.0, rnd, A.eps_bwd(mode), A.eps_bwd(mode))


@pytest.mark.parametrize("M,K,N", [(40, 20, 36), (515, 20, 36)])
@pytest.mark.parametrize("mode", A.MODES)
def test_direct_gradient_path_against_float64(ops, mode, M, K, N, monkeypatch):
    """mark_direct_grad: C += dy^T x straight into W.grad -- (a) zeroed bucket, (b) two passes accumulate, (c) one weight used twice,
    (d) a slice that is not 16-byte aligned, (e) a released bucket, (f) the mark taken back, (g) a padded K, (h) autograd.grad"""
    from emloco_amd.dist import FlatGradBucket
    rat = A.Ratios(f"direct {mode}")
    inp = _direct_inputs(M, K, N)
    i64 = {k: v.double() for k, v in inp.items()}
    dev = {k: v.to(DEV) for k, v in inp.items()}
    kw = A.ksplit_for(M, N * K)
    assert (kw > 1) == (M == 515)

    def params(odd=False, K_=K):
        ps = {k: dev[k].clone().requires_grad_(True) for k in ("W", "b", "V", "vb")}
        if K_ != K:
            ps["W"] = torch.nn.functional.pad(dev["W"], (0, K_ - K)).clone().requires_grad_(True)
        order = ([torch.zeros(3, device=DEV, requires_grad=True)] if odd else []) + [ps["W"], ps["b"], ps["V"], ps["vb"]]
        return ps, order

    def dw_recs(census, since=0):
        return census.gemms(since, ta=1, tb=1)

    with A.precision(ops, mode, monkeypatch):
        # ---- (a) zeroed bucket, one backward; a second, unmarked layer beside it
        with monkeypatch.context() as mp:
            census = A.Census(ops, mp)
            ps, order = params()
            bucket = FlatGradBucket(order, align=4)
            ops.mark_direct_grad([ps["W"]])
            slot = ps["W"].grad.data_ptr()
            ((ops.linear(dev["x"], ps["W"], ps["b"]) * dev["dy"]).sum() + (ops.linear(dev["x"], ps["V"], ps["vb"]) * dev["dz"]).sum()).backward()
            torch.cuda.synchronize()
            recs = dw_recs(census)
            acc = [bool(r["flags"] & A.GEMM_ACC) for r in recs]
            if not (len(recs) == 2 and sorted(acc) == [False, True] and all(r["ksplit"] == kw for r in recs) and ps["W"].grad.data_ptr() == slot):
                rat.fail("a", ("census", acc, [r["ksplit"] for r in recs]))
            rec = recs[acc.index(True)] if True in acc else recs[0]
            ref = _plain_ref(i64["x"], i64["W"], i64["b"], i64["dy"], rec, mode)
            ref2 = _plain_ref(i64["x"], i64["V"], i64["vb"], i64["dz"], rec, mode)
            rat.add("a", "dW", _d64(ps["W"].grad), *ref["dW"])
            rat.add("a", "db", _d64(ps["b"].grad), *ref["db"])
            rat.add("a", "dW other", _d64(ps["V"].grad), *ref2["dW"])
            rat.add("a", "db other", _d64(ps["vb"].grad), *ref2["db"])
            o = bucket.offsets
            if not all((bucket.flat[o[i] + order[i].numel():o[i + 1]] == 0).all() for i in range(len(o) - 1)):
                rat.fail("a", "the bucket's padding between the slices was written")
            # ---- (b) a second pass without zeroing adds to what is there
            c0 = _d64(ps["W"].grad)
            (ops.linear(dev["x2"], ps["W"], ps["b"]) * dev["dy2"]).sum().backward()
            torch.cuda.synchronize()
            refb = _plain_ref(i64["x2"], i64["W"], i64["b"], i64["dy2"], rec, mode)
            rat.add("b", "dW", _d64(ps["W"].grad), refb["dW"][0] + c0, refb["dW"][1] + A.eps_bwd(mode) * c0.abs())
        # ---- (c) the marked weight used twice in one graph
        with monkeypatch.context() as mp:
            census = A.Census(ops, mp)
            ps, order = params()
            FlatGradBucket(order, align=4)
            ops.mark_direct_grad([ps["W"]])
            ((ops.linear(dev["x"], ps["W"], ps["b"]) * dev["dy"]).sum() + (ops.linear(dev["x2"], ps["W"], ps["b"]) * dev["dy2"]).sum()).backward()
            torch.cuda.synchronize()
            recs = dw_recs(census)
            if not (len(recs) == 2 and all(r["flags"] & A.GEMM_ACC for r in recs)):
                rat.fail("c", "census: both uses accumulate")
            r1, r2 = (_plain_ref(i64[a], i64["W"], i64["b"], i64[d], recs[0], mode) for a, d in (("x", "dy"), ("x2", "dy2")))
            total = r1["dW"][0] + r2["dW"][0]
            rat.add("c", "dW", _d64(ps["W"].grad), total, r1["dW"][1] + r2["dW"][1] + A.eps_bwd(mode) * (r1["dW"][0].abs() + r2["dW"][0].abs()))
            rat.add("c", "db", _d64(ps["b"].grad), r1["db"][0] + r2["db"][0], r1["db"][1] + r2["db"][1] + BAR_FP32 * total.new_ones(N) * (r1["db"][0].abs() + r2["db"][0].abs()))
        # ---- (d) a slice that is not 16-byte aligned, (e) a released bucket, (f) the mark taken back, (g) a padded K
        for tag in ("d", "e", "f", "g"):
            with monkeypatch.context() as mp:
                census = A.Census(ops, mp)
                K_ = 257 if tag == "g" else K
                ps, order = params(odd=tag == "d", K_=K_)
                bucket = FlatGradBucket(order, align=1 if tag == "d" else 4)
                ops.mark_direct_grad([ps["W"]])
                xg, xg64 = dev["x"], i64["x"]
                if tag == "g":
                    xg64 = torch.nn.functional.pad(i64["x"], (0, K_ - K)) + 1.0
                    xg = xg64.float().to(DEV)
                if tag == "d" and ps["W"].grad.data_ptr() % 16 == 0:
                    rat.fail(tag, "the slice is aligned: the case does not reach its branch")
                if tag == "e":
                    bucket.release()
                if tag == "f":
                    ops.mark_direct_grad([ps["W"]], on=False)
                (ops.linear(xg, ps["W"], ps["b"]) * dev["dy"]).sum().backward()
                if tag == "e":
                    bucket.gather()
                torch.cuda.synchronize()
                recs = dw_recs(census)
                if not (len(recs) == 1 and not recs[0]["flags"] & A.GEMM_ACC and (recs[0]["n"] == A.ru4(K_))):
                    rat.fail(tag, ("census: the autograd path", [(r["n"], r["flags"]) for r in recs]))
                w64 = _d64(ps["W"])
                ref = _plain_ref(xg64, w64, i64["b"], i64["dy"], recs[0], mode)
                o = bucket.offsets[1 if tag == "d" else 0]
                in_slot = bucket.flat[o:o + ps["W"].numel()].view_as(ps["W"])
                if tuple(ps["W"].grad.shape) != (N, K_):
                    rat.fail(tag, ("gradient shape", tuple(ps["W"].grad.shape)))
                rat.add(tag, "dW", _d64(in_slot), *ref["dW"])
                rat.add(tag, "db", _d64(ps["b"].grad), *ref["db"])
        # ---- (h) torch.autograd.grad on a marked weight: an error, or the right gradient -- never a wrong number
        with monkeypatch.context() as mp:
            census = A.Census(ops, mp)
            ps, order = params()
            FlatGradBucket(order, align=4)
            ops.mark_direct_grad([ps["W"]])
            y = ops.linear(dev["x"], ps["W"], ps["b"])
            try:
                (g,) = torch.autograd.grad(y, [ps["W"]], dev["dy"])
            except RuntimeError as err:
                assert "allow_unused" in str(err) or "not have been used" in str(err), err
                print(f"\n  [direct {mode}] autograd.grad on a marked weight raises: {str(err)[:90]}")
            else:
                torch.cuda.synchronize()
                ref = _plain_ref(i64["x"], i64["W"], i64["b"], i64["dy"], dw_recs(census)[0], mode)
                rat.add("h", "dW", _d64(g), *ref["dW"])
    rat.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# relu_mask

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_relu_mask_is_a_select_both_ways(ops, n, monkeypatch):
    """t where h > 0, else +0: bit-equal to the select (and equal in value to (h > 0) * t, whose zeros carry t's sign); h holds -0.0,
    +0.0 and a denormal (positive: it selects)"""
    g = A.gen(n)
    specials = torch.tensor([-0.0, 0.0, 1e-40, -1e-40])
    for shift in range(4 if n == 1 else 1):
        h = torch.randn(n, generator=g)
        k = min(n, 4)
        h[:k] = specials.roll(-shift)[:k]
        t, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
        census = A.Census(ops, monkeypatch)
        td, hd = t.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
        out = ops.relu_mask(td, hd)
        gt, gh = torch.autograd.grad(out, [td, hd], dy.to(DEV), allow_unused=True)
        assert gh is None
        assert census.names() == ["emloco_act_bwd", "emloco_act_bwd"]
        for got, src in ((out, t), (gt, dy)):
            want = torch.where(h > 0, src, torch.zeros_like(src))
            assert torch.equal(got.detach().cpu().view(torch.int32), want.view(torch.int32)), (n, shift)
            assert torch.equal(got.detach().cpu(), (h > 0).float() * src)


# ---------------------------------------------------------------------------------------------------------------------------------
# feed-forward

def _ffn_leaves(c, inp, names=("W1", "b1", "W2", "b2")):
    x = inp["x"].to(DEV)
    x = _offset_copy(x) if c.x_kind == "offset" else x
    x.requires_grad_(bool(c.need_dx))
    return x, [inp[k].to(DEV).requires_grad_(True) for k in names]


def _ffn_rnd(ops, c, mode, census, fwd_end, chained):
    if chained:
        return {k: True for k in ("h", "f", "dw2", "dz1", "dx", "dw1")}, None
    fw = census.gemms()[:2]
    dw = census.gemms(fwd_end, ta=1, tb=1)
    dx = census.gemms(fwd_end, ta=0, tb=1)
    if len(fw) != 2 or len(dw) != 2 or len(dx) != int(bool(c.need_dx)) or len(census.named("emloco_gemm_relu_bwd")) != 1:
        return None, None
    dw2 = [r for r in dw if (r["m"], r["n"]) == (c.N, c.F)][0]
    dw1 = [r for r in dw if r is not dw2][0]
    rnd = {"h": fw[0]["bf16"], "f": fw[1]["bf16"], "dw2": dw2["bf16"], "dz1": mode == "bf16", "dx": bool(dx) and dx[0]["bf16"], "dw1": dw1["bf16"]}
    return rnd, dict(fw=fw, dw1=dw1, dw2=dw2, dx=dx)


_CHAINED_F = {}


def _ffn_case(ops, c, mode, rat, mp):
    inp = c.inputs()
    x, (W1, b1, W2, b2) = _ffn_leaves(c, inp)
    census, seeds = A.Census(ops, mp), _tap_seeds(ops, mp)
    with A.precision(ops, mode, mp):
        f = ops.feed_forward(x, W1, b1, W2, b2, drop_p=c.p)
        fwd_end = census.mark()
        h = f.grad_fn.saved_tensors[3]
        leaves = ([x] if c.need_dx else []) + [W1, b1, W2, b2]
        grads = torch.autograd.grad(f, leaves, inp["df"].to(DEV))
    torch.cuda.synchronize()
    got = dict(zip((["dx"] if c.need_dx else []) + ["dW1", "db1", "dW2", "db2"], grads))
    chained = "emloco_ffn_fwd" in census.names()
    if chained != c.chained(mode) or ("chain" in c.expect and mode == "bf16" and chained != c.expect["chain"]):
        rat.fail(c, ("census: chained launch", chained))
        return
    rnd, recs = _ffn_rnd(ops, c, mode, census, fwd_end, chained)
    if rnd is None:
        rat.fail(c, ("census: launches", census.names()))
        return
    if chained:
        if any(r["name"] == "gemm" for r in census.calls[:fwd_end]):
            rat.fail(c, "census: a GEMM in the chained forward")
        if census.names(fwd_end).count("emloco_ffn_bwd_input_colsum") != 1:
            rat.fail(c, "census: the chained input-gradient launch")
    else:
        two = mode == "split2"
        if not (_split2(recs["dw1"]) == two and _split2(recs["dw2"]) == two and all(_split2(r) == two for r in recs["dx"])):
            rat.fail(c, "census: pieces of the gradient products")
        if recs["dw1"]["ksplit"] != A.ksplit_for(c.M, c.F * c.K) or recs["dw2"]["ksplit"] != A.ksplit_for(c.M, c.N * c.F):
            rat.fail(c, "census: split of the weight-gradient reductions")
        if c.expect.get("dw_ksplit") and not (recs["dw1"]["ksplit"] > 1 and recs["dw2"]["ksplit"] > 1):
            rat.fail(c, "census: the split weight-gradient reduction is not reached")
    h16 = h.dtype == torch.bfloat16
    if h16 != c.h16(mode):
        rat.fail(c, ("hidden layer dtype", h.dtype))
    k1s = k2s = None
    if c.p > 0:
        s1, s2 = seeds
        k1 = _ffn_keep(s1, c.M, c.F, c.p) if chained else _gemm_keep(s1, c.M, c.F, c.p)
        k1s, k2s = k1 / (1.0 - c.p), _gemm_keep(s2, c.M, c.N, c.p) / (1.0 - c.p)
    i64 = {k: _d64(v) for k, v in inp.items()}
    ref = A.ffn_reference(i64, k1s, k2s, _d64(h), c.p, rnd, h16, A.eps_bwd(mode), A.eps_bwd(mode))
    rat.add(c, "h", _d64(h), *ref["h"])
    rat.add(c, "f", _d64(f), *ref["f"])
    for name, g in got.items():
        rat.add(c, name, _d64(g), *ref[name])
    # the unaligned-x fall-back agrees with the chained launch on the same values (each within its own bar of its reference)
    key = (c.M, c.F, c.p)
    if c.name == "chain" and chained:
        _CHAINED_F[key] = (_d64(f), {k: _d64(v) for k, v in got.items()}, _d64(h))
    elif c.name == "chain" and key in _CHAINED_F and c.p == 0.0:            # (with dropout the two routes hash their hidden masks differently)
        f0, g0, h0 = _CHAINED_F[key]
        # (the fall-back's first product reads an unaligned x, which the launcher serves with the fp32 kernel on UNROUNDED operands:
        # the two routes differ by the reduced-precision mode's stated error, 2e-2 of a tensor's scale.  Each route's backward masks
        # by ITS OWN hidden layer, as every reference here does: a unit whose pre-activation is within the operands' bf16 rounding of
        # zero -- 2 x 2^-9 of sum |x| |w| + |b| -- may be active in one route and not in the other, and then its whole gradient
        # |dz2 W2| is the difference; a unit that flips further from zero than that is an error)
        z = i64["x"] @ i64["W1"].t() + i64["b1"]
        mz = i64["x"].abs() @ i64["W1"].abs().t() + i64["b1"].abs()
        flip = (_d64(h) > 0) != (h0 > 0)
        if (flip & (z.abs() > A.BF16_STORE * mz)).any():
            rat.fail(c, "a hidden unit far from zero is active in one route only")
        g1 = (i64["df"].abs() @ i64["W2"].abs()) * flip.double()
        flipped = {"dx": g1 @ i64["W1"].abs(), "dW1": g1.t() @ i64["x"].abs(), "db1": g1.sum(0)}
        for k, a, b in [("f", _d64(f), f0)] + [(k, _d64(got[k]), g0[k]) for k in g0]:
            rat.add(c, "vs chained " + k, a, b, torch.full_like(b, 2e-2 * b.abs().max().item() + 1e-6) + flipped.get(k, 0.0))


@pytest.mark.parametrize("mode", A.MODES)
def test_feed_forward_matrix_against_float64(ops, mode, monkeypatch):
    rat = A.Ratios(f"ffn {mode}")
    _CHAINED_F.clear()
    for c in A.ffn_cases():
        if mode in c.modes:
            with monkeypatch.context() as mp:
                _ffn_case(ops, c, mode, rat, mp)
    rat.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# layer norm

def _ln_judge(tab, fails, case, c, y, saved, dy_a, dy_b, gx, gres, gg, gb, twice=False):
    """y and the gradients of one layer-norm node against float64, the backward on the node's own saved xr / mean / rstd"""
    xr, gamma, mean, rstd = (t.detach().cpu() for t in saved)
    res = c["x"] if twice else c.get("res")
    want_xr = c["x"] + res if res is not None else c["x"]
    if not torch.equal(xr.reshape(want_xr.shape), want_xr):
        fails.append((case, "xr is not the fp32 sum x + res"))
    ref = R.layernorm_fwd(c["x"], res, c["gamma"], c["beta"], 1e-5)
    r32 = R.layernorm_fwd(c["x"], res, c["gamma"], c["beta"], 1e-5, dtype=F32)
    tab.add(case, "y", R.err_max(y.detach().cpu().reshape(ref[0].shape), ref[0]), R.err_max(r32[0], ref[0]))
    bref = R.layernorm_bwd(xr, c["gamma"], mean, rstd, dy_a, dy_b)
    b32 = R.layernorm_bwd(xr, c["gamma"], mean, rstd, dy_a, dy_b, dtype=F32)
    scale = 2.0 if twice else 1.0
    tab.add(case, "dxr", R.err_max(gx.detach().cpu().reshape(bref[0].shape), scale * bref[0]), R.err_max(b32[0], bref[0]))
    if gres is not None and not torch.equal(gres, gx):
        fails.append((case, "res and x do not get the same dxr"))
    dy = (dy_a + dy_b if dy_b is not None else dy_a).double()
    xh = (xr.double() - mean.double()[:, None]) * rstd.double()[:, None]
    for what, got, want, terms in (("dgamma", gg, bref[1], dy * xh), ("dbeta", gb, bref[2], dy)):
        r = A.worst(got, want, _colsum_bar(terms))
        if not r <= 1.0:
            fails.append((case, what, r))


def test_layer_norm_matrix_against_float64(ops, monkeypatch):
    tab, fails = R.Table("layer_norm node"), []
    for d in A.LN_D:
        for rows in A.LN_ROWS:
            c = A.ln_inputs(rows, d)
            for res_kind, fork, through in (("none", False, "a"), ("given", False, "a"), ("same", False, "a"), ("given", True, "a"), ("given", True, "b"),
                                            ("given", True, "ab"), ("none", True, "ab")):
                case = (rows, d, res_kind, fork, through)
                with monkeypatch.context() as mp:
                    census = A.Census(ops, mp)
                    x = c["x"].to(DEV).requires_grad_(True)
                    res = {"none": None, "given": c["res"].to(DEV).requires_grad_(True), "same": x}[res_kind]
                    gamma, beta = c["gamma"].to(DEV).requires_grad_(True), c["beta"].to(DEV).requires_grad_(True)
                    out = ops.layer_norm(x, res, gamma, beta, 1e-5, fork=fork)
                    ya, yb = out if fork else (out, None)
                    saved = ya.grad_fn.saved_tensors
                    if fork and (yb.grad_fn is not ya.grad_fn or not torch.equal(ya, yb)):
                        fails.append((case, "the fork's two outputs are not one node's"))
                    dy_a, dy_b = (c["dy"] if "a" in through else None), (c["dy2"] if "b" in through else None)
                    outs = [t for t, g in ((ya, dy_a), (yb, dy_b)) if g is not None]
                    gos = [g.to(DEV) for g in (dy_a, dy_b) if g is not None]
                    leaves = [x] + ([res] if res_kind == "given" else []) + [gamma, beta]
                    grads = list(torch.autograd.grad(outs, leaves, gos))
                    torch.cuda.synchronize()
                    gx = grads.pop(0)
                    gres = grads.pop(0) if res_kind == "given" else None
                    if census.names() != ["emloco_layernorm_fwd_save", "emloco_layernorm_bwd2"]:
                        fails.append((case, "census", census.names()))
                    first, second = (dy_a, dy_b) if dy_a is not None else (dy_b, None)
                    inputs = dict(c) if res_kind != "none" else {k: v for k, v in c.items() if k != "res"}
                    _ln_judge(tab, fails, case, inputs, ya, saved, first, second, gx, gres, grads[0], grads[1], twice=res_kind == "same")
    assert not fails, (len(fails), fails[:10])
    tab.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# feed_forward_norm (reduced-precision mode: the chained launch serves nothing else)

def _ffn_norm_run(ops, c, inp, p, fork, through, mp, counter, mutate=None):
    """one run of feed_forward_norm on fresh leaves; -> dict of y, gradients, the node's saved tensors, census, seeds"""
    census, seeds = A.Census(ops, mp), _tap_seeds(ops, mp)
    ops._drop_counter[0] = counter
    t = {k: inp[k].to(DEV) for k in ("x", "res", "W1", "b1", "W2", "b2", "gamma", "beta")}
    if mutate:
        mutate(t)
    for v in t.values():
        v.requires_grad_(True)
    out = ops.feed_forward_norm(t["x"], t["res"], t["W1"], t["b1"], t["W2"], t["b2"], t["gamma"], t["beta"], 1e-5, drop_p=p, fork=fork)
    ya, yb = out if fork else (out, None)
    saved = ya.grad_fn.saved_tensors                        # (read ahead of the backward, which frees them)
    dy_a, dy_b = (inp["df"] if "a" in through else None), (inp["df2"] if "b" in through else None)
    outs = [o for o, g in ((ya, dy_a), (yb, dy_b)) if g is not None]
    gos = [g.to(DEV) for g in (dy_a, dy_b) if g is not None]
    names = ("x", "res", "W1", "b1", "W2", "b2", "gamma", "beta")
    grads = torch.autograd.grad(outs, [t[k] for k in names], gos)
    torch.cuda.synchronize()
    return dict(y=ya, yb=yb, grads=dict(zip(names, grads)), saved=saved, census=census, seeds=seeds, dy=(dy_a, dy_b))


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_feed_forward_norm_chained_launch_and_every_fall_back(ops, M, p, monkeypatch):
    """the chained launch against float64 stage by stage (the feed-forward on the rounded operands and the hidden layer as stored, the
    layer norm on the saved sum, the feed-forward's backward on the dxr that reaches res), fork false and true with a gradient through
    either output and both; then every fall-back of the wrapper, shown by the census to have taken the two-op route, against the
    chained launch's results with the same seeds (the reduced-precision mode's stated error: 2e-2 of a tensor's scale)"""
    c = A.FfnCase("norm", M, 128, 64, 128, p)
    inp = c.inputs()
    i64 = {k: _d64(v) for k, v in inp.items()}
    rat, tab, fails = A.Ratios(f"ffn_norm M={M} p={p}"), R.Table("ffn_norm node"), []
    all_rnd = {k: True for k in ("h", "f", "dw2", "dz1", "dx", "dw1")}
    with A.precision(ops, "bf16", monkeypatch):
        base = None
        for fork, through in ((False, "a"), (True, "a"), (True, "b"), (True, "ab")):
            with monkeypatch.context() as mp:
                r = _ffn_norm_run(ops, c, inp, p, fork, through, mp, 1000)
            names = r["census"].names()
            if names.count("emloco_ffn_fwd_norm") != 1 or "emloco_ffn_fwd" in names or "emloco_layernorm_fwd_save" in names:
                fails.append((fork, through, "census: the chained launch", names))
                continue
            x2, W1b, W2b, h, mbits, xr, gamma, mean, rstd = r["saved"]
            k1s = k2s = None
            if p > 0:
                k1s, k2s = _ffn_keep(r["seeds"][0], M, 64, p) / (1.0 - p), _gemm_keep(r["seeds"][1], M, 128, p) / (1.0 - p)
            g = r["grads"]
            first, second = r["dy"] if r["dy"][0] is not None else (r["dy"][1], None)
            # the layer norm on the saved sum (a pseudo-case whose x is xr itself)
            ln_c = dict(x=xr.detach().cpu(), gamma=inp["gamma"], beta=inp["beta"])
            _ln_judge(tab, fails, (M, p, fork, through), ln_c, r["y"], (xr, gamma, mean, rstd), first, second, g["res"], None, g["gamma"], g["beta"])
            # the feed-forward: its output is xr - res (one more fp32 rounding, of the sum), its incoming gradient the dxr that reached res
            j64 = dict(i64, df=_d64(g["res"]))
            ref = A.ffn_reference(j64, k1s, k2s, _d64(h), p, all_rnd, True, BAR_FP32, BAR_FP32)
            rat.add((fork, through), "h", _d64(h), *ref["h"])
            rat.add((fork, through), "f", _d64(xr) - i64["res"], ref["f"][0], ref["f"][1] + 2.0 ** -23 * _d64(xr).abs())
            for name, key in (("dx", "x"), ("dW1", "W1"), ("db1", "b1"), ("dW2", "W2"), ("db2", "b2")):
                rat.add((fork, through), name, _d64(g[key]), *ref[name])
            if (fork, through) == (False, "a"):
                base = r
        # ---- the fall-backs: each takes the two-op route and agrees with the chained launch
        def off(key):
            def mutate(t):
                t[key] = _offset_copy(t[key])
            return mutate
        if base is not None:
            for tag, mutate in (("res offset by a float", off("res")), ("gamma an offset view", off("gamma")), ("x offset by a float", off("x"))):
                with monkeypatch.context() as mp:
                    r = _ffn_norm_run(ops, c, inp, p, False, "a", mp, 1000, mutate)
                names = r["census"].names()
                if "emloco_ffn_fwd_norm" in names or names.count("emloco_layernorm_fwd_save") != 1:
                    fails.append((tag, "census: the two-op route", names))
                if r["seeds"] != base["seeds"]:
                    fails.append((tag, "seeds differ from the chained run's"))
                compared = list(base["grads"])
                if tag.startswith("x offset"):
                    # (an unaligned x takes the feed-forward itself off the chained launch: its hidden dropout mask is then the GEMM
                    # epilogue's hash, another mask, and its ReLU mask its own hidden layer's -- the feed-forward matrix judges that
                    # route's x / W1 / b1 gradients against float64 with the route's own masks; here what does not pass the hidden mask)
                    if p > 0:
                        continue
                    compared = ["res", "W2", "b2", "gamma", "beta"]
                for what, a, b in [("y", r["y"], base["y"])] + [(k, r["grads"][k], base["grads"][k]) for k in compared]:
                    err, sc = (a - b).abs().max().item(), b.abs().max().item()
                    if not err <= 2e-2 * sc + 1e-6:
                        fails.append((tag, what, err, sc))
        # ---- res of another shape: refused, as layer_norm refuses it, before anything is launched
        with monkeypatch.context() as mp:
            census = A.Census(ops, mp)
            t = {k: inp[k].to(DEV) for k in ("x", "res", "W1", "b1", "W2", "b2", "gamma", "beta")}
            with pytest.raises(ValueError):
                ops.layer_norm(t["x"], t["res"][:1] if M > 1 else t["res"].repeat(2, 1), t["gamma"], t["beta"])
            with pytest.raises(ValueError):
                ops.feed_forward_norm(t["x"], t["res"][:1] if M > 1 else t["res"].repeat(2, 1), t["W1"], t["b1"], t["W2"], t["b2"], t["gamma"], t["beta"])
            if "emloco_ffn_fwd_norm" in census.names() or "emloco_layernorm_fwd_save" in census.names():
                fails.append(("res of another shape", "a launch was made", census.names()))
            # ---- grad disabled with fork: one tensor, returned twice, from the chained launch
            with torch.no_grad():
                ya, yb = ops.feed_forward_norm(t["x"], t["res"], t["W1"], t["b1"], t["W2"], t["b2"], t["gamma"], t["beta"], fork=True)
            if ya is not yb or census.names().count("emloco_ffn_fwd_norm") != 1:
                fails.append(("grad disabled with fork", "not one tensor from one chained launch", census.names()))
            if p == 0.0 and base is not None and not torch.equal(ya, base["y"].detach()):
                fails.append(("grad disabled with fork", "differs from the run with a graph"))
    assert not fails, (len(fails), fails[:10])
    rat.check()
    tab.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# attention

ATTN_MODES = ("fp32", "split", "bf16")


def _attn_judge(ops, rat, case, mode, qkv, kb, H, nq, keep, p, dout, out, dqkv):
    """out and dqkv of a fused launch (or several) against float64: per-element bars in the fp32 classes, the bf16 class of
    check_attention (2e-2 / 3e-2 of a tensor's scale, against float64 on the rounded q|k|v) in the reduced-precision mode"""
    d = 32 * H
    q64 = _bf16_round(qkv) if mode == "bf16" else qkv.double()
    ref = _attn_reference(q64, kb, H, nq, keep, p, dout.double())
    g_out, g_dqkv = _d64(out), _d64(dqkv)
    if mode == "bf16":
        for what, got, want, rel, sc in (("out", g_out, ref[0], 2e-2, None), ("dq", g_dqkv[..., :d], ref[2][..., :d], 3e-2, ref[2].abs().max()),
                                         ("dk", g_dqkv[..., d:2 * d], ref[2][..., d:2 * d], 3e-2, ref[2].abs().max()),
                                         ("dv", g_dqkv[..., 2 * d:], ref[2][..., 2 * d:], 3e-2, ref[2].abs().max())):
            sc = want.abs().max() if sc is None else sc
            rat.add(case, what, got, want, torch.full_like(want, float(rel * sc + 1e-6)))
        if not (g_dqkv[:, nq:, :d] == 0).all():
            rat.fail(case, "dQ of rows that did not attend")
        return
    eps = attn_eps_bwd(_real_lib(), "split") if mode == "split" else BAR_FP32
    mags = attn_mags(q64, kb, H, nq, keep, p, dout.double())
    el = attn_bar_ratios((g_out, ref[3], g_dqkv), (ref[0], ref[3], ref[2]), mags, d, eps)
    for k, v in el.items():
        if k != "dsum":
            rat.rows[k] = max(rat.rows.get(k, 0.0), v)
            if not v <= 1.0:
                rat.fail(case, (k, v))


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_fused_attention_node_against_float64(ops, mode, monkeypatch):
    Bn, S, H = 3, 33, 4
    rat = A.Ratios(f"attention {mode}")
    with A.precision(ops, {"split": "split3"}.get(mode, mode), monkeypatch):
        for kind in A.ATTN_BIAS:
            for nq in A.ATTN_NQ:
                for p in (0.0, 0.1):
                    case = (kind, nq, p)
                    g = A.gen(S + (nq or 0) + len(kind))
                    qkv = torch.randn(Bn, S, 96 * H, generator=g) * 0.6
                    nq_eff = S if (nq is None or nq >= S) else nq
                    dout = torch.randn(Bn, nq_eff, 32 * H, generator=g)
                    kb = _key_bias(kind, Bn, S, 17, "cpu")
                    with monkeypatch.context() as mp:
                        census, seeds = A.Census(ops, mp), _tap_seeds(ops, mp)
                        leaf = qkv.to(DEV).requires_grad_(True)
                        out = ops.attention(leaf, kb.to(DEV) if kb is not None else None, H, drop_p=p, n_query=nq)
                        (dqkv,) = torch.autograd.grad(out, [leaf], dout.to(DEV))
                        torch.cuda.synchronize()
                    fw, bw = census.named("emloco_attention_fwd_queries"), census.named("emloco_attention_bwd_queries")
                    if not (len(fw) == 1 and len(bw) == 1 and fw[0]["args"][2] == nq_eff and bw[0]["args"][2] == nq_eff and len(seeds) == int(p > 0)):
                        rat.fail(case, ("census", census.names()))
                        continue
                    keep = _attn_keep(seeds[0], Bn, H, S, p)[:, :, :nq_eff] if p > 0 else None
                    _attn_judge(ops, rat, case, mode, qkv, kb, H, nq_eff, keep, p, dout, out, dqkv)
                    if kind == "full" and not (out[-1] == 0).all():
                        rat.fail(case, "a fully masked sequence gives zeros")
    rat.check()


@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fused_attention_chunks_replay_their_seeds(ops, mode, p, monkeypatch):
    """MAX_SEQ_HEADS = 9 with four heads: five sequences go out as 2 + 2 + 1, each chunk's mask drawn with seed + b0 and indexed from
    zero inside the chunk, forward and backward alike"""
    Bn, S, H, seed = 5, 33, 4, 0x7FFFFFF0
    monkeypatch.setattr(ops.FusedAttentionFn, "MAX_SEQ_HEADS", 9)
    parts = A.chunks(Bn, H, 9)
    assert parts == [(0, 2), (2, 2), (4, 1)]
    g = A.gen(5)
    qkv, dout = torch.randn(Bn, S, 96 * H, generator=g) * 0.6, torch.randn(Bn, S, 32 * H, generator=g)
    kb = _key_bias("cut", Bn, S, 17, "cpu")
    rat = A.Ratios(f"attention chunks {mode} p={p}")
    with A.precision(ops, {"split": "split3"}.get(mode, mode), monkeypatch):
        census = A.Census(ops, monkeypatch)
        leaf = qkv.to(DEV).requires_grad_(True)
        out = ops.FusedAttentionFn.apply(leaf, kb.to(DEV), H, p, seed, None)
        (dqkv,) = torch.autograd.grad(out, [leaf], dout.to(DEV))
        torch.cuda.synchronize()
    fw, bw = census.named("emloco_attention_fwd_queries"), census.named("emloco_attention_bwd_queries")
    assert [r["args"][0] for r in fw] == [n for _, n in parts] and [r["args"][0] for r in bw] == [n for _, n in parts]
    want_seeds = [(seed + b0) & 0xFFFFFFFF for b0, _ in parts]
    assert [r["args"][-2] for r in fw] == want_seeds and [r["args"][-2] for r in bw] == want_seeds
    keep = torch.cat([_attn_keep(seed + b0, n, H, S, p) for b0, n in parts]) if p > 0 else None
    _attn_judge(ops, rat, "chunks", mode, qkv, kb, H, S, keep, p, dout, out, dqkv)
    rat.check()


def test_fused_attention_at_the_real_chunk_limit(ops, monkeypatch):
    """16384 sequences of four heads cross MAX_SEQ_HEADS = 65535 once (16383 + 1): the two sequences at the boundary against float64
    with each chunk's own mask; every other row finite and bit-equal to a run of its chunk's rows alone"""
    Bn, S, H, p, seed = 16384, 2, 4, 0.1, 0xFFFFF000
    assert ops.FusedAttentionFn.MAX_SEQ_HEADS == 65535
    parts = A.chunks(Bn, H, 65535)
    assert parts == [(0, 16383), (16383, 1)]
    g = A.gen(16384)
    qkv, dout = torch.randn(Bn, S, 96 * H, generator=g) * 0.6, torch.randn(Bn, S, 32 * H, generator=g)
    rat = A.Ratios("attention limit")
    mode = {"fp32_split": "split", "fp32": "fp32", "bf16": "bf16"}[ops.get_matmul_precision()]
    census = A.Census(ops, monkeypatch)
    leaf = qkv.to(DEV).requires_grad_(True)
    out = ops.FusedAttentionFn.apply(leaf, None, H, p, seed, None)
    (dqkv,) = torch.autograd.grad(out, [leaf], dout.to(DEV))
    torch.cuda.synchronize()
    assert len(census.named("emloco_attention_fwd_queries")) == 2 and len(census.named("emloco_attention_bwd_queries")) == 2
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    for b0, n in parts:
        alone = qkv[b0:b0 + n].to(DEV).requires_grad_(True)
        o = ops.FusedAttentionFn.apply(alone, None, H, p, seed + b0, None)
        (gq,) = torch.autograd.grad(o, [alone], dout[b0:b0 + n].to(DEV))
        assert torch.equal(o, out[b0:b0 + n]) and torch.equal(gq, dqkv[b0:b0 + n]), ("chunk alone", b0)
    keep = torch.cat([_attn_keep(seed, 16383, H, S, p)[16382:], _attn_keep(seed + 16383, 1, H, S, p)])
    sl = slice(16382, 16384)
    _attn_judge(ops, rat, "boundary", mode, qkv[sl], None, H, S, keep, p, dout[sl], out[sl], dqkv[sl])
    rat.check()


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("d,H", [(64, 4), (40, 2)])
def test_composed_attention_against_float64(ops, mode, d, H, monkeypatch):
    """head dims 16 and 20 take the GEMM -> softmax -> GEMM composition; every product there is at most 32 wide, which the launcher
    serves with the plain fp32 kernel in every mode (the census says so): fp32 bars throughout, through the head-dim-32 embedding"""
    Bn, S, dh = 3, 21, d // H
    g = A.gen(d + H)
    qkv, dout = torch.randn(Bn, S, 3 * d, generator=g) * 0.6, torch.randn(Bn, S, d, generator=g)
    rat = A.Ratios(f"composed attention {mode} dh={dh}")
    with A.precision(ops, mode, monkeypatch):
        census = A.Census(ops, monkeypatch)
        leaf = qkv.to(DEV).requires_grad_(True)
        out = ops.attention(leaf, None, H)
        (dqkv,) = torch.autograd.grad(out, [leaf], dout.to(DEV))
        torch.cuda.synchronize()
        assert not census.named("emloco_attention_fwd_queries") and len(census.named("emloco_softmax_fwd")) == H == len(census.named("emloco_softmax_bwd"))
        assert len(census.gemms()) == 6 * H and not any(r["bf16"] or r["n"] > 32 for r in census.gemms())
        q32, do32, c = A.embed32(qkv.double(), dout.double(), H, dh)
        ref = _attn_reference(q32, None, H, S, None, 0.0, do32)
        mags = attn_mags(q32, None, H, S, None, 0.0, do32)
        r_out, r_dqkv = A.unembed32(ref[0], ref[2], H, dh, c)
        m_out, m_dqkv = A.unembed32(mags[0], mags[2], H, dh, c)
        rat.add("p0", "out", _d64(out), r_out, BAR_FP32 * m_out)
        for i, what in enumerate(("dq", "dk", "dv")):
            sl = slice(i * d, (i + 1) * d)
            rat.add("p0", what, _d64(dqkv)[..., sl], r_dqkv[..., sl], BAR_FP32 * m_dqkv[..., sl])
        # n_query: the sliced result
        with torch.no_grad():
            assert torch.equal(ops.attention(leaf, None, H, n_query=5), out[:, :5])
            # dropout (a torch.rand mask): repeats under the seed, differs between seeds, and keeps 1 - p of the probability mass
            ones_v = qkv.clone()
            ones_v[..., 2 * d:] = 1.0
            ones_v = ones_v.to(DEV)
            torch.manual_seed(11)
            a = ops.attention(ones_v, None, H, drop_p=0.1)
            torch.manual_seed(11)
            b = ops.attention(ones_v, None, H, drop_p=0.1)
            torch.manual_seed(12)
            c2 = ops.attention(ones_v, None, H, drop_p=0.1)
        assert torch.equal(a, b) and not torch.equal(a, c2)
        assert abs(a.mean().item() - 1.0) < 0.05 and a.std().item() > 1e-3      # rows of P sum to 1: E[sum_j P_ij keep_ij / (1 - p)] = 1
    rat.check()


# ---------------------------------------------------------------------------------------------------------------------------------
# no node can be differentiated twice

def _twice(out, leaf, dy):
    (g,) = torch.autograd.grad(out, [leaf], dy, create_graph=True)
    assert g.requires_grad, "the gradient came back without a graph"
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def _r(*shape, seed=0, scale=1.0, grad=False):
    t = (torch.randn(*shape, generator=A.gen(seed + sum(shape))) * scale).to(DEV)
    return t.requires_grad_(True) if grad else t


def test_linear_node_refuses_a_second_differentiation(ops):
    x = _r(9, 20, grad=True)
    _twice(ops.linear(x, _r(36, 20, grad=True), _r(36, grad=True), relu=True), x, _r(9, 36))


def test_relu_mask_node_refuses_a_second_differentiation(ops):
    t = _r(65, grad=True)
    _twice(ops.relu_mask(t, _r(65, seed=1)), t, _r(65, seed=2))


def test_feed_forward_node_refuses_a_second_differentiation(ops):
    x = _r(9, 20, grad=True)
    _twice(ops.feed_forward(x, _r(36, 20, grad=True), _r(36, grad=True), _r(20, 36, grad=True), _r(20, grad=True)), x, _r(9, 20, seed=3))


def test_feed_forward_norm_node_refuses_a_second_differentiation(ops, monkeypatch):
    with A.precision(ops, "bf16", monkeypatch):
        x = _r(9, 128, grad=True)
        y = ops.feed_forward_norm(x, _r(9, 128, seed=1, grad=True), _r(64, 128, scale=0.1, grad=True), _r(64, grad=True), _r(128, 64, scale=0.1, grad=True),
                                  _r(128, grad=True), _r(128, seed=2, grad=True), _r(128, seed=3, grad=True))
        assert type(y.grad_fn).__name__.startswith("FeedForwardNormFn")
        _twice(y, x, _r(9, 128, seed=4))


def test_layer_norm_node_refuses_a_second_differentiation(ops):
    x = _r(9, 20, grad=True)
    _twice(ops.layer_norm(x, None, _r(20, grad=True), _r(20, seed=1, grad=True)), x, _r(9, 20, seed=2))


@pytest.mark.parametrize("d,H,node", [(128, 4, "FusedAttentionFn"), (64, 4, "AttentionFn")])
def test_attention_nodes_refuse_a_second_differentiation(ops, d, H, node):
    qkv = _r(2, 7, 3 * d, grad=True)
    out = ops.attention(qkv, None, H)
    assert type(out.grad_fn).__name__.startswith(node)
    _twice(out, qkv, _r(2, 7, d))


@pytest.mark.parametrize("variant", [None, 3, 0])
def test_locoval_nodes_refuse_a_second_differentiation(ops, variant):
    c = R.case_locoval(5, 2, 3)
    traj = c["traj"].to(DEV).requires_grad_(True)
    ps = [t.to(DEV).requires_grad_(True) for t in c["params"]]
    ps[4] = c["params"][4].view(1, 24).to(DEV).requires_grad_(True)
    if variant is None:
        value = ops.LocoValFn.apply(traj, c["pose"].to(DEV), c["vel"].to(DEV), *ps)[0]
    else:
        n_in, h1, h2, _ = ops.locoval_dims(variant)
        g = A.gen(variant)
        ps = [(torch.randn(*s, generator=g) * 0.2).to(DEV).requires_grad_(True) for s in ((h1, n_in), (h1,), (h2, h1), (h2,), (1, h2), (1,))]
        value = ops.LocoValVariantFn.apply(variant, traj, c["pose"].to(DEV), c["vel"].to(DEV), *ps)[0]
    _twice(value, traj, _r(5, 1))


def test_ppo_head_nodes_refuse_a_second_differentiation(ops):
    from emloco_amd.learning import ppo_heads
    B, Aa = 33, 7
    mu = _r(B, Aa, grad=True)
    outs = ppo_heads.actor_head(mu, _r(B, Aa, seed=1, scale=0.1, grad=True), _r(B, Aa, seed=2), _r(B, seed=3).abs() + 5.0, _r(B, seed=4), 0.2)
    _twice(outs[0], mu, torch.ones((), device=DEV))
    v = _r(B, 1, grad=True)
    _twice(ppo_heads.critic_head(v, _r(B, 1, seed=1), _r(B, 1, seed=2), 0.2, True), v, torch.ones((), device=DEV))
    a = _r(B, 1, grad=True)
    _twice(ppo_heads.disc_head(a, _r(B, 1, seed=1, grad=True))[0], a, torch.ones((), device=DEV))

"""Cases, float64 references and bars of the autograd-node matrix (tests/test_gpu_autograd_nodes.py, tests/test_autograd_node_refs_cpu.py).

The device matrix drives emloco_amd/predictor/ops.py -- the layer BETWEEN the kernels (pinned by tests/kernel_matrix_cases.py and
tests/test_gpu_elementwise_matrix.py) and the models: which launch runs, which mask reaches the backward, where a gradient lands, how a
launch is chunked.  Everything here is host-only (no device is touched on import, nothing reads the library): the same references and
bars judge the device's results and, in the CPU companion, a float32 stock-torch evaluation of the same case.

REFERENCES are closed-form float64 restatements (dx = dz W, dW = dz^T x, ...); the CPU companion proves them equal to stock torch in
float64 autograd.  A ReLU mask of the BACKWARD is taken from the executor's own forward output (y > 0, as check_relu_bwd does), so a
pre-activation within rounding of zero is no error; the forward is judged on its own.  Dropout masks are given (the device test reads
them from the library's host-side mask functions with the seed the node used).

BARS.  Every element: |got - ref| <= bar, bar = eps x mag + carried, mag = |a| @ |b| (+ |bias|, + |c0| for an accumulation) the
first-order magnitude of the element's own product, `carried` the error an operand that was itself computed brings along (its own bar,
propagated through |b|).  eps = BAR_FP32 for every forward product, for the fp32 mode and for three pieces; BAR_SPLIT2 for a gradient
product launched with two pieces.  Bias gradients: _colsum_bar of what was summed (+ the carried error of the summands).  An element
whose bar is zero must be exactly zero.  The reduced-precision mode is judged against float64 on the bf16-rounded operands of each
launch that really rounds them (the launcher serves bf16 operands for 16-byte-aligned operands and n > 32 only: `Census` says which
launches qualify), a tensor STORED as bf16 carries one more rounding, 2^-8 of its value (the stage-by-stage bars of the chained
feed-forward in tests/test_gpu_elementwise_matrix.py); 2^-22 of the value for a mask-and-scale pass (test_act_bwd_colsum_against_float64).
"""
import contextlib
import itertools

import torch

from kernel_matrix_cases import BAR_FP32, BAR_SPLIT2, _bf16_round, _colsum_bar

MODES = ("fp32", "split3", "split2", "bf16")
BF16_STORE = 2.0 ** -8                  # one round-to-nearest bf16 store: half a spacing
MASK_PASS = 2.0 ** -22                  # dz = dy o mask x (1 / (1 - p)) in fp32: the scale's rounding and the product's
WATCHED = ("emloco_act_bwd", "emloco_act_bwd_colsum", "emloco_colsum_ex", "emloco_ffn_fwd", "emloco_ffn_fwd_norm", "emloco_ffn_bwd_input_colsum",
           "emloco_gemm_relu_bwd", "emloco_attention_fwd_queries", "emloco_attention_bwd_queries", "emloco_layernorm_fwd_save",
           "emloco_layernorm_bwd2", "emloco_softmax_fwd", "emloco_softmax_bwd")
GEMM_ACC, GEMM_SPLIT2 = 4, 4096


def eps_bwd(mode):
    return BAR_SPLIT2 if mode == "split2" else BAR_FP32


def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def worst(got, ref, bar):
    """max |got - ref| / bar; an element whose bar is 0 counts 0 when exact and inf when not; a non-finite result counts inf"""
    got, ref, bar = got.detach().double().cpu(), ref.double().cpu(), bar.double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item() if ratio.numel() else 0.0


class Ratios:
    """worst error / bar per (family, output); `add` keeps the failures, `check` prints the table and asserts"""

    def __init__(self, family):
        self.family, self.rows, self.bad = family, {}, []

    def add(self, case, name, got, ref, bar):
        r = worst(got, ref, bar)
        self.rows[name] = max(self.rows.get(name, 0.0), r)
        if not r <= 1.0:
            self.bad.append((case, name, r))
        return r

    def fail(self, case, what):
        self.bad.append((case, what))

    def check(self):
        print()
        for name in sorted(self.rows):
            print(f"  [{self.family}] {name:<10} worst error / bar {self.rows[name]:.3f}")
        assert not self.bad, (len(self.bad), self.bad[:12])


# ---------------------------------------------------------------------------------------------------------------------------------
# precision modes and the launch census

@contextlib.contextmanager
def precision(ops, mode, monkeypatch):
    """the matmul mode and the pieces of the backward products of a case: `linear` through backward_pieces_for, the feed-forward
    through _BWD_PIECES; everything restored behind the block"""
    before = ops.get_matmul_precision()
    pieces = 2 if mode == "split2" else 3
    with monkeypatch.context() as mp:
        mp.setitem(ops._BWD_PIECES, "dx", pieces)
        mp.setitem(ops._BWD_PIECES, "dw", pieces)
        ops.set_matmul_precision({"split3": "fp32_split", "split2": "fp32_split"}.get(mode, mode))
        try:
            with ops.backward_pieces_for(pieces):
                yield
        finally:
            ops.set_matmul_precision(before)


class Census:
    """records the launches a node makes: every `ops.gemm` (shape, flags as the node passed them, ksplit, piece image, whether the
    launcher will serve bf16 operands) and the watched direct library calls (name and raw arguments)"""

    def __init__(self, ops, monkeypatch):
        self.calls, self.ops = [], ops
        real_gemm, real_lib = ops.gemm, ops._lib
        census = self

        def gemm(batch, m, n, k, A, lda, sa, ta, B, ldb, sb, tb, Cm, ldc, sc, alpha=1.0, bias=None, flags=0, ksplit=1, a_off=0, b_off=0, c_off=0,
                 drop_p=0.0, drop_seed=0, b_image=None):
            vec = all((t.data_ptr() + t.element_size() * off) % 16 == 0 and ld % 4 == 0 and st % 4 == 0 for t, off, ld, st in ((A, a_off, lda, sa), (B, b_off, ldb, sb)))
            any16 = any(t.dtype == torch.bfloat16 for t in (A, B, Cm))
            census.calls.append(dict(name="gemm", m=m, n=n, k=k, ta=ta, tb=tb, flags=flags, ksplit=ksplit, image=b_image is not None, vec=vec,
                                     bf16=(ops.get_matmul_precision() == "bf16" or any16) and vec and n > 32, drop_p=drop_p, drop_seed=drop_seed,
                                     c=Cm, c16=Cm.dtype == torch.bfloat16))
            return real_gemm(batch, m, n, k, A, lda, sa, ta, B, ldb, sb, tb, Cm, ldc, sc, alpha=alpha, bias=bias, flags=flags, ksplit=ksplit, a_off=a_off,
                             b_off=b_off, c_off=c_off, drop_p=drop_p, drop_seed=drop_seed, b_image=b_image)

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real_lib(), name)
                if name not in WATCHED:
                    return fn

                def call(*args):
                    census.calls.append(dict(name=name, args=[getattr(a, "value", a) for a in args]))
                    return fn(*args)
                return call
        proxy = Proxy()
        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(ops, "_lib", lambda: proxy)

    def mark(self):
        return len(self.calls)

    def gemms(self, since=0, **match):
        return [c for c in self.calls[since:] if c["name"] == "gemm" and all(c[k] == v for k, v in match.items())]

    def named(self, name, since=0):
        return [c for c in self.calls[since:] if c["name"] == name]

    def names(self, since=0):
        return [c["name"] for c in self.calls[since:]]


# ---------------------------------------------------------------------------------------------------------------------------------
# the pure predicates of ops.py, restated for the case table (the CPU companion holds them against ops' own)

def ksplit_for(red, out_elems):
    tiles = max(1, (out_elems + 128 * 128 - 1) // (128 * 128))
    return int(max(1, min(max(1, 512 // tiles), red // 256, 512)))


def pads_k(K):
    return K % 4 != 0 and K >= 256


def pads_n(N, rows):
    return N % 4 != 0 and N >= 32 and rows >= 1024


def ru4(v):
    return (v + 3) // 4 * 4


def chunks(Bn, nhead, max_seq_heads):
    step = max_seq_heads // nhead
    return [(b0, min(step, Bn - b0)) for b0 in range(0, Bn, step)]


def ffn_chain_ok(mode, K, F, N):
    return mode == "bf16" and K == 128 and N == 128 and 64 <= F <= 2048 and F % 64 == 0


def ffn_h16(mode, K, F, N):
    return mode == "bf16" and N > 32 and F > 32 and K > 32 and F % 4 == 0 and K % 4 == 0 and N % 4 == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# linear

class LinearCase:
    """y = dropout(relu?(x W^T + b)), x (lead..., K).  needs: which of (x, W, b) require a gradient.  x_kind: plain | transposed (a
    .t() view of a (K, M) tensor) | offset (a slice starting one float into its storage); w_kind: plain | t_view (a .t() view of a
    (K, N) tensor); dy_kind: plain | expanded (y.sum().backward()) | strided (every other column of a wider tensor).
    expect: the branch the case was written for (what the census must show)."""

    def __init__(self, name, M, K, N, lead=None, relu=0, p=0.0, bias=1, needs=(1, 1, 1), x_kind="plain", w_kind="plain", dy_kind="plain",
                 out_bf16=False, x_scale=1.0, modes=MODES, expect=None):
        self.name, self.M, self.K, self.N, self.lead = name, M, K, N, tuple(lead) if lead else (M,)
        self.relu, self.p, self.bias, self.needs = relu, p, bias, tuple(needs)
        self.x_kind, self.w_kind, self.dy_kind, self.out_bf16, self.x_scale, self.modes = x_kind, w_kind, dy_kind, out_bf16, x_scale, modes
        self.expect = dict(expect or {})

    def __repr__(self):
        return (f"linear[{self.name} {self.M}x{self.K}x{self.N} relu={self.relu} p={self.p} bias={self.bias} needs={self.needs} "
                f"x={self.x_kind} W={self.w_kind} dy={self.dy_kind}]")

    # what follows from the predicates (the CPU companion evaluates these against the table)
    @property
    def Kp(self):
        return ru4(self.K) if pads_k(self.K) else self.K

    @property
    def Np(self):
        return ru4(self.N) if pads_n(self.N, self.M) else self.N

    def padded(self):
        return self.Kp != self.K or self.Np != self.N

    def need(self):
        """(x, W, b) as LinearFn.backward sees them: the padded operands of a padded call are non-leaves that need what their source needs"""
        return self.needs[0], self.needs[1], self.needs[2] and self.bias

    def act_launch(self):
        """the mask / bias-gradient launch of the backward"""
        _, _, nb = self.need()
        if self.relu or self.p > 0:
            return "emloco_act_bwd_colsum" if nb else "emloco_act_bwd"
        return "emloco_colsum_ex" if nb else None

    def ksplits(self):
        """(forward, dx, dW) reduction splits of the three launches (bf16 outputs are never split)"""
        M, K, N = self.M, self.Kp, self.Np
        return ksplit_for(K, M * N), ksplit_for(N, M * K), ksplit_for(M, N * K)

    def inputs(self):
        g = gen(7 * self.M + 13 * self.K + 17 * self.N + 3 * self.relu + int(self.p * 100) + len(self.name))
        x = torch.randn(self.M, self.K, generator=g) * self.x_scale
        W = torch.randn(self.N, self.K, generator=g) / self.K ** 0.5
        b = torch.randn(self.N, generator=g) * 0.3 if self.bias else None
        dy = torch.ones(self.M, self.N) if self.dy_kind == "expanded" else torch.randn(self.M, self.N, generator=g)
        return dict(x=x, W=W, b=b, dy=dy)


def _subsets(bias):
    return [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)] if bias else [(1, 0, 0), (0, 1, 0), (1, 1, 0)]


def linear_cases():
    out = []
    for relu, p, bias in itertools.product((0, 1), (0.0, 0.1), (1, 0)):
        for needs in _subsets(bias):
            c = LinearCase("base", 33, 20, 36, lead=(3, 11), relu=relu, p=p, bias=bias, needs=needs)
            c.expect = {"act": c.act_launch()}
            out.append(c)
    out.append(LinearCase("narrow", 33, 20, 8, relu=1, p=0.1, expect={"narrow": True}))
    out.append(LinearCase("narrow", 33, 20, 8, expect={"narrow": True}))
    for M, K, N, which in ((8, 512, 40, "fwd"), (8, 1024, 40, "fwd"), (8, 20, 516, "dx"), (515, 20, 36, "dw"), (1030, 20, 36, "dw")):
        out.append(LinearCase("ksplit", M, K, N, relu=1, expect={"ksplit": which}, modes=("fp32", "split3", "split2")))
        out.append(LinearCase("ksplit", M, K, N, p=0.1, expect={"ksplit": which}, modes=("bf16",)))
    for K in (255, 256, 257, 258):
        out.append(LinearCase("kpad", 9, K, 36, relu=1, x_scale=1.0e3, expect={"kpad": K in (257, 258)}))
    for rows in (1023, 1024):
        for bias in (1, 0):
            out.append(LinearCase("npad", rows, 20, 33, bias=bias, expect={"npad": rows == 1024}))
        out.append(LinearCase("npad", rows, 20, 33, relu=1, p=0.1, expect={"npad": rows == 1024}))
    out.append(LinearCase("view", 33, 20, 36, x_kind="transposed", relu=1))
    out.append(LinearCase("view", 33, 20, 36, x_kind="offset", p=0.1, expect={"unaligned_x": True}))
    out.append(LinearCase("view", 33, 20, 36, w_kind="t_view", relu=1))
    out.append(LinearCase("view", 33, 20, 36, dy_kind="expanded", relu=1))
    out.append(LinearCase("view", 33, 20, 36, dy_kind="strided", p=0.1))
    out.append(LinearCase("out16", 64, 128, 384, out_bf16=True, expect={"out16": True}))
    return out


def scale32(t64, p):
    """t x (1 / (1 - p)) as the mask pass computes it -- float32 values, the float32 scale, one float32 product -- so that a launch
    which rounds the result to bf16 rounds the same number in the reference"""
    s32 = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    return (t64.float() * s32).double()


def linear_reference(inp, relu, keep_s, act, p, rnd, eps_dx, eps_dw, y16=False):
    """float64 (ref, bar) per output of a linear layer.  inp: x (M, K), W (N, K), b (N) | None, dy (M, N), float64; keep_s: keep /
    (1 - p) (M, N) or None; act: the executor's own y > 0 (M, N) for a ReLU layer; rnd: {"fwd", "dx", "dw"} -> the launch rounds its
    operands to bf16; y16: the output is stored as bf16 (and its gradient arrives as bf16: an exact operand)."""
    x, W, b, dy = inp["x"], inp["W"], inp["b"], inp["dy"]
    r = lambda t, on: _bf16_round(t) if on else t
    xa, Wa = r(x, rnd["fwd"]), r(W, rnd["fwd"])
    z = xa @ Wa.t()
    mag = xa.abs() @ Wa.abs().t()
    if b is not None:
        z, mag = z + b, mag + b.abs()
    y = z.clamp_min(0.0) if relu else z
    if keep_s is not None:
        y, mag = y * keep_s, mag * keep_s
    out = {"y": (y, BAR_FP32 * mag + (BF16_STORE * y.abs() if y16 else 0.0))}
    masked = bool(relu) or keep_s is not None
    dz = dy
    if relu:
        dz = dy * act.double()
    elif keep_s is not None:
        dz = dy * (keep_s > 0).double()
    if keep_s is not None:
        dz = scale32(dz, p)
    e_dz = MASK_PASS * dz.abs() if masked else torch.zeros_like(dz)
    for name, a, bm, on, eps in (("dx", dz, W, rnd["dx"], eps_dx), ("dW", dz.t(), x, rnd["dw"], eps_dw)):
        a_r, b_r = r(a, on), r(bm, on)
        e_a = e_dz if name == "dx" else e_dz.t()
        out[name] = (a_r @ b_r, eps * (a_r.abs() @ b_r.abs()) + e_a @ b_r.abs())
    out["db"] = (dz.sum(0), _colsum_bar(dz) + e_dz.sum(0))
    return out


def linear_float32(inp, relu, keep_s, p, rnd, y16=False):
    """the same layer in float32 with stock torch on the host, operands rounded where the launch would round them: the executor of the
    CPU companion's bar check.  -> (outputs, act)"""
    f = lambda t: None if t is None else t.float()
    r = lambda t, on: t.to(torch.bfloat16).float() if on else t
    x, W, b, dy = f(inp["x"]), f(inp["W"]), f(inp["b"]), f(inp["dy"])
    z = r(x, rnd["fwd"]) @ r(W, rnd["fwd"]).t()
    if b is not None:
        z = z + b
    y = torch.relu(z) if relu else z
    if keep_s is not None:
        y = y * keep_s.float()
    if y16:
        y = y.to(torch.bfloat16).float()
    s = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    dz = dy
    if relu:
        dz = dy * (y > 0).float() * (s if keep_s is not None else 1.0)
    elif keep_s is not None:
        dz = dy * (keep_s > 0).float() * s
    return {"y": y, "dx": r(dz, rnd["dx"]) @ r(W, rnd["dx"]), "dW": r(dz, rnd["dw"]).t() @ r(x, rnd["dw"]), "db": dz.sum(0)}, y > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# feed-forward

class FfnCase:
    def __init__(self, name, M, K, F, N, p=0.0, need_dx=True, x_kind="plain", modes=MODES, expect=None):
        self.name, self.M, self.K, self.F, self.N, self.p, self.need_dx, self.x_kind, self.modes = name, M, K, F, N, p, need_dx, x_kind, modes
        self.expect = dict(expect or {})

    def __repr__(self):
        return f"ffn[{self.name} {self.M}x{self.K}x{self.F}x{self.N} p={self.p} dx={self.need_dx} x={self.x_kind}]"

    def chained(self, mode):
        return ffn_chain_ok(mode, self.K, self.F, self.N) and self.x_kind != "offset"

    def h16(self, mode):
        return self.chained(mode) or (ffn_h16(mode, self.K, self.F, self.N) and self.x_kind != "offset")

    def inputs(self):
        g = gen(7 * self.M + 13 * self.K + 17 * self.F + int(self.p * 100) + len(self.name))
        return dict(x=torch.randn(self.M, self.K, generator=g), W1=torch.randn(self.F, self.K, generator=g) / self.K ** 0.5,
                    b1=torch.randn(self.F, generator=g) * 0.3, W2=torch.randn(self.N, self.F, generator=g) / self.F ** 0.5,
                    b2=torch.randn(self.N, generator=g) * 0.3, df=torch.randn(self.M, self.N, generator=g),
                    res=torch.randn(self.M, self.K, generator=g), gamma=1.0 + 0.3 * torch.randn(self.N, generator=g),
                    beta=0.3 * torch.randn(self.N, generator=g), df2=torch.randn(self.M, self.N, generator=g))


def ffn_cases():
    out = []
    for M, K, F, N in ((33, 20, 36, 20), (130, 64, 72, 64), (515, 128, 64, 128)):
        for p, need_dx in itertools.product((0.0, 0.1), (True, False)):
            # (the first is the small model whose hidden layer stays fp32 in the reduced-precision mode; the last is chained there)
            out.append(FfnCase("plain", M, K, F, N, p, need_dx, expect={"dw_ksplit": M == 515}))
    for F, M in itertools.product((64, 2048), (1, 33, 130)):
        out.append(FfnCase("chain", M, 128, F, 128, 0.1 if M == 130 else 0.0, modes=("bf16",), expect={"chain": True}))
        out.append(FfnCase("chain", M, 128, F, 128, 0.1 if M == 130 else 0.0, x_kind="offset", modes=("bf16",), expect={"chain": False}))
    for F in (96, 2112):
        out.append(FfnCase("nochain", 33, 128, F, 128, 0.1, modes=("bf16",), expect={"chain": False}))
    return out


def ffn_reference(inp, k1s, k2s, h_dev, p, rnd, h16, eps_dx, eps_dw):
    """float64 (ref, bar) of a feed-forward block, stage by stage.  k1s / k2s: keep / (1 - p) of the hidden (M, F) and the output (M, N)
    dropout, or None; h_dev: the hidden layer as the executor STORED it (float64 of its fp32 or bf16 values): the operand of every
    product behind it and the ReLU-and-dropout mask of the backward (h > 0: active and kept); rnd: {"h", "f", "dw2", "dz1", "dx", "dw1"}
    -> the launch rounds its fp32 operands to bf16; h16: the hidden layer and its gradient are stored as bf16."""
    x, W1, b1, W2, b2, df = (inp[k] for k in ("x", "W1", "b1", "W2", "b2", "df"))
    r = lambda t, on: _bf16_round(t) if on else t
    out = {}
    xa, Wa = r(x, rnd["h"]), r(W1, rnd["h"])
    h = (xa @ Wa.t() + b1).clamp_min(0.0)
    mag = xa.abs() @ Wa.abs().t() + b1.abs()
    if k1s is not None:
        h, mag = h * k1s, mag * k1s
    out["h"] = (h, BAR_FP32 * mag + (BF16_STORE * h.abs() if h16 else 0.0))
    ha, Wb = r(h_dev, rnd["f"]), r(W2, rnd["f"])
    f = ha @ Wb.t() + b2
    mag = ha.abs() @ Wb.abs().t() + b2.abs()
    if k2s is not None:
        f, mag = f * k2s, mag * k2s
    out["f"] = (f, BAR_FP32 * mag)
    s = 1.0 / (1.0 - p)
    dz2 = scale32(df * (k2s > 0).double(), p) if k2s is not None else df
    e_dz2 = MASK_PASS * dz2.abs() if k2s is not None else torch.zeros_like(dz2)
    out["db2"] = (dz2.sum(0), _colsum_bar(dz2) + e_dz2.sum(0))
    a, bm = r(dz2, rnd["dw2"]), r(h_dev, rnd["dw2"])
    out["dW2"] = (a.t() @ bm, eps_dw * (a.abs().t() @ bm.abs()) + e_dz2.t() @ bm.abs())
    act = (h_dev > 0).double() * (s if k1s is not None else 1.0)
    a, bm = r(dz2, rnd["dz1"]), r(W2, rnd["dz1"])
    dz1 = (a @ bm) * act
    e_dz1 = (eps_dx * (a.abs() @ bm.abs()) + e_dz2 @ bm.abs()) * act + (BF16_STORE * dz1.abs() if h16 else 0.0)
    out["db1"] = (dz1.sum(0), _colsum_bar(dz1) + e_dz1.sum(0))
    for name, a, bm, on, eps in (("dx", dz1, W1, rnd["dx"], eps_dx), ("dW1", dz1.t(), x, rnd["dw1"], eps_dw)):
        b_r = r(bm, on)
        e_a = e_dz1 + (BF16_STORE * dz1.abs() if (on and not h16) else 0.0)       # (an fp32 dz1 is rounded on its way into a bf16 launch)
        e_a = e_a if name == "dx" else e_a.t()
        out[name] = (a @ b_r, eps * (a.abs() @ b_r.abs()) + e_a @ b_r.abs())
    return out


def ffn_float32(inp, k1s, k2s, p, rnd, h16):
    """the block in float32 with stock torch on the host, rounding where the launches round and storing h / dz1 as bf16 where they do"""
    x, W1, b1, W2, b2, df = (inp[k].float() for k in ("x", "W1", "b1", "W2", "b2", "df"))
    r = lambda t, on: t.to(torch.bfloat16).float() if on else t
    h = torch.relu(r(x, rnd["h"]) @ r(W1, rnd["h"]).t() + b1)
    if k1s is not None:
        h = h * k1s.float()
    h = r(h, h16)
    f = r(h, rnd["f"]) @ r(W2, rnd["f"]).t() + b2
    s = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    dz2 = df
    if k2s is not None:
        f, dz2 = f * k2s.float(), df * (k2s > 0).float() * s
    dz1 = (r(dz2, rnd["dz1"]) @ r(W2, rnd["dz1"])) * (h > 0).float() * (s if k1s is not None else 1.0)
    db1 = dz1.sum(0)
    dz1 = r(dz1, h16)
    return {"h": h, "f": f, "db2": dz2.sum(0), "dW2": r(dz2, rnd["dw2"]).t() @ r(h, rnd["dw2"]), "db1": db1, "dx": r(dz1, rnd["dx"]) @ r(W1, rnd["dx"]),
            "dW1": r(dz1, rnd["dw1"]).t() @ r(x, rnd["dw1"])}


# ---------------------------------------------------------------------------------------------------------------------------------
# layer norm

LN_D, LN_ROWS = (128, 20, 1024), (1, 257)


def ln_inputs(rows, d, seed=0):
    g = gen(17 * rows + d + seed)
    sc = 0.5 + torch.rand(rows, 1, generator=g) * 3.0
    return dict(x=torch.randn(rows, d, generator=g) * sc + torch.randn(rows, 1, generator=g), res=torch.randn(rows, d, generator=g) * sc,
                gamma=1.0 + 0.3 * torch.randn(d, generator=g), beta=0.3 * torch.randn(d, generator=g),
                dy=torch.randn(rows, d, generator=g), dy2=torch.randn(rows, d, generator=g))


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: the composed path's head dims 16 and 20 are judged with the fused path's float64 reference and magnitudes (head dim 32)
# by embedding: every head zero-padded to 32 dims and q scaled by sqrt(32 / dh), so that q' . k' / sqrt(32) = q . k / sqrt(dh)

def embed32(qkv64, dout64, H, dh):
    Bn, S, _ = qkv64.shape
    d = H * dh
    c = (32.0 / dh) ** 0.5
    out = torch.zeros(Bn, S, 3, H, 32, dtype=torch.float64)
    out[..., :dh] = qkv64.reshape(Bn, S, 3, H, dh)
    out[:, :, 0] *= c
    do = torch.zeros(Bn, dout64.shape[1], H, 32, dtype=torch.float64)
    do[..., :dh] = dout64.reshape(Bn, -1, H, dh)
    return out.reshape(Bn, S, 3 * H * 32), do.reshape(Bn, -1, H * 32), c


def unembed32(out32, dqkv32, H, dh, c):
    """(out, dqkv) of the embedded problem back in the dh-wide layout (the gradient w.r.t. q' is 1 / c of the one w.r.t. q)"""
    Bn, S = dqkv32.shape[:2]
    out = out32.reshape(Bn, -1, H, 32)[..., :dh].reshape(Bn, -1, H * dh)
    g = dqkv32.reshape(Bn, S, 3, H, 32)[..., :dh].clone()
    g[:, :, 0] *= c
    return out, g.reshape(Bn, S, 3 * H * dh)


ATTN_BIAS = ("null", "plus1", "cut", "full")
ATTN_NQ = (None, 1, 21, 33, 40)

"""Device conformance matrix of the GEMM family and the fused attention kernels against float64.

The emulator tests (tests/test_emu_kernels.py) cover the same kernels on a CPU, through a hand-written model of MFMA, DPP and the
lane crossings; the model-level GPU tests run the kernels at the shipped shapes only.  Here every case calls a C entry point directly
(`ops._lib()`, explicit flags: nothing is added from the global precision mode), so each case decides which kernel runs, and checks it
against a float64 torch reference of the same operation:

- emloco_gemm_f32_ex over the four precision modes (fp32, split, split2, bf16), the four layouts, ragged m / n / k, batch 3 with loose
  batch strides, unaligned bases and leading dimensions (the scalar-load kernels), the small / large split tile (same bits), the 32-deep
  stage, split k with a workspace, the piece image of B (same bits as the matrix), bf16 operands / output in memory and every epilogue.
  The output carries guard bands: slack columns, slack between batches and a tail, all holding a sentinel that must survive, and the
  logical output is NaN before every non-accumulating launch, so an element the kernel never writes fails.  Operand padding (beyond the
  logical rows / columns inside the leading dimension and the strides) holds large values that would show if a kernel read them.
- emloco_gemm_relu_bwd (every gemm_pick branch of the fused backward epilogue), emloco_colsum_ex and emloco_act_bwd_colsum at tall
  ragged row counts.
- emloco_attention_{fwd,bwd}_queries over the four modes (fp32, split, bf16, bf16 q|k|v in memory), S from 1 to 453, 1 / 4 / 8 heads,
  zero / +1 / -inf key biases (cut at 32 t - 1, 32 t, 32 t + 1, and a fully masked sequence), dropout with the library's own mask, and
  n_query in {1, 21, S}; out / dqkv / lse / dsum with guard bands.

Errors of the GEMM are measured against mag = |A| @ |B|^T (plus |bias| and |C| where they enter), the error scale of a dot product.

Not covered (variants reachable only through environment knobs read once when the library loads): EMLOCO_ATTN16_OLD (round 4's
attention kernels for the bf16-in-memory and split modes), EMLOCO_ATTN_BWD_PIECES=3 (the three-piece split attention backward),
EMLOCO_GEMM_WIDE_STORES=0 (per-register GEMM stores everywhere) and EMLOCO_GEMM_BK (a forced stage depth: the only way to reach the
32-deep kernels of the (trans_a, trans_b) = (1, 1) layout).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
FP32, SPLIT, SPLIT2, BF16 = 0, 1024, 1024 | 4096, 16
MODES = {"fp32": FP32, "split": SPLIT, "split2": SPLIT2, "bf16": BF16}
BIAS, RELU, ACC, DROP = 1, 2, 4, 8
A16, B16, C16, MASK16, IMG = 64, 128, 256, 512, 2048
SENT = -777.25                          # guard-band sentinel (fp32)
SENT16 = 0x1234                         # guard-band sentinel (bf16 bits)
NAN16 = 0x7FC0
GARBAGE = 1.0e6                         # operand padding: would dominate any element whose reduction read it
TAIL = 64                               # guard elements behind every output

BAR_FP32 = 2e-6                         # include/emloco_predictor.h: 1e-7 .. 2e-6 of sum |a b| (fp32 and split)
BAR_SPLIT2 = 3 * 2.0 ** -16             # two pieces: the three dropped piece products are each <= 2^-16 of |a| |b|


def _lib():
    from emloco_amd.predictor import ops
    return ops._lib()


def _ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + t.element_size() * off)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _bf16_round(x):
    """round-to-nearest-even to bf16, back as float64"""
    return x.float().to(torch.bfloat16).double()


class small_tile:
    """emloco_gemm_set_small_tile(mode) for a block, the launcher's default (-1) restored after it"""
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        assert _lib().emloco_gemm_set_small_tile(self.mode) == 0

    def __exit__(self, *exc):
        _lib().emloco_gemm_set_small_tile(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# strided operands and guarded outputs

def _operand(gen, batch, rows, cols, ld, stride, off, bf16=False, scale=1.0):
    """A buffer holding `batch` rows x cols matrices at element offset `off`, leading dimension ld, batch stride `stride`; everything
    outside them is GARBAGE.  Returns (buffer, logical float64 values as stored [batch][rows][cols])."""
    total = off + (batch - 1) * stride + (rows - 1) * ld + cols + TAIL
    buf = torch.randn(total, generator=gen, device=DEV) * GARBAGE
    val = torch.randn(batch, rows, cols, generator=gen, device=DEV) * scale
    if bf16:
        buf, val = buf.to(torch.bfloat16), val.to(torch.bfloat16)
    buf.as_strided((batch, rows, cols), (stride, ld, 1), off).copy_(val)
    return buf, val.double()


class _Guarded:
    """an output of `batch` x rows x cols at offset `off`, leading dimension ld, batch stride `stride`, sentinel everywhere else"""

    def __init__(self, batch, rows, cols, ld, stride, off, bf16=False):
        self.shape, self.strides, self.off, self.bf16 = (batch, rows, cols), (stride, ld, 1), off, bf16
        total = off + (batch - 1) * stride + (rows - 1) * ld + cols + TAIL
        if bf16:
            self.buf = torch.full((total,), SENT16, dtype=torch.int16, device=DEV)
        else:
            self.buf = torch.full((total,), SENT, dtype=torch.float32, device=DEV)
        self.inside = torch.zeros(total, dtype=torch.bool, device=DEV)
        self.inside.as_strided(self.shape, self.strides, off).fill_(True)
        self.before = self.buf.clone()

    def view(self):
        return self.buf.as_strided(self.shape, self.strides, self.off)

    def fill(self, values=None):
        """NaN into the logical output (or the given values, for an accumulating launch)"""
        v = self.view()
        if values is None:
            v.fill_(NAN16 if self.bf16 else float("nan"))
        elif self.bf16:
            v.copy_(values.to(torch.bfloat16).view(torch.int16))
        else:
            v.copy_(values)
        self.before = self.buf.clone()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.buf.element_size() * self.off)

    def got(self):
        """(logical output as float64, its raw bits) after checking that nothing outside it changed"""
        outside = ~self.inside
        assert torch.equal(_bits(self.buf)[outside], _bits(self.before)[outside]), "a store landed outside the output (guard band changed)"
        v = self.view()
        if self.bf16:
            return v.contiguous().view(torch.bfloat16).double(), v.contiguous()
        return v.double(), v.contiguous()


def _gemm_launch(lib, batch, m, n, k, alpha, A, a_off, lda, sa, ta, B, b_off, ldb, sb, tb, out, ldc, sc, bias, flags, ksplit, p=0.0, seed=0):
    ws = torch.empty(max(ksplit, 1) * batch * m * n + TAIL, device=DEV) if ksplit > 1 else None
    return lib.emloco_gemm_f32_ex(batch, m, n, k, float(alpha), _ptr(A, a_off), lda, sa, ta, _ptr(B, b_off), ldb, sb, tb, out.ptr(), ldc, sc,
                                  _ptr(bias), flags, ksplit, _ptr(ws), float(p), seed & 0xFFFFFFFF, _stream())


def _vec(buf, off, ld, stride):
    return (buf.data_ptr() + buf.element_size() * off) % 16 == 0 and ld % 4 == 0 and stride % 4 == 0


def _ru4(x):
    return (x + 3) // 4 * 4


class GemmCase:
    """One launch of emloco_gemm_f32_ex and its float64 reference."""

    def __init__(self, batch, m, n, k, ta=0, tb=0, mode="fp32", alpha=1.0, epi=0, ksplit=1, a_off=0, b_off=0, c_off=0, ld_pad=0,
                 loose=0, mem=0, p=0.0, tile=-1, seed=0):
        self.batch, self.m, self.n, self.k, self.ta, self.tb, self.mode = batch, m, n, k, ta, tb, mode
        self.alpha, self.epi, self.ksplit, self.mem, self.p, self.tile = alpha, epi, ksplit, mem, p, tile
        self.a_off, self.b_off, self.c_off, self.ld_pad, self.loose, self.seed = a_off, b_off, c_off, ld_pad, loose, seed
        # ld_pad < 0: leading dimensions rounded up to a multiple of 4 (the 16-byte-load kernels); >= 0: row + ld_pad
        ra, ca = (k, m) if ta else (m, k)
        rb, cb = (k, n) if tb else (n, k)
        pad = (lambda c: _ru4(c) + (-ld_pad - 1)) if ld_pad < 0 else (lambda c: c + ld_pad)
        self.lda, self.ldb = pad(ca), pad(cb)
        self.ldc = n if epi & DROP else pad(n)
        self.ra, self.ca, self.rb, self.cb = ra, ca, rb, cb
        self.sa = ra * self.lda + loose if batch > 1 else 0
        self.sb = rb * self.ldb + loose if batch > 1 else 0
        self.sc = m * self.ldc + (0 if epi & DROP else loose) if batch > 1 else 0

    def __repr__(self):
        return (f"GemmCase(batch={self.batch}, m={self.m}, n={self.n}, k={self.k}, ta={self.ta}, tb={self.tb}, mode={self.mode}, "
                f"alpha={self.alpha}, epi={self.epi}, ksplit={self.ksplit}, off=({self.a_off},{self.b_off},{self.c_off}), "
                f"ld=({self.lda},{self.ldb},{self.ldc}), loose={self.loose}, mem={self.mem}, p={self.p}, tile={self.tile})")

    def make(self):
        g = torch.Generator(device=DEV)
        g.manual_seed(1000003 * self.seed + 7 * self.m + 13 * self.n + 17 * self.k + 3 * self.ta + 5 * self.tb)
        sa_ = self.sa if self.batch > 1 else 0
        sb_ = self.sb if self.batch > 1 else 0
        self.A, a = _operand(g, self.batch, self.ra, self.ca, self.lda, sa_, self.a_off, bool(self.mem & A16))
        self.B, b = _operand(g, self.batch, self.rb, self.cb, self.ldb, sb_, self.b_off, bool(self.mem & B16))
        self.Al = a.transpose(1, 2) if self.ta else a          # [batch][m][k]
        self.Bl = b.transpose(1, 2) if self.tb else b          # [batch][n][k]
        self.bias = torch.randn(self.n, generator=g, device=DEV) if self.epi & BIAS else None
        self.c0 = torch.randn(self.batch, self.m, self.n, generator=g, device=DEV) if self.epi & ACC else None
        if self.c0 is not None and self.mem & C16:
            self.c0 = self.c0.to(torch.bfloat16).float()
        self.vec = _vec(self.A, self.a_off, self.lda, self.sa) and _vec(self.B, self.b_off, self.ldb, self.sb)

    def flags(self):
        f = MODES[self.mode] | self.epi | self.mem
        return f

    def effective(self):
        """the precision class the launcher serves this case in (include/emloco_predictor.h: split needs 16-byte-aligned operands and
        n > 32, else the plain fp32 kernel; the bf16 operand path likewise)"""
        if self.mode in ("split", "split2"):
            return self.mode if self.vec and self.n > 32 else "fp32"
        if self.mode == "bf16":
            return "bf16" if self.vec and self.n > 32 else "fp32"
        return "fp32"

    def out(self, flags=None):
        c16 = bool((self.flags() if flags is None else flags) & C16)
        o = _Guarded(self.batch, self.m, self.n, self.ldc, self.sc if self.batch > 1 else 0, self.c_off, c16)
        o.fill(self.c0)
        return o

    def run(self, lib, flags=None, B=None, b_off=None):
        o = self.out(flags)
        with small_tile(self.tile):
            rc = _gemm_launch(lib, self.batch, self.m, self.n, self.k, self.alpha, self.A, self.a_off, self.lda, self.sa, self.ta,
                              self.B if B is None else B, self.b_off if b_off is None else b_off, self.ldb, self.sb, self.tb, o, self.ldc,
                              self.sc, self.bias, self.flags() if flags is None else flags, self.ksplit, self.p, 0xC0FFEE + self.seed)
        assert rc == 0, ("launch refused", self)
        torch.cuda.synchronize()
        return o

    def keep(self, lib):
        n = self.batch * self.m * self.n
        h = np.zeros(n, np.uint8)
        assert lib.emloco_dropout_keep_mask(0xC0FFEE + self.seed, 0, n, self.p, h.ctypes.data_as(C.c_void_p)) == 0
        return torch.from_numpy(h.reshape(self.batch, self.m, self.n)).to(DEV).double()

    def reference(self, lib, rounded):
        a, b = (_bf16_round(self.Al), _bf16_round(self.Bl)) if rounded else (self.Al, self.Bl)
        ref = self.alpha * (a @ b.transpose(1, 2))
        mag = abs(self.alpha) * (a.abs() @ b.abs().transpose(1, 2))
        if self.bias is not None:
            ref = ref + self.bias.double()
            mag = mag + self.bias.double().abs()
        if self.epi & RELU:
            ref = ref.clamp_min(0.0)
        if self.epi & DROP:
            s = 1.0 / (1.0 - self.p)
            ref = ref * self.keep(lib) * s
            mag = mag * s
        if self.c0 is not None:
            ref = ref + self.c0.double()
            mag = mag + self.c0.double().abs()
        return ref, mag


def _rel_err(got, ref, mag):
    assert torch.isfinite(got).all(), "non-finite output (an element not written, or a bad value)"
    return ((got - ref).abs() / mag.clamp_min(1e-30)).max().item()


def _check_gemm(lib, case):
    case.make()
    if case.mem & C16:
        # the bf16 output is the RNE rounding of the fp32 result of the same launch (same kernel, fp32 C) ...
        bits = case.run(lib).got()[1]
        got = case.run(lib, flags=case.flags() & ~C16).got()[0]
        want = got.float().to(torch.bfloat16).view(torch.int16)
        assert torch.equal(bits, want), ("bf16 output is not the RNE rounding of the fp32 result", case)
    else:
        got = case.run(lib).got()[0]
    eff = case.effective()
    if eff == "bf16":                   # ... which is checked like any other
        ref, mag = case.reference(lib, rounded=True)
        err = _rel_err(got, ref, mag)
        assert err <= BAR_FP32, ("bf16 mode vs float64 on the rounded operands", case, err)
        if (case.mem & (A16 | B16)) != (A16 | B16):            # (two bf16 operands in memory: nothing left to round)
            ref_full, mag_full = case.reference(lib, rounded=False)
            full = _rel_err(got, ref_full, mag_full)
            assert full > 1e-4, ("bf16 mode is not visibly reduced precision", case, full)
        return
    ref, mag = case.reference(lib, rounded=False)
    err = _rel_err(got, ref, mag)
    if eff == "split2":
        assert err <= BAR_SPLIT2, ("split2 vs float64", case, err)
        three = case.run(lib, flags=case.flags() & ~4096)
        err3 = _rel_err(three.got()[0], ref, mag)
        assert err3 <= BAR_FP32 and err > err3, ("split2 must be coarser than the three-piece product", case, err, err3)
    else:
        assert err <= BAR_FP32, (eff, "vs float64", case, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. GEMM matrix

LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
# ragged shapes: narrow (n <= 32, the 128 x 32 tile), wide, long reductions (k > 256 on few workgroups: the 32-deep stage)
RAGGED = [(1, 33, 1), (33, 1, 15), (129, 31, 17), (300, 65, 44), (129, 129, 257), (1, 264, 521), (300, 32, 257), (33, 64, 17),
          (300, 129, 521)]


def _ragged_cases():
    out = []
    for (m, n, k) in RAGGED:
        for ta, tb in LAYOUTS:
            for mode in MODES:
                out.append(GemmCase(1, m, n, k, ta, tb, mode, ld_pad=-1))
    return out


def _alignment_cases():
    out = []
    for (m, n, k) in ((129, 65, 44), (300, 264, 300), (33, 31, 257)):
        for ta, tb in LAYOUTS:
            for mode in MODES:
                out.append(GemmCase(1, m, n, k, ta, tb, mode, a_off=1, b_off=4, c_off=1, ld_pad=3))       # scalar loads, loose ldc
                out.append(GemmCase(1, m, n, k, ta, tb, mode, a_off=4, b_off=4, c_off=4, ld_pad=-5))      # 16-byte loads, ldc = ru4(n) + 4
                out.append(GemmCase(1, m, n, k, ta, tb, mode, a_off=4, b_off=1, c_off=0, ld_pad=-1))      # one operand unaligned
    return out


def _batch_cases():
    out = []
    for ta, tb in LAYOUTS:
        for mode in MODES:
            out.append(GemmCase(3, 33, 65, 44, ta, tb, mode, ld_pad=-1, loose=8, c_off=4))
            out.append(GemmCase(3, 129, 31, 17, ta, tb, mode, ld_pad=3, loose=5, c_off=1))
            out.append(GemmCase(3, 65, 129, 300, ta, tb, mode, ld_pad=-1, loose=12, ksplit=2, epi=BIAS))
    return out


def _epilogue_cases():
    out = []
    for i, (ta, tb) in enumerate(LAYOUTS):
        for j, mode in enumerate(MODES):
            s = 4 * i + j
            out.append(GemmCase(1, 300, 129, 44, ta, tb, mode, alpha=-1.25, epi=BIAS | RELU, ld_pad=-1, seed=s))
            out.append(GemmCase(1, 129, 65, 257, ta, tb, mode, alpha=0.5, epi=ACC, ld_pad=-1, seed=s))
            out.append(GemmCase(1, 33, 31, 15, ta, tb, mode, epi=BIAS | ACC, ld_pad=3, a_off=1, seed=s))
            out.append(GemmCase(1, 129, 264, 44, ta, tb, mode, epi=BIAS | RELU | DROP, p=0.1, ld_pad=-1, seed=s))
            out.append(GemmCase(2, 65, 33, 17, ta, tb, mode, epi=RELU | DROP, p=0.3, ld_pad=-1, seed=s))
            out.append(GemmCase(1, 300, 65, 17, ta, tb, mode, epi=BIAS | ACC | DROP, p=0.1, ld_pad=-1, seed=s))
            for ks in (2, 3, 7):
                out.append(GemmCase(1, 129, 65, 300, ta, tb, mode, alpha=0.75, epi=BIAS | RELU, ksplit=ks, ld_pad=-1, seed=s))
            out.append(GemmCase(1, 33, 129, 17, ta, tb, mode, ksplit=7, epi=ACC, ld_pad=-1, seed=s))
            out.append(GemmCase(2, 129, 31, 44, ta, tb, mode, ksplit=3, epi=BIAS | DROP, p=0.2, ld_pad=-1, seed=s))
    return out


def _threshold_cases():
    """the launcher's small-tile choice at its threshold (GEMM_SMALL_MAX_WG = 128 workgroups of the 128 x 128 grid, split k included)"""
    out = []
    for mode in ("split", "split2"):
        for ta, tb in LAYOUTS:
            out.append(GemmCase(1, 8192, 129, 20, ta, tb, mode, ld_pad=-1))          # 64 x 2 = 128: the small tile
            out.append(GemmCase(1, 8193, 129, 20, ta, tb, mode, ld_pad=-1))          # 65 x 2 = 130: the large tile
        out.append(GemmCase(1, 4096, 129, 40, 0, 0, mode, ksplit=2, ld_pad=-1))      # 32 x 2 x 2 = 128
        out.append(GemmCase(1, 4097, 129, 40, 0, 0, mode, ksplit=2, ld_pad=-1))      # 33 x 2 x 2 = 132
    return out


def _mem_cases():
    """bf16 operands / output in memory: every combination the launcher serves"""
    out = []
    for ta, tb in LAYOUTS:
        for (m, n, k) in ((300, 65, 44), (129, 129, 300), (33, 264, 20)):
            out.append(GemmCase(1, m, n, k, ta, tb, "bf16", mem=A16, ld_pad=-1))
            out.append(GemmCase(1, m, n, k, ta, tb, "bf16", mem=C16, ld_pad=-1, epi=BIAS))
            out.append(GemmCase(1, m, n, k, ta, tb, "bf16", mem=A16 | C16, ld_pad=-5, epi=ACC))
        out.append(GemmCase(1, 256, 256, 44, ta, tb, "bf16", mem=C16, ld_pad=-1, epi=BIAS | RELU))      # whole tiles: 16-byte bf16 stores
        out.append(GemmCase(3, 65, 129, 44, ta, tb, "bf16", mem=A16, ld_pad=-1, loose=8, epi=BIAS | RELU))
        out.append(GemmCase(1, 129, 65, 300, ta, tb, "bf16", mem=A16, ld_pad=-1, ksplit=3, epi=BIAS))
    for (m, n, k) in ((300, 65, 44), (129, 129, 257), (33, 264, 20), (1, 33, 1)):     # the weight-gradient layout
        out.append(GemmCase(1, m, n, k, 1, 1, "bf16", mem=B16, ld_pad=-1))
        out.append(GemmCase(1, m, n, k, 1, 1, "bf16", mem=A16 | B16, ld_pad=-1))
        out.append(GemmCase(1, m, n, k, 1, 1, "bf16", mem=A16 | B16 | C16, ld_pad=-1, epi=BIAS | RELU))
        out.append(GemmCase(1, m, n, k, 1, 1, "bf16", mem=A16 | B16, ld_pad=-1, ksplit=2, epi=ACC))
    out.append(GemmCase(2, 65, 129, 44, 1, 1, "bf16", mem=A16 | B16, ld_pad=-1, loose=8))
    return out


@pytest.mark.parametrize("group", ["ragged", "alignment", "batch", "epilogue", "threshold", "mem"])
def test_gemm_matrix_against_float64(group):
    """every case of the group: float64 bar of its precision class, guard bands intact, every output element written"""
    lib = _lib()
    cases = {"ragged": _ragged_cases, "alignment": _alignment_cases, "batch": _batch_cases, "epilogue": _epilogue_cases,
             "threshold": _threshold_cases, "mem": _mem_cases}[group]()
    failed = []
    for case in cases:
        try:
            _check_gemm(lib, case)
        except AssertionError as e:         # every failing case of the group in one report
            failed.append(str(e))
    assert not failed, f"{len(failed)} of {len(cases)} cases failed:\n" + "\n".join(failed)


@pytest.mark.parametrize("mode", ["split", "split2"])
def test_gemm_split_tiles_give_the_same_bits(mode):
    """include/emloco_predictor.h: the 64 x 64 and the 128 x 128 split tile reduce an output element in the same order -- bit-equal
    (the emulator's claim, tests/test_emu_kernels.py), on every layout, ragged, with split k and with epilogues; both within the bar"""
    lib = _lib()
    for (m, n, k, ks, epi) in ((300, 264, 44, 1, 0), (129, 65, 257, 1, BIAS | RELU), (33, 129, 17, 3, ACC), (257, 33, 300, 2, BIAS)):
        for ta, tb in LAYOUTS:
            case = GemmCase(1, m, n, k, ta, tb, mode, epi=epi, ksplit=ks, ld_pad=-1, seed=m + ta)
            case.make()
            res = {}
            for tile in (0, 1):
                case.tile = tile
                res[tile] = case.run(lib).got()
            assert torch.equal(res[0][1], res[1][1]), ("small and large tile differ", case)
            ref, mag = case.reference(lib, rounded=False)
            err = _rel_err(res[1][0], ref, mag)
            assert err <= (BAR_FP32 if mode == "split" else BAR_SPLIT2), ("small tile vs float64", case, err)


def test_gemm_piece_image_gives_the_same_bits_as_the_matrix():
    """EMLOCO_GEMM_B_SPLITIMG: B as its piece image, packed from either layout of the weight, on both tiles, with split k and an
    epilogue -- bit-equal to the launch on the matrix; with EMLOCO_GEMM_SPLIT2 the image (three pieces) wins: the three-piece bits"""
    lib = _lib()
    for (m, n, k, ks, epi) in ((300, 129, 44, 1, 0), (129, 264, 257, 1, BIAS | RELU), (1, 33, 17, 1, 0), (65, 65, 300, 3, BIAS)):
        for trans in (0, 1):
            for tile in (0, 1):
                case = GemmCase(1, m, n, k, 0, trans, "split", epi=epi, ksplit=ks, ld_pad=-1, tile=tile, seed=trans)
                case.make()
                want = case.run(lib).got()[1]
                words = lib.emloco_gemm_split_image_words(n, k)
                img = torch.full((words + TAIL,), -1, dtype=torch.int32, device=DEV)
                assert lib.emloco_gemm_split_pack(_ptr(case.B, case.b_off), n, k, case.ldb, trans, _ptr(img), _stream()) == 0
                for extra in (0, 4096):
                    got = case.run(lib, flags=case.flags() | IMG | extra, B=img, b_off=0).got()[1]
                    assert torch.equal(got, want), ("piece image differs from the matrix", case, extra)
                assert (img[words:] == -1).all(), ("the packer wrote past the image", n, k)


@pytest.mark.parametrize("mode", ["split", "split2"])
def test_gemm_non_finite_operands_on_every_layout_and_tile(mode):
    """include/emloco_predictor.h, NON-FINITE AND HUGE OPERANDS: an Inf, a NaN or a finite value above bf16's range makes the output
    elements whose reduction it enters non-finite (NaN in the three-piece mode); every other element equals the clean product bit for
    bit -- all four layouts, both split tiles (test_gpu_predictor.py covers the (0, 0) layout by default tile)"""
    lib = _lib()
    m, n, k = 300, 264, 512
    for ta, tb in LAYOUTS:
        for tile in (0, 1):
            case = GemmCase(1, m, n, k, ta, tb, mode, ld_pad=-1, tile=tile, seed=ta + 2 * tb)
            case.make()
            clean = case.run(lib).got()[0]
            A, B = case.A.clone(), case.B.clone()
            sa = case.A.as_strided((case.ra, case.ca), (case.lda, 1), case.a_off)
            sb = case.B.as_strided((case.rb, case.cb), (case.ldb, 1), case.b_off)
            def at(r, c, t):         # logical (row, k) of A / (col, k) of B to stored (row, col)
                return (c, r) if t else (r, c)
            sa[at(5, 7, ta)] = float("inf")
            sa[at(140, 300, ta)] = 3.40e38
            sb[at(200, 3, tb)] = float("nan")
            got = case.run(lib).got()[0]
            case.A.copy_(A); case.B.copy_(B)
            bad = torch.zeros(m, n, dtype=torch.bool, device=DEV)
            bad[5, :] = True; bad[140, :] = True; bad[:, 200] = True
            g = got[0]
            if mode == "split":
                assert torch.isnan(g[bad]).all(), ("non-finite operands must give NaN", case)
            else:
                assert (~torch.isfinite(g[bad])).all(), ("non-finite operands must give non-finite outputs", case)
            assert torch.equal(g[~bad], clean[0][~bad]), ("clean elements changed", case)


def test_gemm_launcher_refuses_what_it_does_not_serve():
    """combinations outside the stated limits are refused with an error and leave the output alone"""
    lib = _lib()
    bad = [GemmCase(1, 65, 65, 44, 0, 0, "bf16", mem=B16, ld_pad=-1),           # bf16 B: the weight-gradient layout only
           GemmCase(1, 65, 65, 44, 1, 0, "bf16", mem=A16 | B16, ld_pad=-1),
           GemmCase(1, 65, 31, 44, 0, 0, "bf16", mem=A16, ld_pad=-1),           # n <= 32
           GemmCase(1, 65, 65, 44, 0, 0, "fp32", mem=A16, ld_pad=-1),           # bf16 memory without EMLOCO_GEMM_BF16
           GemmCase(1, 65, 65, 44, 0, 0, "bf16", mem=A16, a_off=1, ld_pad=3),   # unaligned bf16 operand
           GemmCase(1, 65, 65, 44, 0, 0, "bf16", mem=C16, ksplit=2, ld_pad=-1)]  # bf16 output split along k
    for case in bad:
        case.make()
        o = case.out()
        with small_tile(-1):
            rc = _gemm_launch(lib, 1, case.m, case.n, case.k, 1.0, case.A, case.a_off, case.lda, case.sa, case.ta, case.B, case.b_off,
                              case.ldb, case.sb, case.tb, o, case.ldc, case.sc, None, case.flags(), case.ksplit)
        torch.cuda.synchronize()
        assert rc != 0, ("accepted", case)
        assert torch.equal(_bits(o.buf), _bits(o.before)), ("a refused launch wrote", case)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the fused backward epilogue and the column sums

def _colsum_bar(x64):
    """fp32 summation error of a fixed-order column sum: a few hundred units of 2^-24 of sum |x|"""
    return 1e-5 * x64.abs().sum(0) + 1e-30


# (m, n, k, tb, mode, hidden16): every gemm_pick branch of the fused epilogue -- split3 / split2 / split + image, fp32 and bf16 operands
# on the 16- and 32-deep stage (k > 256 on at most 1024 workgroups), the bf16 hidden layer
RELU_BWD = []
for _tb in (0, 1):
    for _m, _n, _k in ((4 * 453 + 7, 129, 64), (4 * 453 + 7, 264, 300), (100003, 65, 36)):
        for _mode in ("split", "split2", "fp32", "bf16", "bf16mem"):
            RELU_BWD.append((_m, _n, _k, _tb, _mode))
RELU_BWD += [(4 * 453 + 7, 129, 64, 0, "split_img"), (4 * 453 + 7, 264, 300, 1, "split_img"), (100003, 65, 36, 0, "split_img")]


@pytest.mark.parametrize("m,n,k,tb,mode", RELU_BWD)
def test_gemm_relu_bwd_is_the_masked_gemm_and_its_column_sums(m, n, k, tb, mode):
    """emloco_gemm_relu_bwd: C is BIT-equal to the plain GEMM of the same mode followed by the mask and the scale (the emulator's claim,
    tests/test_emu_kernels.py); the column sums are within fp32 summation error of a float64 sum of what was written"""
    lib = _lib()
    g = torch.Generator(device=DEV)
    g.manual_seed(m + n + k + tb)
    case = (m, n, k, tb, mode)
    A = torch.randn(m, k, generator=g, device=DEV)
    ldb = _ru4(n) if tb else k                     # (the launcher wants leading dimensions that are multiples of 4)
    Bst = torch.randn(*((k, ldb) if tb else (n, ldb)), generator=g, device=DEV) * 0.1
    B = Bst[:, :n] if tb else Bst
    hid16 = mode == "bf16mem"
    y = torch.relu(torch.randn(m, n, generator=g, device=DEV))
    y16 = y.to(torch.bfloat16)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))
    base = {"split": SPLIT, "split2": SPLIT2, "split_img": SPLIT, "fp32": 0, "bf16": BF16, "bf16mem": BF16}[mode]
    flags = base | (C16 | MASK16 if hid16 else 0)
    Bp, ldbp, tbp = Bst, ldb, tb
    if mode == "split_img":
        words = lib.emloco_gemm_split_image_words(n, k)
        Bp = torch.zeros(words, dtype=torch.int32, device=DEV)
        assert lib.emloco_gemm_split_pack(_ptr(Bst), n, k, ldb, tb, _ptr(Bp), _stream()) == 0
        flags |= IMG
        ldbp, tbp = 0, 0
    out = _Guarded(1, m, n, n, 0, 0, hid16)
    out.fill()
    ws = torch.empty(lib.emloco_gemm_relu_bwd_workspace(m, n) + TAIL, device=DEV)
    colsum = torch.full((n + TAIL,), SENT, device=DEV)
    rc = lib.emloco_gemm_relu_bwd(m, n, k, _ptr(A), k, _ptr(Bp), ldbp, tbp, out.ptr(), _ptr(y16 if hid16 else y), C.c_float(scale),
                                  _ptr(colsum), _ptr(ws), flags, _stream())
    assert rc == 0, case
    torch.cuda.synchronize()
    got, bits = out.got()
    assert (colsum[n:] == SENT).all(), ("column sums written past n", case)
    # the plain GEMM of the same mode (128 x 128 tile, the same stage depth rule), then mask and scale in fp32
    plain = _Guarded(1, m, n, n, 0, 0)
    plain.fill()
    with small_tile(0):
        rc = _gemm_launch(lib, 1, m, n, k, 1.0, A, 0, k, 0, 0, Bst, 0, ldb, 0, tb, plain, n, 0, None, base, 1)
    assert rc == 0
    torch.cuda.synchronize()
    p32 = plain.view()[0]
    mask = (y16.float() if hid16 else y) > 0
    want = torch.where(mask, p32 * scale, torch.zeros_like(p32))
    if hid16:
        assert torch.equal(bits[0], want.to(torch.bfloat16).view(torch.int16)), ("bf16 gradient is not the rounded masked product", case)
    else:
        assert torch.equal(bits[0], want), ("masked gradient differs from the masked plain GEMM", case)
    # ... which is the float64 product within its class
    ref = (A.double() @ (B.double() if tb else B.double().t())) * mask.double() * scale
    mag = (A.double().abs() @ (B.double().abs() if tb else B.double().abs().t())) * scale
    if mode.startswith("bf16"):
        Ar, Br = _bf16_round(A), _bf16_round(B)
        ref = (Ar @ (Br if tb else Br.t())) * mask.double() * scale
        bar = BAR_FP32 + (2.0 ** -8 if hid16 else 0.0)     # (a bf16 gradient in memory: bf16's unit roundoff on top)
    else:
        bar = BAR_SPLIT2 if mode == "split2" else BAR_FP32
    err = _rel_err(got[0], ref, mag)
    assert err <= bar, ("vs float64", case, err)
    written = got[0]
    cs = colsum[:n].double()
    want_cs = written.sum(0)
    assert ((cs - want_cs).abs() <= _colsum_bar(written)).all(), ("column sums", case, (cs - want_cs).abs().max().item())


@pytest.mark.parametrize("m,n", [(4 * 453 + 7, 129), (4 * 453 + 7, 384), (100003, 65), (100003, 132), (1, 1), (33, 3)])
@pytest.mark.parametrize("x16", [0, 1])
def test_colsum_ex_against_float64(m, n, x16):
    """emloco_colsum_ex, fp32 and bf16 input, the quad kernel (n % 4 == 0) and the scalar one"""
    lib = _lib()
    g = torch.Generator(device=DEV)
    g.manual_seed(m * 7 + n + x16)
    X = torch.randn(m, n, generator=g, device=DEV) + 0.5
    if x16:
        X = X.to(torch.bfloat16)
    out = torch.full((n + TAIL,), SENT, device=DEV)
    ws = torch.empty(lib.emloco_colsum_workspace(m, n) + TAIL, device=DEV)
    assert lib.emloco_colsum_ex(m, n, _ptr(X), _ptr(out), _ptr(ws), A16 if x16 else 0, _stream()) == 0
    torch.cuda.synchronize()
    x64 = X.double()
    assert (out[n:] == SENT).all(), ("column sums written past n", m, n, x16)
    err = (out[:n].double() - x64.sum(0)).abs()
    assert (err <= _colsum_bar(x64)).all(), (m, n, x16, err.max().item())


@pytest.mark.parametrize("m,n", [(4 * 453 + 7, 129), (100003, 64), (37, 1)])
@pytest.mark.parametrize("relu,p", [(1, 0.0), (1, 0.1), (0, 0.1), (0, 0.0)])
def test_act_bwd_colsum_against_float64(m, n, relu, p):
    """emloco_act_bwd_colsum: dz = dy [y > 0] / (1 - p) with ReLU (a positive output is active and kept), dy keep(seed) / (1 - p)
    without; column sums of dz within fp32 summation error"""
    lib = _lib()
    g = torch.Generator(device=DEV)
    g.manual_seed(m + n + relu + int(p * 10))
    dy = torch.randn(m, n, generator=g, device=DEV)
    y = torch.relu(torch.randn(m, n, generator=g, device=DEV))
    seed = 0xBEEF + m
    dz = _Guarded(1, m, n, n, 0, 0)
    dz.fill()
    colsum = torch.full((n + TAIL,), SENT, device=DEV)
    ws = torch.empty(lib.emloco_colsum_workspace(m, n) + TAIL, device=DEV)
    assert lib.emloco_act_bwd_colsum(m, n, _ptr(dy), _ptr(y), relu, float(p), seed, dz.ptr(), _ptr(colsum), _ptr(ws), _stream()) == 0
    torch.cuda.synchronize()
    got = dz.got()[0][0]
    s = 1.0 / (1.0 - p)
    if relu:
        mask = (y > 0).double()
    elif p > 0:
        h = np.zeros(m * n, np.uint8)
        assert lib.emloco_dropout_keep_mask(seed, 0, m * n, p, h.ctypes.data_as(C.c_void_p)) == 0
        mask = torch.from_numpy(h.reshape(m, n)).to(DEV).double()
    else:
        mask = torch.ones(m, n, dtype=torch.float64, device=DEV)
    ref = dy.double() * mask * s
    assert ((got - ref).abs() <= 2.0 ** -22 * ref.abs()).all(), ("dz", m, n, relu, p)
    assert (colsum[n:] == SENT).all()
    err = (colsum[:n].double() - got.sum(0)).abs()
    assert (err <= _colsum_bar(got)).all(), ("column sums", m, n, relu, p, err.max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. fused attention

ATTN_MODES = {"fp32": 0, "split": 64, "bf16": 16, "bf16mem": 16 | 32}
S_LIST = [1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 453]
SCALE = 1.0 / np.sqrt(32.0)


def _p8(p):
    return int(p * 256.0 + 0.5) / 256.0


def _key_bias(kind, n_seq, S, cut=None):
    if kind == "null":
        return None
    kb = torch.zeros(n_seq, S, device=DEV)
    if kind == "plus1":
        kb[0, 1::3] = 1.0
        kb[-1, :] = 1.0
    elif kind == "cut":
        kb[-1, cut:] = float("-inf")
        kb[0, ::5] = 1.0
    elif kind == "full":
        kb[-1, :] = float("-inf")
    return kb


def _attn_reference(qkv64, kb, H, nq, keep, p, dout64):
    n_seq, S, _ = qkv64.shape
    d = 32 * H
    q, k, v = (qkv64[..., i * d:(i + 1) * d].reshape(n_seq, S, H, 32).transpose(1, 2) for i in range(3))
    s = q[:, :, :nq] @ k.transpose(-1, -2) * SCALE
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx)
    lsum = e.sum(-1, keepdim=True)
    P = e / torch.where(lsum > 0, lsum, torch.ones_like(lsum))
    lse = (mx + torch.log(lsum))[..., 0]                       # -inf on a fully masked row
    M = keep / (1.0 - _p8(p)) if keep is not None else torch.ones_like(P)
    Pd = P * M
    oh = Pd @ v                                                # [n_seq][H][nq][32]
    out = oh.transpose(1, 2).reshape(n_seq, nq, d)
    do = dout64.reshape(n_seq, nq, H, 32).transpose(1, 2)
    D = (do * oh).sum(-1)
    dP = (do @ v.transpose(-1, -2)) * M
    dS = P * (dP - D[..., None])
    dq = dS @ k * SCALE
    dk = dS.transpose(-1, -2) @ q[:, :, :nq] * SCALE
    dv = Pd.transpose(-1, -2) @ do
    dqkv = torch.zeros(n_seq, S, 3 * d, dtype=torch.float64, device=DEV)
    back = lambda t: t.transpose(1, 2).reshape(n_seq, -1, d)
    dqkv[:, :nq, :d] = back(dq)
    dqkv[:, :, d:2 * d] = back(dk)
    dqkv[:, :, 2 * d:] = back(dv)
    return out, lse.reshape(n_seq * H, nq), dqkv, D.reshape(n_seq * H, nq)


def _attn_cases():
    kinds = ["null", "zeros", "plus1", "cut", "full"]
    out = []
    for mi, mode in enumerate(ATTN_MODES):
        for i, S in enumerate(S_LIST):
            H = (1, 4, 8)[(i + mi) % 3]
            kind = kinds[(i + 2 * mi) % len(kinds)]
            cut = None
            if kind == "cut":
                t = max(1, S // 64)
                cut = 32 * t + (-1, 0, 1)[(i + mi) % 3]
                if S < 2 or cut >= S:
                    kind, cut = "plus1", None
            p = (0.0, 0.1)[(i + mi) % 2]
            nq = (S, 21, 1)[(i // 2 + mi) % 3]
            out.append((mode, S, min(nq, S), H, kind, cut, p))
        # -inf cuts on both sides of a tile edge (32-key tiles, 128-query blocks), two query blocks
        for cut in (31, 32, 33, 255, 256, 257):
            out.append((mode, 453 if cut > 128 else 129, 453 if cut > 128 else 129, (4, 1, 8)[cut % 3], "cut", cut, 0.1 if cut % 2 else 0.0))
        out.append((mode, 257, 21, 8, "full", None, 0.1))
        out.append((mode, 2, 2, 1, "full", None, 0.0))
    return out


ATTN_CASES = _attn_cases()


def _attn_run(lib, mode, S, nq, H, kind, cut, p, n_seq=2):
    d = 32 * H
    flags = ATTN_MODES[mode]
    q16 = bool(flags & 32)
    g = torch.Generator(device=DEV)
    g.manual_seed(S * 131 + nq * 7 + H + int(p * 10) + len(kind))
    qkv = torch.randn(n_seq, S, 3 * d, generator=g, device=DEV) * 0.6
    if q16:
        qkv = qkv.to(torch.bfloat16)
    kb = _key_bias(kind, n_seq, S, cut)
    dout = torch.randn(n_seq, nq, d, generator=g, device=DEV)
    seed = 0x1234567 + S
    # guarded outputs: 64 elements of sentinel before each, TAIL after
    out = _Guarded(1, 1, n_seq * nq * d, 0, 0, 64)
    lse = _Guarded(1, 1, n_seq * H * nq, 0, 0, 64)
    dqkv = _Guarded(1, 1, n_seq * S * 3 * d, 0, 0, 64, bf16=q16)
    dsum = _Guarded(1, 1, n_seq * H * S, 0, 0, 64)
    for t in (out, lse, dqkv, dsum):
        t.fill()
    st = _stream()
    rc = lib.emloco_attention_fwd_queries(n_seq, S, nq, H, d, C.c_float(SCALE), _ptr(qkv), _ptr(kb), out.ptr(), lse.ptr(), flags,
                                          C.c_float(p), seed, st)
    assert rc == 0
    rc = lib.emloco_attention_bwd_queries(n_seq, S, nq, H, d, C.c_float(SCALE), _ptr(qkv), _ptr(kb), out.ptr(), lse.ptr(), _ptr(dout),
                                          dqkv.ptr(), dsum.ptr(), flags, C.c_float(p), seed, st)
    assert rc == 0
    torch.cuda.synchronize()
    keep = None
    if p > 0:
        h = np.zeros(n_seq * H * S * S, np.uint8)
        assert lib.emloco_attention_keep_mask(seed, n_seq * H, S, p, h.ctypes.data_as(C.c_void_p)) == 0
        keep = torch.from_numpy(h.reshape(n_seq, H, S, S)[:, :, :nq]).to(DEV).double()
    return qkv, kb, dout, keep, out, lse, dqkv, dsum


@pytest.mark.parametrize("mode,S,nq,H,kind,cut,p", ATTN_CASES, ids=[f"{c[0]}-S{c[1]}-q{c[2]}-h{c[3]}-{c[4]}{c[5] or ''}-p{c[6]}" for c in ATTN_CASES])
def test_fused_attention_matrix_against_float64(mode, S, nq, H, kind, cut, p):
    """forward (out, lse) and backward (dq, dk, dv, dsum) against float64 softmax attention with the same key bias and dropout mask.
    fp32 / split: 2e-5 of the tensor's scale (outputs) and 2e-4 (gradients), as the model-level tests; bf16 modes: against float64 on
    the bf16-rounded q|k|v, the emulator's bf16 class (out 2e-2, lse 2e-3, dq / dk / dv 3e-2)"""
    lib = _lib()
    n_seq = 2
    d = 32 * H
    case = (mode, n_seq, S, nq, H, kind, cut, p)
    qkv, kb, dout, keep, out, lse, dqkv, dsum = _attn_run(lib, mode, S, nq, H, kind, cut, p, n_seq)
    bf = mode.startswith("bf16")
    q64 = _bf16_round(qkv) if bf else qkv.double()
    r_out, r_lse, r_dqkv, r_D = _attn_reference(q64, kb, H, nq, keep, p, dout.double())
    g_out = out.got()[0].reshape(n_seq, nq, d)
    g_lse = lse.got()[0].reshape(n_seq * H, nq)
    g_dqkv = dqkv.got()[0].reshape(n_seq, S, 3 * d)
    g_D = dsum.got()[0].reshape(-1)[:n_seq * H * nq].reshape(n_seq * H, nq)
    bars = {"out": 2e-2, "lse": 2e-3, "dsum": 2e-2, "grad": 3e-2} if bf else {"out": 2e-5, "lse": 2e-5, "dsum": 2e-5, "grad": 2e-4}

    def close(got, want, rel, what, sc=None):
        assert torch.isfinite(got).all(), (what, "non-finite", case)
        err = (got - want).abs().max().item()
        sc = want.abs().max().item() if sc is None else sc
        assert err <= rel * sc + 1e-6, (what, case, err, sc)
    close(g_out, r_out, bars["out"], "out")
    live = torch.isfinite(r_lse)
    if live.any():
        close(g_lse[live], r_lse[live], bars["lse"], "lse")
    assert (g_lse[~live] > 1e38).all(), ("lse of a fully masked row", case)
    close(g_D, r_D, bars["dsum"], "dsum")
    # (the gradient's scale is the whole dqkv's, as in the model-level tests: dq alone can vanish -- S = 1 has a zero dq)
    for i, what in enumerate(("dq", "dk", "dv")):
        close(g_dqkv[..., i * d:(i + 1) * d], r_dqkv[..., i * d:(i + 1) * d], bars["grad"], what, sc=r_dqkv.abs().max().item())
    assert (g_dqkv[:, nq:, :d] == 0).all(), ("dQ of rows that did not attend", case)
    if kind in ("cut", "full"):
        c = 0 if kind == "full" else cut
        assert (g_dqkv[-1, c:, d:] == 0).all(), ("masked keys receive no gradient", case)
        if kind == "full":
            assert (g_out[-1] == 0).all(), ("a fully masked sequence gives zeros", case)

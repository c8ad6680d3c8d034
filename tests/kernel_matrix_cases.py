"""The cases of the device conformance matrix of the GEMM family and the fused attention kernels (tests/test_gpu_kernel_matrix.py):
case tables, strided operands and guarded outputs, float64 references and the per-case checks.  tests/test_gpu_kernel_knobs.py runs the
same cases in child processes whose environment selects a kernel variant that the library reads once when it loads:

    python -m tests.kernel_matrix_cases [--expect NAME=VALUE ...] [--dump FILE] GROUP [GROUP ...]

runs the groups in this process and prints one JSON line per case -- {"id", "group", "ok", "ratios": worst error / bar per checked
tensor, "error"} -- then one summary line {"cases", "failed"}; the exit status is non-zero if a case failed.  --expect asserts what
emloco_kernel_variants reports (attn_bwd_pieces, attn16_old, wide_stores, gemm_bk) before any case runs; --dump writes the raw output
bits of the fp32 / split / split2 cases to an .npz (the parent of the EMLOCO_GEMM_WIDE_STORES=0 child compares them with its own).

PER-ELEMENT BARS OF THE ATTENTION (fp32 and split modes; `attn_mags`).  A GEMM element is judged against mag = |A| @ |B|^T, the error
scale of a dot product; the attention is a chain of such products, and every tensor is judged by |got - ref| <= eps * mag with mag the
first-order magnitude of its chain, in float64, from the inputs and the float64 reference alone.  Per (sequence, head), c = scale,
s = c q k^T + bias, P = softmax(s), M = keep / (1 - p8) (ones without dropout), Pd = P o M, O = Pd v, D = rowsum(dO o O),
dP = (dO v^T) o M, dS = P o (dP - D), dq = c dS k, dk = c dS^T q, dv = Pd^T dO.  A computed product sum_j a_j b_j carries
eps * sum_j |a_j| |b_j|; an error e_a in a computed operand adds sum_j e_a_j |b_j|.  So, in units of eps:

    ms   = c |q| |k|^T + |bias|  (finite entries)   the logits
    ml_i = sum_j P_ij ms_ij                          the log-sum-exp: d lse_i = sum_j P_ij d s_ij
    rP   = 1 + ms_ij + ml_i                          RELATIVE error of P_ij = exp(s_ij - lse_i): the logit's, the log-sum-exp's, and 1 for
                                                     the exponential, the rounding of lse and of s - lse (some tens of 2^-24, below eps)
    out  : Pd @ |v|  +  (Pd o rP) @ |v|              the product + the logits' error carried through P
    dsum : sum_d |dO| (|O| + mag_out)                the row dot product + the forward output's own error
    mdP  = (|dO| |v|^T) o M
    mdS  = P o (mdP + mag_dsum + rP o |dP - D|)      absolute error of dS: of dP, of D, and P's relative error on the difference
    dq   : c (|dS| @ |k|  +  mdS @ |k|)
    dk   : c (|dS|^T @ |q|  +  mdS^T @ |q|)
    dv   : Pd^T @ |dO|  +  (Pd o rP)^T @ |dO|

eps is BAR_FP32 for the forward (always three pieces or the fp32 instruction), for dsum (a plain fp32 row sum in every mode: the two- and
three-piece launches give the same bits), and for the backward in the fp32 mode and with three pieces; BAR_SPLIT2 for dq / dk / dv of the
two-piece backward.  An element whose mag is zero (rows that did not attend, masked keys, a fully masked sequence) must be exactly zero.
tests/test_emu_kernels.py holds the emulated kernels to these bars on every row of the matrix, on the CPU.
"""
import ctypes as C
import json
import sys

import numpy as np
import torch

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

VARIANT_NAMES = ("attn_bwd_pieces", "attn16_old", "wide_stores", "gemm_bk")      # the order of emloco_kernel_variants


def _lib():
    from emloco_amd.predictor import ops
    return ops._lib()


def variants(lib):
    """{name: value} of what the loaded library parsed from its variant knobs (emloco_kernel_variants)"""
    v = (C.c_int32 * 4)()
    rc = lib.emloco_kernel_variants(v)
    assert rc == 0, ("emloco_kernel_variants", rc, lib.emloco_last_error().decode())
    return dict(zip(VARIANT_NAMES, (int(x) for x in v)))


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


def _check_gemm(lib, case, ratios=None, sink=None):
    """the case against float64 at the bar of its precision class.  ratios (a dict): takes the worst error / bar; sink (a dict): takes
    the raw output bits (numpy) of a case in the fp32, split or split2 mode under the key "bits"."""
    ratios = {} if ratios is None else ratios
    case.make()
    if case.mem & C16:
        # the bf16 output is the RNE rounding of the fp32 result of the same launch (same kernel, fp32 C) ...
        bits = case.run(lib).got()[1]
        got = case.run(lib, flags=case.flags() & ~C16).got()[0]
        want = got.float().to(torch.bfloat16).view(torch.int16)
        assert torch.equal(bits, want), ("bf16 output is not the RNE rounding of the fp32 result", case)
    else:
        got, bits = case.run(lib).got()
        if sink is not None and case.mode != "bf16":
            sink["bits"] = bits.cpu().numpy().view(np.uint32)
    eff = case.effective()
    if eff == "bf16":                   # ... which is checked like any other
        ref, mag = case.reference(lib, rounded=True)
        err = _rel_err(got, ref, mag)
        ratios["bf16_rounded"] = err / BAR_FP32
        assert err <= BAR_FP32, ("bf16 mode vs float64 on the rounded operands", case, err)
        if (case.mem & (A16 | B16)) != (A16 | B16):            # (two bf16 operands in memory: nothing left to round)
            ref_full, mag_full = case.reference(lib, rounded=False)
            full = _rel_err(got, ref_full, mag_full)
            assert full > 1e-4, ("bf16 mode is not visibly reduced precision", case, full)
        return
    ref, mag = case.reference(lib, rounded=False)
    err = _rel_err(got, ref, mag)
    if eff == "split2":
        ratios["split2"] = err / BAR_SPLIT2
        assert err <= BAR_SPLIT2, ("split2 vs float64", case, err)
        three = case.run(lib, flags=case.flags() & ~4096)
        err3 = _rel_err(three.got()[0], ref, mag)
        ratios["split"] = err3 / BAR_FP32
        assert err3 <= BAR_FP32 and err > err3, ("split2 must be coarser than the three-piece product", case, err, err3)
    else:
        ratios[eff] = err / BAR_FP32
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


def _bk_cases():
    """EMLOCO_GEMM_BK: the (trans_a, trans_b) = (1, 1) layout, which the launcher never serves 32 deep by itself -- n > 32, the fp32 mode
    on 16-byte loads and (unaligned bases) on scalar loads, the bf16 mode with fp32 operands and with A, B, or both in memory as bf16;
    k around the 32-deep stage (a ragged last stage, a single partial one), alone and split in three; bias / accumulate epilogues"""
    out = []
    variants_ = [("fp32", 0, {}), ("fp32", 0, dict(a_off=1, b_off=1, c_off=1, ld_pad=3)), ("bf16", 0, {}), ("bf16", A16, {}), ("bf16", B16, {}),
                 ("bf16", A16 | B16, {})]
    epis = (0, BIAS, ACC, BIAS | ACC)
    for mi, (m, n) in enumerate(((129, 130), (64, 33))):
        for ki, k in enumerate((1, 31, 32, 33, 95, 300)):
            for si, ks in enumerate((1, 3)):
                for vi, (mode, mem, kw) in enumerate(variants_):
                    kw = dict({"ld_pad": -1}, **kw)
                    out.append(GemmCase(1, m, n, k, 1, 1, mode, mem=mem, ksplit=ks, epi=epis[(mi + ki + si + vi) % 4], seed=ki, **kw))
    return out


def _default_deep_cases():
    """the matrix's cases that the launcher serves 32 deep by itself (k / ksplit > 256 outside the split modes; n <= 32, or a layout other
    than (1, 1) on at most 1024 workgroups): a forced depth must leave them inside their bars"""
    return [c for c in _ragged_cases() + _alignment_cases()
            if c.k // c.ksplit > 256 and c.mode in ("fp32", "bf16") and (c.n <= 32 or not (c.ta and c.tb))]


GEMM_GROUPS = {"ragged": _ragged_cases, "alignment": _alignment_cases, "batch": _batch_cases, "epilogue": _epilogue_cases,
               "threshold": _threshold_cases, "mem": _mem_cases, "bk": _bk_cases, "default_deep": _default_deep_cases}


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the fused backward epilogue

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
RELU_BWD_SMALL = [c for c in RELU_BWD if c[0] < 10000]


def check_relu_bwd(lib, m, n, k, tb, mode, ratios=None, sink=None):
    """emloco_gemm_relu_bwd: C is BIT-equal to the plain GEMM of the same mode followed by the mask and the scale; the column sums are
    within fp32 summation error of a float64 sum of what was written (sink: as _check_gemm, for the modes with an fp32 gradient)"""
    ratios = {} if ratios is None else ratios
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
    if sink is not None and mode in ("split", "split2", "fp32", "split_img"):
        sink["bits"] = bits.cpu().numpy().view(np.uint32)
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
    ratios[mode] = err / bar
    assert err <= bar, ("vs float64", case, err)
    written = got[0]
    cs = colsum[:n].double()
    want_cs = written.sum(0)
    ratios["colsum"] = ((cs - want_cs).abs() / _colsum_bar(written)).max().item()
    assert ((cs - want_cs).abs() <= _colsum_bar(written)).all(), ("column sums", case, (cs - want_cs).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. fused attention

ATTN_MODES = {"fp32": 0, "split": 64, "bf16": 16, "bf16mem": 16 | 32}
S_LIST = [1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 453]
SCALE = 1.0 / np.sqrt(32.0)


def _p8(p):
    return int(p * 256.0 + 0.5) / 256.0


def _key_bias(kind, n_seq, S, cut=None, dev=None):
    if kind in ("null", "coherent"):
        return None
    kb = torch.zeros(n_seq, S, device=DEV if dev is None else dev)
    if kind == "plus1":
        kb[0, 1::3] = 1.0
        kb[-1, :] = 1.0
    elif kind == "cut":
        kb[-1, cut:] = float("-inf")
        kb[0, ::5] = 1.0
    elif kind == "full":
        kb[-1, :] = float("-inf")
    return kb


def _attn_heads(qkv64, H, nq, dout64):
    n_seq, S, _ = qkv64.shape
    d = 32 * H
    q, k, v = (qkv64[..., i * d:(i + 1) * d].reshape(n_seq, S, H, 32).transpose(1, 2) for i in range(3))
    return q[:, :, :nq], k, v, dout64.reshape(n_seq, nq, H, 32).transpose(1, 2)


def _attn_softmax(q, k, kb):
    s = q @ k.transpose(-1, -2) * SCALE
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx)
    lsum = e.sum(-1, keepdim=True)
    P = e / torch.where(lsum > 0, lsum, torch.ones_like(lsum))
    return P, (mx + torch.log(lsum))[..., 0]                   # (-inf on a fully masked row)


def _attn_reference(qkv64, kb, H, nq, keep, p, dout64):
    n_seq, S, _ = qkv64.shape
    d = 32 * H
    q, k, v, do = _attn_heads(qkv64, H, nq, dout64)
    P, lse = _attn_softmax(q, k, kb)
    M = keep / (1.0 - _p8(p)) if keep is not None else torch.ones_like(P)
    Pd = P * M
    oh = Pd @ v                                                # [n_seq][H][nq][32]
    out = oh.transpose(1, 2).reshape(n_seq, nq, d)
    D = (do * oh).sum(-1)
    dP = (do @ v.transpose(-1, -2)) * M
    dS = P * (dP - D[..., None])
    dq = dS @ k * SCALE
    dk = dS.transpose(-1, -2) @ q * SCALE
    dv = Pd.transpose(-1, -2) @ do
    dqkv = torch.zeros(n_seq, S, 3 * d, dtype=torch.float64, device=qkv64.device)
    back = lambda t: t.transpose(1, 2).reshape(n_seq, -1, d)
    dqkv[:, :nq, :d] = back(dq)
    dqkv[:, :, d:2 * d] = back(dk)
    dqkv[:, :, 2 * d:] = back(dv)
    return out, lse.reshape(n_seq * H, nq), dqkv, D.reshape(n_seq * H, nq)


def attn_mags(qkv64, kb, H, nq, keep, p, dout64):
    """first-order error magnitudes of out [n_seq][nq][d], dsum [n_seq * H][nq] and dqkv [n_seq][S][3 d], laid out as the reference's
    tensors (the module docstring derives every term); float64, from the inputs and the float64 reference only"""
    n_seq, S, _ = qkv64.shape
    d = 32 * H
    q, k, v, do = _attn_heads(qkv64, H, nq, dout64)
    P, _ = _attn_softmax(q, k, kb)
    M = keep / (1.0 - _p8(p)) if keep is not None else torch.ones_like(P)
    Pd = P * M
    ms = q.abs() @ k.abs().transpose(-1, -2) * SCALE
    if kb is not None:
        kb64 = kb.double()
        ms = ms + torch.where(torch.isfinite(kb64), kb64.abs(), torch.zeros_like(kb64))[:, None, None, :]
    ml = (P * ms).sum(-1, keepdim=True)
    rP = 1.0 + ms + ml
    PdE = Pd * (1.0 + rP)                                      # the product's own term and the logits' error carried through P
    oh = Pd @ v
    m_oh = PdE @ v.abs()
    m_out = m_oh.transpose(1, 2).reshape(n_seq, nq, d)
    m_D = (do.abs() * (oh.abs() + m_oh)).sum(-1)
    D = (do * oh).sum(-1)
    dP = (do @ v.transpose(-1, -2)) * M
    diff = dP - D[..., None]
    dS = P * diff
    m_dS = P * ((do.abs() @ v.abs().transpose(-1, -2)) * M + m_D[..., None] + rP * diff.abs())
    e_dS = dS.abs() + m_dS
    m_dq = e_dS @ k.abs() * SCALE
    m_dk = e_dS.transpose(-1, -2) @ q.abs() * SCALE
    m_dv = PdE.transpose(-1, -2) @ do.abs()
    m_dqkv = torch.zeros(n_seq, S, 3 * d, dtype=torch.float64, device=qkv64.device)
    back = lambda t: t.transpose(1, 2).reshape(n_seq, -1, d)
    m_dqkv[:, :nq, :d] = back(m_dq)
    m_dqkv[:, :, d:2 * d] = back(m_dk)
    m_dqkv[:, :, 2 * d:] = back(m_dv)
    return m_out, m_D.reshape(n_seq * H, nq), m_dqkv


def attn_bar_ratios(got, ref, mag, d, eps_bwd):
    """worst |got - ref| / (eps mag) of out, dsum, dq, dk, dv -- got / ref / mag: (out, dsum, dqkv) float64 tensors; eps is BAR_FP32 for
    out and dsum, eps_bwd for the three gradients; an element with mag = 0 counts 0 when it is exact and inf when it is not"""
    def worst(g, r, m, eps):
        err = (g - r).abs()
        if not torch.isfinite(g).all():
            return float("inf")
        ratio = torch.where(m > 0, err / (eps * m).clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        return ratio.max().item() if ratio.numel() else 0.0
    out = {"out": worst(got[0], ref[0], mag[0], BAR_FP32), "dsum": worst(got[1], ref[1], mag[1], BAR_FP32)}
    for i, what in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        out[what] = worst(got[2][..., sl], ref[2][..., sl], mag[2][..., sl], eps_bwd)
    return out


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
# The case that tells two pieces from three (random operands average the dropped third pieces away): every operand positive, every low
# mantissa bit chosen so that the remainder after two bf16 pieces has one sign and nearly its largest size -- `coherent_values`.
ATTN_COHERENT = ("split", 129, 129, 4, "coherent", None, 0.0)


def attn_id(c):
    return f"{c[0]}-S{c[1]}-q{c[2]}-h{c[3]}-{c[4]}{c[5] or ''}-p{c[6]}"


def coherent_values(gen, shape, exponent, dev):
    """positive fp32 values 2^exponent (1 + f), f < 2^-7, whose mantissa is [0000000][01xxxxxx][00111111]: the first bf16 piece rounds
    down to 2^exponent, the second (8 significant bits from bit 14 of the 16 that remain) rounds down as well, and the remainder that a
    two-piece operand drops is +63 units of 2^-23 of the value (2^-17 would be 64) for EVERY element -- in a sum of products of such
    operands the dropped pieces add up instead of averaging out"""
    mid = torch.randint(0x40, 0x80, shape, generator=gen, device=dev, dtype=torch.int32)
    bits = ((127 + exponent) << 23) | (mid << 8) | 0x3F
    return bits.to(torch.int32).view(torch.float32)


def attn_inputs(case, n_seq=2, dev=None):
    """(qkv, key bias or None, dout, dropout seed) of a case, on `dev`"""
    mode, S, nq, H, kind, cut, p = case
    dev = DEV if dev is None else dev
    d = 32 * H
    g = torch.Generator(device=dev)
    g.manual_seed(S * 131 + nq * 7 + H + int(p * 10) + len(kind))
    if kind == "coherent":
        # q = 1, v = dO = 1, keys 2^-6 except one heavy key per sequence at 2^-1: its logits are ~2.8 above the others', so the logits'
        # two-piece error (both operands' dropped pieces) reaches its dv row undiluted by the log-sum-exp
        qkv = coherent_values(g, (n_seq, S, 3 * d), 0, dev)
        qkv[..., d:2 * d] = coherent_values(g, (n_seq, S, d), -6, dev)
        qkv[:, 77, d:2 * d] = coherent_values(g, (n_seq, d), -1, dev)
        dout = coherent_values(g, (n_seq, nq, d), 0, dev)
    else:
        qkv = torch.randn(n_seq, S, 3 * d, generator=g, device=dev) * 0.6
        if ATTN_MODES[mode] & 32:
            qkv = qkv.to(torch.bfloat16)
        dout = torch.randn(n_seq, nq, d, generator=g, device=dev)
    return qkv, _key_bias(kind, n_seq, S, cut, dev), dout, 0x1234567 + S


def _attn_run(lib, mode, S, nq, H, kind, cut, p, n_seq=2):
    d = 32 * H
    flags = ATTN_MODES[mode]
    q16 = bool(flags & 32)
    qkv, kb, dout, seed = attn_inputs((mode, S, nq, H, kind, cut, p), n_seq)
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


def attn_eps_bwd(lib, mode):
    """the bar of dq / dk / dv in the fp32 and split modes: BAR_SPLIT2 where the loaded library launches the two-piece backward (split
    mode, round 5's kernels, EMLOCO_ATTN_BWD_PIECES unset or 2), BAR_FP32 everywhere else"""
    v = variants(lib)
    return BAR_SPLIT2 if mode == "split" and not v["attn16_old"] and v["attn_bwd_pieces"] == 2 else BAR_FP32


def check_attention(lib, mode, S, nq, H, kind, cut, p, ratios=None, eps_bwd=None):
    """forward (out, lse) and backward (dq, dk, dv, dsum) against float64 softmax attention with the same key bias and dropout mask.
    fp32 / split: 2e-5 of the tensor's scale (outputs) and 2e-4 (gradients), as the model-level tests, and the per-element bars of the
    module docstring; bf16 modes: against float64 on the bf16-rounded q|k|v, the emulator's bf16 class (out 2e-2, lse 2e-3,
    dq / dk / dv 3e-2)"""
    ratios = {} if ratios is None else ratios
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
        ratios["scale_" + what] = err / (rel * sc + 1e-6)
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
    if not bf:                                                 # every element against its own chain's magnitude
        eps_bwd = attn_eps_bwd(lib, mode) if eps_bwd is None else eps_bwd
        mags = attn_mags(q64, kb, H, nq, keep, p, dout.double())
        el = attn_bar_ratios((g_out, g_D, g_dqkv), (r_out, r_D, r_dqkv), mags, d, eps_bwd)
        ratios.update(el)
        bad = {k: v for k, v in el.items() if not v <= 1.0}
        assert not bad, ("per-element bars (error / (eps mag))", case, "eps_bwd", eps_bwd, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the groups by name, for a run in a process of its own

def group_cases(name):
    """[(id, callable(lib, ratios, sink))] of a group"""
    if name in GEMM_GROUPS:
        return [(f"{name}[{i}]:{c!r}", (lambda lib, r, s, c=c: _check_gemm(lib, c, r, s))) for i, c in enumerate(GEMM_GROUPS[name]())]
    if name == "relu_bwd_small":
        return [("relu_bwd:" + "-".join(map(str, c)), (lambda lib, r, s, c=c: check_relu_bwd(lib, *c, ratios=r, sink=s))) for c in RELU_BWD_SMALL]
    if name in ("attn_split", "attn_bf16mem"):
        return [("attn:" + attn_id(c), (lambda lib, r, s, c=c: check_attention(lib, *c, ratios=r))) for c in ATTN_CASES if c[0] == name[5:]]
    if name == "attn_coherent":
        return [("attn:" + attn_id(ATTN_COHERENT), (lambda lib, r, s: check_attention(lib, *ATTN_COHERENT, ratios=r)))]
    raise SystemExit(f"unknown group {name!r}")


GROUPS = tuple(GEMM_GROUPS) + ("relu_bwd_small", "attn_split", "attn_bf16mem", "attn_coherent")


def run_groups(lib, names, emit=None, sinks=None):
    """every case of the groups, in order; emit(record) per case; sinks (a dict): id -> raw output bits.  Returns (cases, failed ids)."""
    n, failed = 0, []
    for name in names:
        for cid, fn in group_cases(name):
            ratios, sink = {}, ({} if sinks is not None else None)
            rec = {"id": cid, "group": name, "ok": True}
            try:
                fn(lib, ratios, sink)
            except AssertionError as e:
                rec["ok"], rec["error"] = False, str(e)[:2000]
                failed.append(cid)
            rec["ratios"] = {k: (round(v, 4) if np.isfinite(v) else str(v)) for k, v in ratios.items()}
            if sink:
                sinks[cid] = sink["bits"]
            n += 1
            if emit is not None:
                emit(rec)
    return n, failed


def main(argv):
    expect, dump, names = {}, None, []
    it = iter(argv)
    for a in it:
        if a == "--expect":
            k, v = next(it).split("=")
            expect[k] = int(v)
        elif a == "--dump":
            dump = next(it)
        else:
            names.append(a)
    for n in names:
        if n not in GROUPS:
            raise SystemExit(f"unknown group {n!r}: one of {GROUPS}")
    lib = _lib()
    got = variants(lib)
    emit = lambda rec: print(json.dumps(rec), flush=True)
    emit({"variants": got})
    for k, v in expect.items():
        if got[k] != v:
            raise SystemExit(f"the library reports {k} = {got[k]}, expected {v}: the variant under test is not the selected one")
    sinks = {} if dump else None
    n, failed = run_groups(lib, names, emit, sinks)
    if dump:
        np.savez(dump, **{f"c{i}": b for i, b in enumerate(sinks.values())}, ids=np.array(list(sinks), dtype=np.str_))
    emit({"cases": n, "failed": failed})
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

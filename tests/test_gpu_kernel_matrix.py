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

The attention's out / dsum / dq / dk / dv are also measured per element against the first-order magnitude of their product chain
(tests/kernel_matrix_cases.py derives it), as the GEMM is against mag.

The cases, operand builders, references and per-case checks live in tests/kernel_matrix_cases.py.  The kernel variants that environment
knobs select when the library loads (EMLOCO_ATTN_BWD_PIECES=3, EMLOCO_ATTN16_OLD=1, EMLOCO_GEMM_BK=16 / 32, EMLOCO_GEMM_WIDE_STORES=0)
run the same cases in child processes: tests/test_gpu_kernel_knobs.py.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (GARBAGE, _Guarded and the other builders are also what the task / reset / chain / elementwise matrices import from here)
from kernel_matrix_cases import (A16, ACC, ATTN_CASES, B16, BAR_FP32, BAR_SPLIT2, BIAS, C16, DEV, GARBAGE, GEMM_GROUPS, IMG, LAYOUTS,  # noqa: E402,F401
                                 RELU, RELU_BWD, SENT, TAIL, GemmCase, _bits, _check_gemm, _colsum_bar, _gemm_launch, _Guarded, _lib, _ptr,
                                 _rel_err, _stream, attn_id, check_attention, check_relu_bwd, small_tile)

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. GEMM matrix

@pytest.mark.parametrize("group", ["ragged", "alignment", "batch", "epilogue", "threshold", "mem"])
def test_gemm_matrix_against_float64(group):
    """every case of the group: float64 bar of its precision class, guard bands intact, every output element written"""
    lib = _lib()
    cases = GEMM_GROUPS[group]()
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

@pytest.mark.parametrize("m,n,k,tb,mode", RELU_BWD)
def test_gemm_relu_bwd_is_the_masked_gemm_and_its_column_sums(m, n, k, tb, mode):
    """emloco_gemm_relu_bwd: C is BIT-equal to the plain GEMM of the same mode followed by the mask and the scale (the emulator's claim,
    tests/test_emu_kernels.py); the column sums are within fp32 summation error of a float64 sum of what was written"""
    check_relu_bwd(_lib(), m, n, k, tb, mode)


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

@pytest.mark.parametrize("mode,S,nq,H,kind,cut,p", ATTN_CASES, ids=[attn_id(c) for c in ATTN_CASES])
def test_fused_attention_matrix_against_float64(mode, S, nq, H, kind, cut, p):
    """forward (out, lse) and backward (dq, dk, dv, dsum) against float64 softmax attention with the same key bias and dropout mask.
    fp32 / split: 2e-5 of the tensor's scale (outputs) and 2e-4 (gradients), as the model-level tests, and every element of out, dsum,
    dq, dk and dv within eps of its product chain's magnitude (BAR_FP32; BAR_SPLIT2 for the gradients of the two-piece backward);
    bf16 modes: against float64 on the bf16-rounded q|k|v, the emulator's bf16 class (out 2e-2, lse 2e-3, dq / dk / dv 3e-2)"""
    check_attention(_lib(), mode, S, nq, H, kind, cut, p)

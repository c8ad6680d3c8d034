"""The kernel variants behind load-time knobs, on the device.  The library reads EMLOCO_ATTN_BWD_PIECES, EMLOCO_ATTN16_OLD, EMLOCO_GEMM_BK
and EMLOCO_GEMM_WIDE_STORES once, so a variant can only be reached by a process that starts with the variable set: every test here
starts ONE fresh child, `python -m tests.kernel_matrix_cases GROUP ...`, with os.environ plus that one variable.  The child first
asserts through emloco_kernel_variants that the library selected the variant, then runs the cases of the device matrix that the knob
affects (tests/kernel_matrix_cases.py: the same operands, guard bands, references and bars as tests/test_gpu_kernel_matrix.py) and
prints one JSON line per case; the parent fails with the knob and the ids of the failing cases, or if fewer cases ran than it expects.

Children run one at a time, each under its own timeout, none is started twice.  A child that ends by a signal or a timeout (status
134, 139, 124, 137 or their negative forms) or reports an illegal memory access is recorded in `_DEVICE_TROUBLE`: every later test of
this file then fails at once, with that text, and starts no process.

What each child launches (attention_capi.hip / predictor_capi.hip):
- EMLOCO_ATTN_BWD_PIECES=3: attn16_bwd_dq_kernel<3, 1, DROP, 0> and attn16_bwd_dkv_kernel<3, 1, DROP, 0> (DROP = 0, 1) behind
  attn16_fwd_kernel<3, 2, DROP, 0>.
- EMLOCO_ATTN16_OLD=1: attn_fwd_kernel, attn_bwd_dq_kernel and attn_bwd_dkv_kernel in <2, DROP> (split) and <1, DROP, 1> (bf16
  q|k|v in memory), with the launcher's zeroing of dQ where n_query < S.
- EMLOCO_GEMM_BK=32 / 16: the (trans_a, trans_b) = (1, 1) layout of gemm_pick at the forced depth -- fp32 on 16-byte and on scalar
  loads, bf16, and bf16 with A, B or both in memory as bf16; the launcher only ever picks the 16-deep ones of this layout by itself.
- EMLOCO_GEMM_WIDE_STORES=0: the per-register epilogue stores of emloco_gemm_f32_ex and emloco_gemm_relu_bwd on aligned outputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import kernel_matrix_cases as kmc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEVICE_TROUBLE = []                    # the first child that died or faulted: [text]
CRASH_STATUS = {134: "abort", 139: "segmentation fault", 124: "time limit", 137: "killed", -6: "abort", -11: "segmentation fault", -9: "killed"}


def _child(knob, value, expect, groups, timeout, dump=None):
    """one child with os.environ + {knob: value}: the parsed JSON records of its cases, after every check the parent makes on the run"""
    if _DEVICE_TROUBLE:
        pytest.fail("not started: an earlier child of this file " + _DEVICE_TROUBLE[0])
    cmd = [sys.executable, "-m", "tests.kernel_matrix_cases"]
    for k, v in expect.items():
        cmd += ["--expect", f"{k}={v}"]
    if dump is not None:
        cmd += ["--dump", str(dump)]
    want = sum(len(kmc.group_cases(g)) for g in groups)
    try:
        run = subprocess.run(cmd + list(groups), cwd=ROOT, env=dict(os.environ, **{knob: value}), capture_output=True, text=True, timeout=timeout)
        status, text = run.returncode, run.stdout + run.stderr
    except subprocess.TimeoutExpired as e:
        status = 124
        text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
    if status in CRASH_STATUS or "illegal memory access" in text:
        why = CRASH_STATUS.get(status, "illegal memory access")
        _DEVICE_TROUBLE.append(f"({knob}={value}) ended with status {status} ({why})")
        pytest.fail(f"{knob}={value}: the child ended with status {status} ({why}); output tail:\n{text[-3000:]}")
    recs = []
    for ln in text.splitlines():
        if ln.startswith("{"):
            try:
                recs.append(json.loads(ln))
            except ValueError:
                pass
    cases = [r for r in recs if "id" in r]
    summary = [r for r in recs if "cases" in r]
    reported = [r["variants"] for r in recs if "variants" in r]
    failed = [r["id"] for r in cases if not r["ok"]]
    assert not failed, f"{knob}={value}: {len(failed)} of {len(cases)} cases failed: {failed}\n" + "\n".join(
        r.get("error", "") for r in cases if not r["ok"])[:6000]
    assert status == 0 and summary, f"{knob}={value}: the child ended with status {status} before its summary; output tail:\n{text[-3000:]}"
    assert reported and all(reported[0][k] == v for k, v in expect.items()), (knob, value, "the child did not report the variant", reported)
    assert len(cases) == summary[0]["cases"] == want, f"{knob}={value}: {len(cases)} cases ran, {want} expected"
    return cases


def test_attention_three_piece_backward():
    """EMLOCO_ATTN_BWD_PIECES=3: every split row of the matrix at the three-piece bars (BAR_FP32 per element on dq / dk / dv), and the
    constructed case on which the two-piece backward exceeds those bars 7 x (tests/test_emu_kernels.py) -- with the export, the proof
    that the three-piece kernels ran"""
    _child("EMLOCO_ATTN_BWD_PIECES", "3", {"attn_bwd_pieces": 3, "attn16_old": 0}, ("attn_split", "attn_coherent"), timeout=240)


def test_attention_round4_kernels():
    """EMLOCO_ATTN16_OLD=1: every split and bf16-memory row -- the rows with n_query < S (the launcher's zeroing of dQ, 2-byte and 4-byte
    elements) and the fully masked ones included"""
    _child("EMLOCO_ATTN16_OLD", "1", {"attn16_old": 1}, ("attn_split", "attn_bf16mem"), timeout=240)


@pytest.mark.parametrize("depth", ["32", "16"])
def test_gemm_forced_stage_depth(depth):
    """EMLOCO_GEMM_BK: the (1, 1) layout at the forced depth (the only way to its 32-deep kernels), k on both sides of a stage, split k,
    every memory dtype -- and the matrix's own 32-deep cases, which a forced depth must leave inside their bars"""
    _child("EMLOCO_GEMM_BK", depth, {"gemm_bk": int(depth)}, ("bk", "default_deep"), timeout=240)


def test_gemm_per_register_stores():
    """EMLOCO_GEMM_WIDE_STORES=0: the same bars as the wide-store run, and for the fp32, split and split2 modes the SAME BITS as this
    process (wide stores) computes: the store path does not touch the arithmetic"""
    groups = ("ragged", "alignment", "batch", "epilogue", "mem", "relu_bwd_small")
    lib = kmc._lib()
    assert kmc.variants(lib)["wide_stores"] == 1, "the parent must run with wide stores (EMLOCO_GEMM_WIDE_STORES unset or 1)"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "per_register.npz")
        _child("EMLOCO_GEMM_WIDE_STORES", "0", {"wide_stores": 0}, groups, timeout=420, dump=dump)
        with np.load(dump) as z:
            theirs = {str(i): z[f"c{n}"] for n, i in enumerate(z["ids"])}
    mine = {}
    n, failed = kmc.run_groups(lib, groups, sinks=mine)
    assert not failed, ("the wide-store run of the same cases failed in the parent", failed)
    want = sum(c.mode != "bf16" for g in groups[:-1] for c in kmc.GEMM_GROUPS[g]()) + sum(c[4] in ("fp32", "split", "split2", "split_img") for c in kmc.RELU_BWD_SMALL)
    assert set(mine) == set(theirs) and len(mine) == want > 0, (len(mine), len(theirs), want)
    differ = [i for i in mine if not np.array_equal(mine[i], theirs[i])]
    assert not differ, f"EMLOCO_GEMM_WIDE_STORES=0 changed the bits of {len(differ)} of {len(mine)} outputs: {differ[:20]}"

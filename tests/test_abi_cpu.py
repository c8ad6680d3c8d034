"""CPU-only: the Python side of the C ABI against include/*.h -- the prototypes `emloco_amd._abi` reads, what `_lib.load()` binds,
and the hand-written mirrors (structures, constants) that a header edit would otherwise leave behind silently."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from emloco_amd import _abi, _lib as L
from test_capi_and_model import _declared

STRUCTS = {"EmlocoSimParams": L.SimParams, "EmlocoModelDesc": L.ModelDesc, "EmlocoSelfCollisionDesc": L.SelfCollisionDesc,
           "EmlocoTaskBufs": L.TaskBufs, "EmlocoResetBufs": L.ResetBufs, "EmlocoResetPool": L.ResetPool,
           "EmlocoLocoValStep": L.LocoValStep, "EmlocoLocoValEval": L.LocoValEval}
UNMIRRORED = {"EmlocoLocoValRecord"}                     # a device table read back as 32-bit words (learning/locoval_eval.py), never built on the host
ALIASES = {"GEMM_ACC": "EMLOCO_GEMM_ACCUMULATE", "GEMM_A16": "EMLOCO_GEMM_A_BF16MEM", "GEMM_B16": "EMLOCO_GEMM_B_BF16MEM",
           "GEMM_C16": "EMLOCO_GEMM_C_BF16MEM", "GEMM_MASK16": "EMLOCO_GEMM_MASK_BF16MEM", "ATTN_QKV16": "EMLOCO_ATTN_QKV_BF16MEM"}
vp, ci, cf, cd, i64, u32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_int64, C.c_uint32, C.c_uint64


def _text(header):
    """The header without comments (preprocessor lines kept)."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(_abi.INCLUDE, header)).read(), flags=re.S)


@pytest.mark.parametrize("header", _abi.HEADERS)
def test_parser_finds_every_prototype(header):
    """against the crude regex of test_capi_and_model.py, written independently: a prototype the parser dropped shows here"""
    parsed = _abi.parse(header)
    assert sorted(parsed) == _declared(header)
    mapped = set(_abi.SCALARS.values()) | {vp}
    for name, (restype, argtypes) in parsed.items():
        assert restype in mapped | {C.c_char_p} and all(t in mapped for t in argtypes), name


def test_parser_refuses_what_it_cannot_map(tmp_path, monkeypatch):
    monkeypatch.setattr(_abi, "INCLUDE", str(tmp_path))
    for i, proto in enumerate(("int emloco_a(long double x);", "int emloco_b(EmlocoSimParams by_value);", "short emloco_c(void);",
                               "float *emloco_d(int n);", "int emloco_e(int);", "int other_f(int n);")):
        (tmp_path / f"bad{i}.h").write_text("/* c */\n#include <stdint.h>\nint emloco_fine(int n, const float *x);\n" + proto + "\n")
        with pytest.raises(L.EmlocoError, match=rf"bad{i}\.h.*{proto.split('(')[0].split()[-1].lstrip('*')}"):      # names header and prototype
            _abi.parse(f"bad{i}.h")


def test_bind_refuses_a_library_that_lacks_a_declared_function():
    with pytest.raises(L.EmlocoError, match="does not export emloco_"):
        _abi.bind(object())


def test_load_binds_every_function_as_declared():
    lib = L.load()
    # arity and return type of every function, read off the header text with two crude patterns of this test's own
    sigs = [(n, a) for h in _abi.HEADERS for n, a in re.findall(r"\b(emloco_[a-z0-9_]+)\s*\(([^)]*)\)", _text(h))]
    rets = [(r, n) for h in _abi.HEADERS for r, n in re.findall(r"^(int|int64_t|float|const char \*)\s*(emloco_\w+)\s*\(", _text(h), flags=re.M)]
    assert len(sigs) == len(rets) == len(_abi.prototypes())
    for name, args in sigs:
        assert getattr(lib, name).argtypes is not None, name
        assert len(getattr(lib, name).argtypes) == (0 if args.strip() in ("", "void") else args.count(",") + 1), name
    for ret, name in rets:
        assert getattr(lib, name).restype is {"int": ci, "int64_t": i64, "float": cf, "const char *": C.c_char_p}[ret], name
    # the signatures where a wrong width would not show as a wrong arity
    assert lib.emloco_sim_tensor.argtypes == [vp, ci, vp, vp]                                          # int64_t shape[2]
    assert lib.emloco_adam_clip_flat.argtypes == [i64, vp, vp, vp, vp, cf, cd, cd, cf, cf, cf, cf, cf, vp, vp]
    assert lib.emloco_gemm_f32_ex.argtypes == [ci, ci, ci, ci, cf, vp, ci, i64, ci, vp, ci, i64, ci, vp, ci, i64, vp, ci, ci, vp, cf, u32, vp]
    assert lib.emloco_task_reset_obs_pooled.argtypes == [vp, vp, vp, ci, vp, vp, ci, u64, vp, vp, vp, vp]
    assert lib.emloco_obs_normalize.argtypes == [ci, ci, vp, ci, vp, vp, cf, cf, ci, vp, ci, vp, ci, vp]   # (was called with no argtypes at all)
    assert lib.emloco_adam_clip_flat_workspace.argtypes == [i64]
    for name in ("emloco_gemm_relu_bwd_workspace", "emloco_layernorm_bwd_workspace", "emloco_colsum_workspace", "emloco_rms_update_workspace",
                 "emloco_locoval_bwd_workspace", "emloco_locoval_variant_bwd_workspace", "emloco_adam_clip_flat_workspace",
                 "emloco_gemm_split_image_words", "emloco_ffn_bwd_colsum_rows"):
        assert getattr(lib, name).restype is i64, name
    assert lib.emloco_last_error.restype is C.c_char_p and lib.emloco_last_error.argtypes == []
    assert lib.emloco_sim_last_step_ms.restype is cf and lib.emloco_task_last_ms.restype is cf


def _structs():
    """{name: [(field, "ptr" | ctypes scalar)]} of every `typedef struct { ... } Name;` of the headers."""
    out = {}
    for h in _abi.HEADERS:
        for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", _abi.source(h)):
            fields = out[name] = []
            for decl in filter(str.strip, body.split(";")):
                first, *more = decl.replace("*", " * ").split(",")           # `const float *kp, *kd`: one type, a star per declarator
                base, *first = [w for w in first.split() if w != "const"]
                for d in [first] + [m.split() for m in more]:
                    assert len(d) == 1 + ("*" in d) and re.fullmatch(r"\w+", d[-1]), f"{name}: cannot parse `{decl.strip()}`"
                    fields.append((d[-1], "ptr" if "*" in d else _abi.SCALARS[base]))       # (an unmapped scalar is a KeyError)
    return out


def test_structure_mirrors_follow_the_headers():
    parsed = _structs()
    assert set(parsed) == set(STRUCTS) | UNMIRRORED
    assert len(parsed["EmlocoResetBufs"]) == 54 and ("vscale", cf) in parsed["EmlocoTaskBufs"]     # the `float a, b;` lists are split
    for name, mirror in STRUCTS.items():
        assert [(f, "ptr" if t is vp or issubclass(t, C._Pointer) else t) for f, t in mirror._fields_] == parsed[name], name


def test_structure_mirrors_have_the_compilers_size(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc to ask for sizeof")
    (tmp_path / "sizes.c").write_text("".join(f'#include "{h}"\n' for h in _abi.HEADERS) + "#include <stdio.h>\nint main(void) {\n" + "".join(
        f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in STRUCTS) + "    return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", _abi.INCLUDE, "-o", str(tmp_path / "sizes"), str(tmp_path / "sizes.c")])
    sizes = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "sizes")], text=True).splitlines())
    assert {n: C.sizeof(m) for n, m in STRUCTS.items()} == {n: int(s) for n, s in sizes.items()}


def test_constant_mirrors_follow_the_headers():
    from emloco_amd import model
    from emloco_amd.predictor import ops
    consts = {}
    for txt in map(_text, _abi.HEADERS):                 # `#define NAME <int>` and `NAME = <int>` enumerators
        for k, v in re.findall(r"^[ \t]*#define[ \t]+(EMLOCO_\w+)[ \t]+(-?\d+)[ \t]*$", txt, flags=re.M) + re.findall(r"\b(EMLOCO_\w+)\s*=\s*(-?\d+)", txt):
            assert consts.setdefault(k, int(v)) == int(v)
    # the two computed ones: the header's expressions, restated
    assert "#define EMLOCO_TASK_OBS (2 * EMLOCO_TRAJ_SAMPLES + EMLOCO_HEIGHT_POINTS)\n" in _text("emloco_task.h")
    assert "#define EMLOCO_OBS (EMLOCO_SELF_OBS + EMLOCO_TASK_OBS)\n" in _text("emloco_task.h")
    consts["EMLOCO_TASK_OBS"] = 2 * consts["EMLOCO_TRAJ_SAMPLES"] + consts["EMLOCO_HEIGHT_POINTS"]
    consts["EMLOCO_OBS"] = consts["EMLOCO_SELF_OBS"] + consts["EMLOCO_TASK_OBS"]
    checked = {}
    for mod in (L, ops, model):                          # every integer that a module spells like a header constant
        for py, val in vars(mod).items():
            c = ALIASES.get(py, "EMLOCO_" + py)
            if py.isupper() and type(val) is int and c in consts:
                assert val == consts[c], f"{mod.__name__}.{py} = {val}, {c} = {consts[c]}"
                checked[c] = mod
    # ... which is all of NB NDOF MAXC MAXCAND, SELF_OBS .. AMP_STEPS (8), T_* (7), POST_* (9), RESET_* (8), RND_* (14), POOL_FLOATS in _lib,
    # EVAL_MOMENTS, GEMM_* (12), ATTN_* (3), LOCOVAL_* (4) in ops, GEOM_* (3) and SC_MAXSEG in model
    assert all(sum(m is mod for m in checked.values()) >= n for mod, n in ((L, 51), (ops, 20), (model, 4))), sorted(checked)
    assert set(ALIASES.values()) | {"EMLOCO_NB", "EMLOCO_OBS", "EMLOCO_T_WARM_START", "EMLOCO_POST_AMP_DONE_ONLY", "EMLOCO_RND_DSPEED"} <= set(checked)

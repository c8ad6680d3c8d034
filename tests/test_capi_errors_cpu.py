"""The C ABI's one error channel: every refusal of every translation unit of libemloco_hip.so leaves its text in emloco_last_error(),
per thread, and prints nothing; `_lib.check` is the one place that turns a status into an EmlocoError with that text.

Every call below is refused by an argument check that comes before any HIP call (all pointers NULL, all sizes 0), so the answers
need no device."""
import ctypes as C
import threading

import pytest

E_ARG, E_NODEV = -1, -4          # EMLOCO_E_ARG, EMLOCO_E_NODEV (include/emloco_sim.h)

# one refusal per translation unit (csrc/*_capi.hip): entry point, the bad argument that all-NULL / all-zero arguments amount to
UNITS = (
    ("emloco_sim_create", "NULL params and handle"),                    # sim_capi.hip
    ("emloco_task_post_physics", "NULL buffers"),                       # task_capi.hip
    ("emloco_act_bwd", "total = 0"),                                    # predictor_capi.hip
    ("emloco_attention_fwd_queries", "n_query = 0"),                    # attention_capi.hip
    ("emloco_ffn_fwd", "M = 0"),                                        # ffn_capi.hip
    ("emloco_ppo_critic_head_fwd", "B = 0"),                            # ppo_capi.hip
    ("emloco_locoval_eval_reduce", "n_env = 0"),                        # eval_capi.hip
    ("emloco_motion_build", "null device arrays"),                      # motion_capi.hip
    ("emloco_getup_split", "NULL buffers"),                             # getup_capi.hip
)


@pytest.fixture(scope="module")
def lib():
    from emloco_amd import _lib as L
    return L.load()


def refuse(lib, name):
    """Call `name` with every pointer NULL and every scalar 0; returns (status, text)."""
    fn = getattr(lib, name)
    rc = fn(*[None if t is C.c_void_p else 0 for t in fn.argtypes])
    return rc, lib.emloco_last_error().decode()


@pytest.mark.parametrize("name,bad", UNITS, ids=[u[0] for u in UNITS])
def test_every_unit_refuses_into_the_one_channel(lib, capfd, name, bad):
    rc, text = refuse(lib, name)
    assert rc == E_ARG, (name, bad)
    assert name in text, (name, bad, text)
    out = capfd.readouterr()
    assert out.err == "" and out.out == ""


@pytest.mark.parametrize("first,second", [("emloco_sim_create", "emloco_task_post_physics"), ("emloco_task_post_physics", "emloco_act_bwd"),
                                          ("emloco_getup_split", "emloco_sim_create")])
def test_the_text_is_the_last_failing_calls_whatever_its_unit(lib, first, second):
    rc, text = refuse(lib, first)
    assert rc == E_ARG and first in text
    rc, text = refuse(lib, second)
    assert rc == E_ARG and second in text and first not in text


def test_the_text_is_per_thread(lib):
    _, mine = refuse(lib, "emloco_sim_create")
    seen = {}

    def other():
        seen["fresh"] = lib.emloco_last_error()
        seen["rc"], seen["text"] = refuse(lib, "emloco_ffn_fwd")

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["fresh"] == b""                                        # a thread starts with no text
    assert seen["rc"] == E_ARG and "emloco_ffn_fwd" in seen["text"]
    assert lib.emloco_last_error().decode() == mine and "emloco_sim_create" in mine


def test_check_raises_with_the_text_of_the_call_it_checks(lib):
    """The status of a task entry point, checked right after a simulator refusal on the same thread: the error carries the task
    unit's reason (before the single channel it carried the simulator's stale one, the task unit's went to stderr only)."""
    from emloco_amd import _lib as L
    rc, sim_text = refuse(lib, "emloco_sim_create")
    assert rc == E_ARG and sim_text
    rc = lib.emloco_task_post_physics(None, 0, None, 0, None)
    with pytest.raises(L.EmlocoError) as err:
        L.check(rc, "emloco_task_post_physics")
    said = str(err.value)
    assert "emloco_task_post_physics: null buffers" in said and f"code {E_ARG}" in said
    assert sim_text not in said and "emloco_sim_create" not in said
    L.check(0, "anything")                                              # success raises nothing


def test_the_predictor_ops_raise_through_the_same_check(lib):
    from emloco_amd import _lib as L
    from emloco_amd.predictor import ops
    assert ops._chk is L.check
    rc, text = refuse(lib, "emloco_act_bwd")
    with pytest.raises(L.EmlocoError, match="emloco_act_bwd: bad argument"):
        ops._chk(rc, "emloco_act_bwd")


def test_no_device_is_reported_with_a_text(lib, capfd):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from emloco_amd import _lib as L
    refuse(lib, "emloco_ffn_fwd")                                       # some other text first
    params = L.default_sim_params()
    handle = C.c_void_p()
    assert lib.emloco_sim_create(C.byref(params), 0, C.byref(handle)) == E_NODEV
    text = lib.emloco_last_error().decode()
    assert text and "emloco_ffn_fwd" not in text
    assert capfd.readouterr().err == ""


# a launch refused for a variant knob, in a process that starts with the knob set: (variable, value, entry point, arguments that pass every
# argument check -- the pointers are never dereferenced: the knob is consulted ahead of the launch)
_A = 4096                                # a 16-byte-aligned non-NULL "device address"
KNOB_REFUSALS = (
    ("EMLOCO_GEMM_BK", "7", "emloco_gemm_f32_ex", (1, 64, 64, 64, 1.0, _A, 64, 0, 0, _A, 64, 0, 0, _A, 64, 0, None, 0, 1, None, 0.0, 0, None)),
    ("EMLOCO_GEMM_WIDE_STORES", "off", "emloco_gemm_f32_ex", (1, 64, 64, 64, 1.0, _A, 64, 0, 0, _A, 64, 0, 0, _A, 64, 0, None, 0, 1, None, 0.0, 0, None)),
    ("EMLOCO_GEMM_WIDE_STORES", "2", "emloco_gemm_relu_bwd", (64, 64, 64, _A, 64, _A, 64, 0, _A, _A, 1.0, _A, _A, 0, None)),
    ("EMLOCO_ATTN_BWD_PIECES", "30", "emloco_attention_bwd_queries", (1, 8, 8, 1, 32, 0.5, _A, None, _A, _A, _A, _A, _A, 64, 0.0, 0, None)),
    ("EMLOCO_ATTN16_OLD", "yes", "emloco_attention_fwd_queries", (1, 8, 8, 1, 32, 0.5, _A, None, _A, _A, 64, 0.0, 0, None)),
    ("EMLOCO_ATTN16_OLD", "", "emloco_attention_bwd_queries", (1, 8, 8, 1, 32, 0.5, _A, None, _A, _A, _A, _A, _A, 16 | 32, 0.0, 0, None)),
)


@pytest.mark.parametrize("knob,value,entry,args", KNOB_REFUSALS, ids=[f"{k[0]}={k[1]}" for k in KNOB_REFUSALS])
def test_a_launch_refuses_a_knob_value_outside_its_list(knob, value, entry, args):
    """csrc/capi_knobs.h: the variant knobs accept their documented values only; the first launch that consults one that holds anything
    else returns EMLOCO_E_ARG with a text naming the variable and its value, and emloco_kernel_variants reports -1 for it"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C, sys; from emloco_amd import _lib as L; lib = L.load(); "
            f"rc = lib.{entry}(*{args!r}); print('launch', rc, lib.emloco_last_error().decode()); "
            "v = (C.c_int32 * 4)(); rc = lib.emloco_kernel_variants(v); print('report', rc, list(v), lib.emloco_last_error().decode())")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, **{knob: value}), capture_output=True, text=True)
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("launch", "report"))}
    assert r.returncode == 0 and set(lines) == {"launch", "report"}, r.stderr[-2000:]
    assert lines["launch"].startswith(f"launch {E_ARG} {entry}: {knob}={value}: "), lines["launch"]
    slot = ("EMLOCO_ATTN_BWD_PIECES", "EMLOCO_ATTN16_OLD", "EMLOCO_GEMM_WIDE_STORES", "EMLOCO_GEMM_BK").index(knob)
    want = [2, 0, 1, 0]
    want[slot] = -1
    assert lines["report"].startswith(f"report {E_ARG} {want} emloco_kernel_variants: {knob}={value}: "), lines["report"]


def test_kernel_variants_reports_the_parsed_knobs():
    """unset: the defaults; every documented value is accepted and reported (one child with all four set)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ("EMLOCO_ATTN_BWD_PIECES", "EMLOCO_ATTN16_OLD", "EMLOCO_GEMM_WIDE_STORES", "EMLOCO_GEMM_BK")
    env = {k: v for k, v in os.environ.items() if k not in names}
    env["PYTHONPATH"] = root
    code = ("import ctypes as C; from emloco_amd import _lib as L; lib = L.load(); v = (C.c_int32 * 4)(); "
            "print('report', lib.emloco_kernel_variants(v), list(v))")
    run = lambda **kw: subprocess.run([sys.executable, "-c", code], env=dict(env, **kw), capture_output=True, text=True).stdout.strip().splitlines()[-1]
    assert run() == "report 0 [2, 0, 1, 0]"
    assert run(EMLOCO_ATTN_BWD_PIECES="3", EMLOCO_ATTN16_OLD="1", EMLOCO_GEMM_WIDE_STORES="0", EMLOCO_GEMM_BK="32") == "report 0 [3, 1, 0, 32]"
    assert run(EMLOCO_ATTN_BWD_PIECES="2", EMLOCO_ATTN16_OLD="0", EMLOCO_GEMM_WIDE_STORES="1", EMLOCO_GEMM_BK="16") == "report 0 [2, 0, 1, 16]"
    from emloco_amd import _lib as L
    lib = L.load()
    assert lib.emloco_kernel_variants(None) == E_ARG and "emloco_kernel_variants: null argument" in lib.emloco_last_error().decode()

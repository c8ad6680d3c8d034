"""The rigid-body step's conformance matrix on the CPU emulator (case tables: tests/sim_abi_cases.py; the device run of the same
tables: tests/test_gpu_sim_matrix.py).  The emulated kernels stay on the oracle's bytes for every split of the substeps into parts
and on a height field that is neither square nor at the world origin; the key of the cost-ordered dispatch equals the float64
contact counts; the row copy of the indexed setters writes the listed rows and nothing else, -1 padding included."""
import numpy as np
import pytest

import emu
import sim_abi_cases as S


def _same(a, b, what):
    for name in S.NAMES:
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


@pytest.mark.parametrize("n_sub,n_calls,n_parts", S.SPLIT_CASES)
def test_split_cases_are_bit_exact_vs_oracle(n_sub, n_calls, n_parts, monkeypatch):
    """Every (n_sub, n_calls, n_parts) of the table: uneven and odd splits, and more parts than substeps (the emulator clamps the
    parts to the substep total as emloco_sim_step does)."""
    monkeypatch.setenv("EMLOCO_EMU_PARTS", str(n_parts))
    E = S.SPLIT_ENVS_EMU
    a = S.split_oracle(E, n_sub, n_calls)
    b = S.split_oracle(E, n_sub, n_calls)
    b.params.n_sub = n_sub                                     # the emulator multiplies by n_calls itself, as the launcher does
    for t in range(S.SPLIT_STEPS):
        a.step(1)
        emu.sim_step(b, n_calls)
        _same(a, b, f"step {t}")
    assert np.abs(a.contact_force).max() > 50.0


@pytest.mark.parametrize("kind", S.HF_KINDS)
def test_offset_nonsquare_heightfield_is_bit_exact_vs_oracle(kind, monkeypatch):
    """90 x 41 samples starting at (48.3, 52.7), sloped along x / along y / with one-cell risers (the slope-corrected mesh): two
    humanoids inside the field, one before its first row, one behind its last row, as the task's 4-part split launch."""
    monkeypatch.setenv("EMLOCO_EMU_PARTS", "4")
    a, _ = S.hf_oracle(kind, 4)
    b, _ = S.hf_oracle(kind, 4)
    b.params.n_sub = 2
    assert (getattr(a, "hf_mv", None) is not None) == kind.endswith("_risers")
    for t in range(S.HF_STEPS):
        a.step(1)
        emu.sim_step(b, 2)
        _same(a, b, f"{kind} step {t}")
    assert np.abs(a.contact_force).max() > 50.0


def test_float64_lookup_honours_the_origin():
    """contact_layout_cases._hf_plane on the offset field: the analytic plane of the gradient inside the field, the border cell's
    plane extended outside it (the samples are rounded to 0.005 m: half a unit of slack, plus the slope over that rounding)."""
    import contact_layout_cases as K
    for kind, g in (("slope_x", (0.3, 0.0)), ("slope_y", (0.0, 0.3))):
        hf = S.offset_field(kind)
        for (px, py) in S.HF_XY + ((48.31, 52.71), (57.19, 56.69)):
            zt, n, _ = K._hf_plane(hf, px, py)
            assert abs(zt - (g[0] * (px - 50.0) + g[1] * (py - 55.0))) < 0.006, (kind, px, py, zt)
            assert abs(n[0] + g[0] * n[2]) < 0.03 and abs(n[1] + g[1] * n[2]) < 0.03 and n[2] > 0.9, (kind, n)


@pytest.mark.parametrize("scene", S.KEY_SCENES)
def test_cost_key_is_the_float64_contact_count(scene):
    """Single-substep steps: the key a step leaves for the cost-ordered dispatch is 10 + the contacts kept (at most 20) where the
    float64 count at the state it starts from finds any, else 0 -- in every contact regime of the plane and `hf` scenes (cap at 20
    included), and on the offset field with env-steps in and out of contact."""
    a, hf = S.key_oracle(scene)
    b, _ = S.key_oracle(scene)
    a.fk()
    chk = S.KeyCheck()
    keys = np.full(a.E, 0xFFFFFFFF, np.uint32)
    for t in range(S.KEY_STEPS):
        chk.before_step(a, hf)
        a.step(1)
        emu.sim_step(b, 1, cost_ticks=keys)
        _same(a, b, f"{scene} step {t}")
        chk.after_step(keys, f"{scene} step {t}")
    print(f"cost key {scene}: {chk.doubtful} of {chk.doubtful + chk.compared} env-steps doubtful")
    assert chk.share_doubtful() <= S.KEY_MAX_DOUBTFUL
    if scene in ("plane", "hf"):
        chk.cov.check()
    else:
        assert 0 in chk.cov.counts and any(n > 0 for n in chk.cov.counts), sorted(set(chk.cov.counts))


GUARD, SENT = 512, np.float32(-7.25e11)


@pytest.mark.parametrize("row_len", [13, 138])
@pytest.mark.parametrize("case", range(6))
def test_copy_rows_writes_the_listed_rows_and_nothing_else(case, row_len):
    """copy_rows_kernel (the indexed setters with a foreign `dev_full`) on guarded host buffers: a sentinel band before and behind
    the destination, and a bitwise compare of everything but the listed rows with a copy taken before the launch.  An unchecked -1
    writes row_len floats ahead of the destination -- into the band."""
    name, ids, n_env = S.id_lists()[case]
    rng = np.random.default_rng(100 + case)
    src = rng.normal(size=(n_env, row_len)).astype(np.float32)
    buf = np.full(GUARD + n_env * row_len + GUARD, SENT, np.float32)
    dst = buf[GUARD:GUARD + n_env * row_len].reshape(n_env, row_len)
    dst[:] = rng.normal(size=(n_env, row_len)).astype(np.float32)
    before = buf.copy()
    src0 = src.copy()
    emu.sim_copy_rows(src, dst, ids, row_len, n_env)
    assert np.array_equal(buf[:GUARD].view(np.uint32), before[:GUARD].view(np.uint32)), f"{name}: a store landed ahead of the destination"
    assert np.array_equal(buf[-GUARD:].view(np.uint32), before[-GUARD:].view(np.uint32)), f"{name}: a store landed behind the destination"
    listed = np.zeros(n_env, bool)
    listed[ids[ids >= 0]] = True
    want = before[GUARD:GUARD + n_env * row_len].reshape(n_env, row_len).copy()
    want[listed] = src0[listed]
    assert np.array_equal(dst.view(np.uint32), want.view(np.uint32)), name
    assert np.array_equal(src.view(np.uint32), src0.view(np.uint32))


def test_copy_rows_ignores_ids_past_the_end():
    """(the check is free in the kernel; the header still calls an id >= n_env the caller's error)"""
    n_env, row_len = 4, 13
    src = np.ones((n_env, row_len), np.float32)
    buf = np.full(GUARD + n_env * row_len + GUARD, SENT, np.float32)
    buf[GUARD:-GUARD] = 0.0
    before = buf.copy()
    emu.sim_copy_rows(src, buf[GUARD:-GUARD], np.array([4, 40, -3], np.int32), row_len, n_env)
    assert np.array_equal(buf.view(np.uint32), before.view(np.uint32))

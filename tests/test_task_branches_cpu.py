"""Which branches of the kernels BETWEEN two rigid-body steps do the conformance tables take?  (CPU only.)

The twin of tests/test_sim_branches_cpu.py for chain_kernels.hip (compaction + order, the pooled reset / observation launch and its
launcher arithmetic), reset_kernels.hip, task_kernels.hip, task_device.h, traj_kernels.hip, order_device.h and
locoval_returns_device.h.  One child process, with the emulator built under --coverage, runs tests/task_branch_cases.py: the chain table
(tests/chain_cases.py) plus the existing reset, task, observation-pass and densifier tables, each with its own float64 / oracle / bit
assertions.  `gcov -b -c` is then read for EVERY object of the emulator library and summed per (file, line, branch index): the inline
functions of a header that emu_sim and emu_task both include are merged at link time, and the copy that runs may be counted in the other
object (order_device.h showed 0 executed lines inside emu_task alone although compact_order_kernel runs it).  A line that still holds a
never-taken branch, and any line of these files that never ran, must be on tests/golden/task_branches_allow.json with a count and one
sentence of reason -- unreachable by the code around it, or diagnostic; nothing else is listed.  Anything else fails the test and names
the line.  Under another major version of gcc than the allow-list records the table is printed and the test skips.

Measured (gcc 11.4; an inlined helper counts once per copy):

                                before: the whole CPU suite (571 tests)                 after: the tables of task_branch_cases.py
    chain_kernels.hip           82 / 129 lines, 59 / 180 branches, 49 lines short       129 / 129 lines, 174 / 180 branches,  5 lines short
    reset_kernels.hip           269 / 269 lines, 193 / 212 branches, 13 lines short     269 / 269 lines, 209 / 212 branches,  2 lines short
    task_kernels.hip            61 / 61 lines,  54 / 62 branches,  8 lines short        61 / 61 lines,  58 / 62 branches,  4 lines short
    task_device.h               204 / 204 lines, 186 / 190 branches,  4 lines short     204 / 204 lines, 188 / 190 branches,  2 lines short
    traj_kernels.hip            80 / 80 lines,  72 / 76 branches,  4 lines short        80 / 80 lines,  76 / 76 branches
    order_device.h              20 / 20 lines,  14 / 14 branches                        unchanged
    locoval_returns_device.h    30 / 30 lines,  24 / 24 branches                        unchanged

(Before: the 129 lines of chain_kernels.hip include the launcher arithmetic chain_pack / chain_pool_error, which moved there from
task_capi.hip with this gate; the pool-hit copy, the whole pool-draw role and every refusal were unexecuted.  Every line left short is
on the allow-list: launch-grid guards behind a grid that is exactly the count, clamps whose operand cannot leave its range, and a mode
test behind a launcher that refuses the other modes.)

Which case closes which line:
    chain_kernels.hip   pool-hit copy, pool-draw role, pool_hit, draw count            every sequence of chain_cases.SEQUENCES
                        chain_pool_error, every return                                 chain_cases.REFUSED / ACCEPTED
                        `n == 0 && !a->live_mode && !a->pool_next`                      "empty first call"; the two empty calls of run_live
                        the stamps (`a.prof`, a diagnostic)                            test_live_role_beside_a_pool (emulated stamps)
    reset_kernels.hip   `mid > t.n_motions - 1`, `li > t.n_valid - 1`                  direct case "uniform of one" (1.0, not TOP: see chain_cases)
                        the real_pick clamp, `is < mn`                                 "real-path edges"
                        `dmag > 0`                                                     "empty first segment"
                        `rmag > 0`                                                     "still root"
                        `u[EMLOCO_RND_INVERSION] > 0.5f`, `*inv_out = inv ? 1 : 0`     flag set "inversion"
                        `t.n_real > 0`, `phase > 1` of r_calc_pos                      "no real table, short trajectory"
                        `if (env < 0) break;` of traj_reset_kernel                     test_traj_reset_kernel_stops_at_the_padding_of_its_list
    task_kernels.hip    `env < 0` of post_physics_kernel                               run_live (a list with -1 entries in the middle)
                        `actions_copy`                                                 test_pd_targets_tail_and_action_copy
                        `out_h`, `out_px`                                              test_get_heights_kernel_with_either_output_left_out
    task_device.h       `mode & EMLOCO_POST_AMP_ROW` inside the AMP block              run_live (the history shift alone)
                        `lv_inverted &&`                                               test_flags_launch_with_the_return_bookkeeping_without_inversion_flags
    traj_kernels.hip    four refusals of densify_pack                                  test_emulated_entry_refuses_null_tables_...

Leaving a case out fails the gate and names the line (`python tests/task_branch_cases.py --skip EXPR` under --coverage), e.g.
    --skip "uniform and one"      reset_kernels.hip: 1 (allowed 0) x `if (li > t.n_valid - 1) li = t.n_valid - 1;`;
                                  reset_kernels.hip: 2 (allowed 1) x `if (mid > t.n_motions - 1) mid = t.n_motions - 1;`
    --skip "still and root"       reset_kernels.hip: 1 (allowed 0) x `const float root_rot = rmag > 0.0f ? atan2f(rvy, rvx) : 0.0f;`
    --skip "first and segment"    reset_kernels.hip: 1 (allowed 0) x `const float ih = dmag > 0.0f ? atan2f(dy, dx) : 0.0f;`
    --skip "edges"                reset_kernels.hip: 2 (allowed 0) x `if (t.real_pick) { ri = t.real_pick[bi]; ri = ri < 0 ? 0 : ...`;
                                  reset_kernels.hip: 1 (allowed 0) x `is = is < mn ? mn : is;`
"""
import json
import os
import shutil
import subprocess

import pytest

import gcov_branches as G

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOW = os.path.join(HERE, "golden", "task_branches_allow.json")
FILES = ("chain_kernels.hip", "reset_kernels.hip", "task_kernels.hip", "task_device.h", "traj_kernels.hip", "order_device.h",
         "locoval_returns_device.h")
# a library of its own (the flag names the file; -O1 is the emulator's level anyway): the rigid-body gate removes the counters of
# libemu_coverage* before it runs, and the two gates may run side by side
EXTRA = "-O1 --coverage"


def check(allow, tables):
    """the gate's rule on gcov's tables: what it finds beyond the allow-list (never-taken branches, lines never run) and the allow-list
    entries that are taken after all"""
    missed = G.never_taken(tables)
    for base, rows in G.never_executed(tables).items():
        for _, text in rows:
            missed.setdefault((base, text), 0)
            missed[(base, text)] = max(missed[(base, text)], 1)
    listed = {(e["file"], e["line"]): e["untaken"] for e in allow["lines"]}
    beyond = {k: n for k, n in missed.items() if n > listed.get(k, 0)}
    stale = {k: n for k, n in listed.items() if missed.get(k, 0) < n}
    return missed, listed, beyond, stale


@pytest.mark.skipif(shutil.which("gcov") is None or shutil.which("g++") is None, reason="gcov / g++ not on this machine")
def test_every_never_taken_branch_between_two_steps_is_accounted_for():
    with open(ALLOW) as f:
        allow = json.load(f)
    log = G.run_child("task_branch_cases.py", EXTRA)
    print(log[-600:])
    tables = G.gcov_tables(EXTRA, None, FILES)
    G.report(tables, FILES)
    missed, listed, beyond, stale = check(allow, tables)
    for (base, text), n in sorted(missed.items()):
        print(f"never taken: {base}: {n} x  {text}")
    print("allow-list:")
    for e in allow["lines"]:
        assert e["file"] in FILES and e["untaken"] >= 1 and len(e["reason"]) > 40, e
        print(f"  {e['file']}: {e['untaken']} x  {e['line']}\n      {e['reason']}")
    major = subprocess.run(["gcc", "-dumpversion"], stdout=subprocess.PIPE, text=True).stdout.strip().split(".")[0]
    if major != allow["gcc_major"]:
        pytest.skip(f"allow-list made with gcc {allow['gcc_major']} ({allow['gcc_version']}), this is gcc {major}: branch structure differs")
    assert not beyond, "branches no table takes and the allow-list does not explain: " + "; ".join(
        f"{b}: {n} (allowed {listed.get((b, t), 0)}) x `{t}`" for (b, t), n in sorted(beyond.items()))
    assert not stale, f"allow-list entries that are taken after all -- remove them: {stale}"

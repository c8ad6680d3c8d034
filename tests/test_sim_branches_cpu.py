"""Which branches of the rigid-body kernel do the bit-exact scenes take?  (CPU only; the device twin of the new scenes is
tests/test_gpu_sim_branches.py.)

The emulator (tests/emu) compiles emloco_amd/csrc/sim_kernels.hip itself with g++, so gcov can count its lines and branches.  One
child process, with EMLOCO_EMU_EXTRA=--coverage, runs the scene table of tests/sim_branch_cases.py through the emulated kernel and
the oracle -- bit equality on all six outputs after every control step -- and `gcov -b -c` then reports on the emulator's emu_sim
object.  Counts are summed over template instantiations and inlined copies per (source line, branch index); branches gcov marks as
exceptional (`throw`) are dropped.  A source line that still holds a never-taken branch must be on the committed allow-list
tests/golden/sim_branches_allow.json -- keyed by the line's stripped text, with the number of never-taken branches it may hold and one
sentence on why no input reaches them (or why they are timing / diagnostic only).  Anything else fails the test and names the line: a
path no scene enters can hold any bug while every bit-exact test stays green.

Branch structure belongs to the compiler: under another major version of gcc than the allow-list records the table is printed and the
test skips.  `pytest -s` prints taken / total per file and the allow-list.

Measured (gcc 11.4, counts summed as above; an inlined helper counts once per copy, so totals are larger than a per-function view):

                          before: the 56 emulator tests of the rigid-body step     after: the table of sim_branch_cases.py
    sim_kernels.hip       953 / 957 lines, 1461 / 1512 branches, 37 lines short    954 / 957 lines, 1490 / 1512 branches, 17 lines short
    sim_math.h            65 / 65 lines,     10 / 12 branches,    2 lines short    65 / 65 lines,     11 / 12 branches,    1 line short
    dev_math.h            31 / 31 lines,     38 / 38 branches                      unchanged
    fk_device.h           44 / 44 lines,     44 / 44 branches                      unchanged

Every line left short is on the allow-list with its reason (unreachable by the code around it, hand-over timing, or diagnostics).
Closed by new scenes: the sign flip of fdet_sincos (joint angles at and beyond pi); the root clamp `n > prm.max_ang_vel` and the
side of `prm.max_ang_vel < wlim` where the rotation cap binds alone (root spin, the second on a height field: the copy of the link
limiter in the height-field instantiation had never run, which gcov showed as two dead branches in one inlined ld4); the tie rule of
the contact cut in the lane's two slots and in the butterfly; `dist2 <= 1e-12`, `vt2 <= 1e-12`, `sc_mu == 0` in the limb-limb
phase; the edge-region sides `d3 > 0` / `d6 > 0` of obtuse wall triangles, the face-normal fall-back and
its line, and the turned-over side of the orientation test in mesh_plane.  Closed by the emulator taking the launcher's arguments
(order, id list, skip flags, ticks, id list of the forward kinematics, grids rounded up): the hand-over buffer's null side and every
launch-level branch of sim_step_kernel, sim_fk_kernel and copy_rows_kernel.  The contact-matrix lines (`row < nr`, `if (big)`,
`nc > 0` in the packed layout) are classified unreachable: the packed layout is entered with more than 14 contacts.

One scene is not visible to gcov: g++ -O1 compiles `hit && slot < EMLOCO_SC_MAXHITS` and the clamp of `nh` behind it without a branch
of their own, so limbs_more_hits_than_slots is held by its float64 hit count (more than 34 pairs) and by bit equality alone.

Leaving any other new scene out fails the test and names the line (`python tests/sim_branch_cases.py --skip NAME` under --coverage), e.g.
    without ties_at_the_20th_contact        sim_kernels.hip: 3 (allowed 1) x `if (act[s] && (cdist[s] > best || (cdist[s] == best && ...`
    without joint_angles_at_and_beyond_pi   sim_math.h: 1 (allowed 0) x `const float sgn = (((long)kf) & 1) ? -1.0f : 1.0f;`
"""
import json
import os
import shutil
import subprocess

import pytest

import gcov_branches as G

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOW = os.path.join(HERE, "golden", "sim_branches_allow.json")
FILES = ("sim_kernels.hip", "sim_math.h", "dev_math.h", "fk_device.h")        # (sim_pair_kernels.hip: an unshipped experiment)
EXTRA = "--coverage"


def run_table(extra_args=()):
    """The scene table in a fresh child (tests/gcov_branches.py); returns its output."""
    return G.run_child("sim_branch_cases.py", EXTRA, extra_args)


def gcov_tables():
    """`gcov -b -c` on the emulator's emu_sim object"""
    return G.gcov_tables(EXTRA, ("emu_sim",), FILES)


never_taken = G.never_taken


def report(tables):
    G.report(tables, FILES)


@pytest.mark.skipif(shutil.which("gcov") is None or shutil.which("g++") is None, reason="gcov / g++ not on this machine")
def test_every_never_taken_branch_of_the_rigid_body_kernel_is_accounted_for():
    with open(ALLOW) as f:
        allow = json.load(f)
    log = run_table()
    print(log[-1500:])
    tables = gcov_tables()
    report(tables)
    missed = never_taken(tables)
    for (base, text), n in sorted(missed.items()):
        print(f"never taken: {base}: {n} x  {text}")
    print("allow-list:")
    listed = {}
    for e in allow["lines"]:
        assert e["file"] in FILES and e["untaken"] >= 1 and len(e["reason"]) > 40, e
        listed[(e["file"], e["line"])] = e["untaken"]
        print(f"  {e['file']}: {e['untaken']} x  {e['line']}\n      {e['reason']}")
    major = subprocess.run(["gcc", "-dumpversion"], stdout=subprocess.PIPE, text=True).stdout.strip().split(".")[0]
    if major != allow["gcc_major"]:
        pytest.skip(f"allow-list made with gcc {allow['gcc_major']} ({allow['gcc_version']}), this is gcc {major}: branch structure differs")
    beyond = {k: n for k, n in missed.items() if n > listed.get(k, 0)}
    assert not beyond, "branches no scene takes and the allow-list does not explain: " + "; ".join(
        f"{b}: {n} (allowed {listed.get((b, t), 0)}) x `{t}`" for (b, t), n in sorted(beyond.items()))
    stale = {k: n for k, n in listed.items() if missed.get(k, 0) < n}
    assert not stale, f"allow-list entries that are taken after all -- remove them: {stale}"

"""gcov over the emulator's own objects: what tests/test_sim_branches_cpu.py (the rigid-body step) and tests/test_task_branches_cpu.py (the
kernels between two steps) share.  The emulator (tests/emu) compiles the kernel sources with g++, so a build with --coverage counts their
lines and branches; a gate runs its case table in ONE child process against such a build and reads `gcov -b -c` afterwards.

Counts are summed per (source file, line, branch index) over template instantiations, inlined copies and -- when several objects are
read -- translation units; branches gcov marks as exceptional (`throw`) are dropped.  Inline functions of a header that two objects
include are merged at link time, so the copy that runs may be counted in another object than the one whose kernel called it: a gate
over headers reads every object of the library."""
import collections
import glob
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "emu", "_build")


def lib_stem(extra):
    """file name stem of the emulator library built with EMLOCO_EMU_EXTRA=extra (tests/emu/__init__.py: _SO)"""
    return "libemu_" + "".join(c for c in "".join(extra.split()) if c.isalnum())


def run_child(script, extra, extra_args=()):
    """`script` (under tests/) in a fresh child with EMLOCO_EMU_EXTRA=extra (tests/emu reads it at import); returns its output.  Counters
    of earlier runs are removed first: gcov adds up."""
    for f in glob.glob(os.path.join(BUILD, lib_stem(extra) + "*.gcda")):
        os.remove(f)
    env = dict(os.environ, EMLOCO_EMU_EXTRA=extra, PYTHONPATH=os.pathsep.join([ROOT, HERE] + sys.path))
    env.pop("EMLOCO_EMU_PARTS", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *extra_args], cwd=HERE, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _notes(extra, objects):
    """the newest notes file of each object (a rebuild leaves the older notes behind); objects None: every object of the library"""
    newest = {}
    for path in glob.glob(os.path.join(BUILD, lib_stem(extra) + "*.gcno")):
        obj = os.path.basename(path)[:-len(".gcno")].rsplit("-", 1)[-1]
        if (objects is None or obj in objects) and (obj not in newest or os.path.getmtime(path) > os.path.getmtime(newest[obj])):
            newest[obj] = path
    assert newest and (objects is None or set(newest) == set(objects)), ("the coverage build left no notes file for", objects, sorted(newest))
    return [newest[k] for k in sorted(newest)]


def gcov_tables(extra, objects, files):
    """{file: (lines executed, lines, {(line number, branch index): summed count}, source lines, {line number: summed count})} from
    `gcov -b -c` on the objects"""
    lines = {f: collections.defaultdict(int) for f in files}
    br = {f: collections.defaultdict(int) for f in files}
    src = {}
    for note in _notes(extra, objects):
        out = subprocess.run(["gcov", "-b", "-c", "--json-format", "--stdout", os.path.basename(note)], cwd=BUILD,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True).stdout
        for doc in out.splitlines():
            if not doc.startswith("{"):
                continue
            for f in json.loads(doc)["files"]:
                base = os.path.basename(f["file"])
                if base not in files:
                    continue
                for ln in f["lines"]:                                          # one entry per function instance that holds the line
                    lines[base][ln["line_number"]] += ln["count"]
                    for k, b in enumerate(x for x in ln["branches"] if not x["throw"]):
                        br[base][(ln["line_number"], k)] += b["count"]
                if base not in src:
                    path = f["file"] if os.path.isabs(f["file"]) else os.path.normpath(os.path.join(BUILD, f["file"]))
                    with open(path) as fh:
                        src[base] = fh.read().splitlines()
    res = {b: (sum(1 for v in lines[b].values() if v), len(lines[b]), dict(br[b]), src[b], dict(lines[b])) for b in files if b in src}
    assert set(res) == set(files), sorted(res)
    return res


def never_taken(tables):
    """{(file, stripped source text): number of never-taken branches on that line}"""
    out = collections.Counter()
    for base, (_, _, br, src, _) in tables.items():
        for (line, _), count in br.items():
            if count == 0:
                out[(base, src[line - 1].strip())] += 1
    return out


def never_executed(tables):
    """{file: [(line number, stripped text)]}: lines that hold code and never ran (they may hold no branch at all)"""
    return {base: [(ln, src[ln - 1].strip()) for ln, count in sorted(lines.items()) if count == 0] for base, (_, _, _, src, lines) in tables.items()}


def report(tables, files):
    for base in files:
        ex, n, br = tables[base][:3]
        print(f"{base}: {ex} / {n} lines executed, {sum(1 for v in br.values() if v)} / {len(br)} branches taken")

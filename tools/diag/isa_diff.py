"""Compare the gfx950 device code of this tree with another tree's, kernel symbol by kernel symbol.

For each translation unit both trees are compiled with the Makefile's flags (kernel_resources.FLAGS; hipcc -S --cuda-device-only) and
every symbol reports "same" or the number of differing instruction lines with the first difference; symbols that only one side has are
listed too.  Whole instruction lists are compared (only the function's number inside its module is taken out of the basic-block labels:
it follows the order of instantiation) — what a refactor that must not change generated code is checked with.  Needs only the compiler,
no GPU.
    python tools/diag/isa_diff.py OTHER_TREE [sources..] [-D...]      # exit status 1 when anything differs
Without sources: every .hip unit of the Makefile's SRC.
"""
import difflib
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import ROOT, demangle, kernel_isa  # noqa: E402


def makefile_sources():
    """The .hip translation units of the Makefile's SRC, in its order."""
    with open(os.path.join(ROOT, "Makefile")) as f:
        src = re.search(r"^SRC\s*:=\s*(.*)$", f.read(), re.M).group(1)
    return [s for s in src.split() if s.endswith(".hip")]


def normalise(lines):
    """Instruction lines without what is no part of an instruction: the number of the function inside its module in the basic-block
    labels (.LBB<function>_<block>), which follows the order the kernels are instantiated in."""
    return [re.sub(r"\.LBB\d+_", ".LBB_", t) for t in lines]


def diff_lists(a, b):
    """(number of instruction lines that differ, first differing pair) of two instruction lists."""
    n, first = 0, None
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        n += max(i2 - i1, j2 - j1)
        if first is None:
            first = (i1, a[i1] if i1 < i2 else "(nothing)", b[j1] if j1 < j2 else "(nothing)")
    return n, first


def compare(source, other, extra_flags=()):
    """[(symbol, "same" | "differs" | "only here" | "only there", detail)] for one translation unit, and the count of k_search symbols."""
    with ThreadPoolExecutor(2) as ex:
        fa, fb = ex.submit(kernel_isa, source, extra_flags, ROOT), ex.submit(kernel_isa, source, extra_flags, other)
        here, there = ({k: normalise(v) for k, v in f.result().items()} for f in (fa, fb))
    rows = []
    for sym in sorted(set(here) | set(there)):
        if sym not in there:
            rows.append((sym, "only here", ""))
        elif sym not in here:
            rows.append((sym, "only there", ""))
        elif here[sym] == there[sym]:
            rows.append((sym, "same", "%d instructions" % len(here[sym])))
        else:
            n, (at, x, y) = diff_lists(there[sym], here[sym])
            rows.append((sym, "differs", "%d lines, first at %d: there `%s` / here `%s`" % (n, at, x, y)))
    return rows


def main(argv):
    flags = [a for a in argv if a.startswith("-")]
    pos = [a for a in argv if not a.startswith("-")]
    if not pos:
        print(__doc__)
        return 2
    other, sources = os.path.abspath(pos[0]), pos[1:] or makefile_sources()
    bad = 0
    for src in sources:
        if not os.path.exists(os.path.join(other, src)):           # (a unit the other tree does not have: nothing existed before)
            print("%-36s only here" % src)
            continue
        rows = compare(src, other, flags)
        names = demangle([r[0] for r in rows])
        for (sym, what, detail), name in zip(rows, names):
            if what != "same":
                print("  %-10s %s\n             %s" % (what, name, detail))
        same = sum(1 for r in rows if r[1] == "same")
        nks = sum(1 for r, n in zip(rows, names) if "k_search<" in n and r[1] == "same")
        bad += len(rows) - same
        print("%-36s %3d symbols: %3d same (%d of them k_search), %d differ, %d only here, %d only there" % (
            src, len(rows), same, nks, sum(1 for r in rows if r[1] == "differs"), sum(1 for r in rows if r[1] == "only here"),
            sum(1 for r in rows if r[1] == "only there")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

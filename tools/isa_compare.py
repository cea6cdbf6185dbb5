#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 ISA two source trees compile to: the check of a refactor that must not move a kernel.

    python tools/isa_compare.py PARENT_TREE BRANCH_TREE conv_x3_pipe.hip conv_x3_patch.hip ... [-o profiles/NAME.txt]

Every listed file of thinktwice_amd/csrc is compiled in both trees with the library's own flags (build.FLAGS + build.EXTRA_FLAGS of
the tree this tool lies in) and `-x hip --cuda-device-only -S`.  The assembly is cut per function symbol; comments go, and the two
label families that carry a file-wide counter (.LBB<n>_<m>, .Lpost_getpc<n>) are renamed, so that a function's text does not depend
on what stands before it in the file.  Per symbol the tool prints the instruction count and `identical` or `differs`, whether the
kernel descriptor (the .amdhsa_* lines) is equal, and the symbols only one side has.  It compares text for equality and knows no
instruction names.  No GPU is needed.  Exit status 0: every symbol of every file is on both sides, identical, with equal descriptors.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+)\s*,\s*@function")
_END = re.compile(r"^\s*\.Lfunc_end\d+:")
_DESC = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_DESC_END = re.compile(r"^\s*\.end_amdhsa_kernel")
_LBB = re.compile(r"\.LBB\d+_(\d+)")
_GETPC = re.compile(r"\.Lpost_getpc\d+")


def normalise(lines):
    """The lines of one function as they are compared: comments and blank lines dropped, white space collapsed, .LBB<n>_<m> ->
    .LBB_<m> (n counts the file's functions), .Lpost_getpc<n> numbered in order of appearance inside the function."""
    out, getpc = [], {}
    for line in lines:
        line = " ".join(line.split(";", 1)[0].split())
        if not line:
            continue
        line = _LBB.sub(r".LBB_\1", line)
        line = _GETPC.sub(lambda m: getpc.setdefault(m.group(0), ".Lpost_getpc_%d" % len(getpc)), line)
        out.append(line)
    return out


def split_functions(text):
    """Assembly text of a file -> ({symbol: normalised body lines}, {kernel symbol: normalised descriptor lines}).  A body runs from
    the symbol's label to its .Lfunc_end; a descriptor from .amdhsa_kernel SYMBOL to .end_amdhsa_kernel."""
    bodies, descs = {}, {}
    pending, cur, cur_lines, desc, desc_lines = None, None, None, None, None
    for line in text.splitlines():
        if desc is not None:        # (the descriptor stands inside the function, in front of its end label)
            if _DESC_END.match(line):
                descs[desc] = normalise(desc_lines)
                desc = None
            else:
                desc_lines.append(line)
            continue
        m = _DESC.match(line)
        if m:
            desc, desc_lines = m.group(1), []
            continue
        if cur is not None:
            if _END.match(line):
                bodies[cur] = normalise(cur_lines)
                cur = None
            else:
                cur_lines.append(line)
            continue
        m = _TYPE.match(line)
        if m:
            pending = m.group(1)
        elif pending is not None and line.split(";", 1)[0].strip() == pending + ":":
            cur, cur_lines, pending = pending, [], None
    return bodies, descs


def instruction_count(body):
    """Lines of a normalised body that are neither labels nor directives."""
    return sum(1 for l in body if not l.endswith(":") and not l.startswith("."))


def compare(text_a, text_b):
    """Two assembly texts -> {"symbols": [(symbol, count a, count b, body identical, descriptor equal or None)], "only_a": [...],
    "only_b": [...]}: the symbols both sides have, in name order, and those only one side has."""
    (ba, da), (bb, db) = split_functions(text_a), split_functions(text_b)
    rows = []
    for s in sorted(set(ba) & set(bb)):
        desc = (da.get(s) == db.get(s)) if (s in da or s in db) else None
        rows.append((s, instruction_count(ba[s]), instruction_count(bb[s]), ba[s] == bb[s], desc))
    return {"symbols": rows, "only_a": sorted(set(ba) - set(bb)), "only_b": sorted(set(bb) - set(ba))}


def first_difference(text_a, text_b, symbol):
    """(index, line a, line b) of the first normalised line at which `symbol` differs, or None."""
    a, b = split_functions(text_a)[0][symbol], split_functions(text_b)[0][symbol]
    for i in range(max(len(a), len(b))):
        la, lb = (a[i] if i < len(a) else None), (b[i] if i < len(b) else None)
        if la != lb:
            return i, la, lb
    return None


def demangle(symbols):
    """{symbol: readable name} where the toolchain has llvm-cxxfilt, else the symbols themselves."""
    try:
        out = subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt"], input="\n".join(symbols), capture_output=True, text=True, check=True)
        names = out.stdout.splitlines()
        return dict(zip(symbols, names)) if len(names) == len(symbols) else {s: s for s in symbols}
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}


def assemble(tree, src, out):
    sys.path.insert(0, ROOT)
    from thinktwice_amd import build
    cmd = [build.HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["-x", "hip", "--cuda-device-only", "-S",
                                                                         os.path.join(tree, "thinktwice_amd", "csrc", src), "-o", out]
    subprocess.run(cmd, check=True)
    return open(out).read()


def report(src, res, texts):
    lines = ["== " + src]
    names = demangle([r[0] for r in res["symbols"]] + res["only_a"] + res["only_b"])
    ok = not res["only_a"] and not res["only_b"]
    for s, na, nb, same, desc in res["symbols"]:
        d = "" if desc is None else ("   descriptor equal" if desc else "   descriptor DIFFERS")
        n = "%7d" % na if na == nb else "%7d -> %d" % (na, nb)
        lines.append("%s  %-9s%s   %s" % (n, "identical" if same else "differs", d, names[s]))
        if not same:
            i, la, lb = first_difference(texts[0], texts[1], s)
            lines.append("          first difference at line %d:  %s  |  %s" % (i, la, lb))
        ok = ok and same and desc is not False
    for side, only in (("parent", res["only_a"]), ("branch", res["only_b"])):
        for s in only:
            lines.append("only in %s: %s" % (side, names[s]))
    return lines, ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="+", help="file names under thinktwice_amd/csrc")
    ap.add_argument("-o", "--output", help="also write the report to this file")
    ap.add_argument("-j", "--jobs", type=int, default=4)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.jobs) as ex:
        jobs = {(src, side): ex.submit(assemble, tree, src, os.path.join(tmp, "%s.%d.s" % (src, side)))
                for src in a.files for side, tree in enumerate((a.parent, a.branch))}
        out, all_ok = ["instructions, ISA text, kernel descriptor, symbol (parent -> branch where the counts differ)"], True
        for src in a.files:
            texts = (jobs[(src, 0)].result(), jobs[(src, 1)].result())
            lines, ok = report(src, compare(*texts), texts)
            out += lines
            all_ok = all_ok and ok
    out.append("RESULT: " + ("every kernel identical, descriptors equal" if all_ok else "DIFFERENCES"))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.output:
        open(a.output, "w").write(text)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())

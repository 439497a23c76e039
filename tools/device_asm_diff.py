#!/usr/bin/env python3
"""Is the device code of one translation unit the same in two source trees?

    python tools/device_asm_diff.py PARENT_TREE BRANCH_TREE [--unit sq_dense.hip] [--asm-a a.s --asm-b b.s]

Compiles smqtk_indexing_amd/csrc/<unit> of both trees with each tree's Makefile flags plus `--cuda-device-only -S`
(tools/mfma_hazard_lint.py compile_to_asm) and compares PER KERNEL SYMBOL, not per file: a host-only edit moves
functions around and renumbers labels.  A function's text runs from `.type NAME,@function` to its `.Lfunc_end`; a kernel
also has its `.amdhsa_kernel NAME` block.  Before comparing, the numbers in `.LBB<n>_`, `.Ltmp<n>`, `.Lfunc_*<n>` and
`.LJTI<n>` are replaced, comments and trailing blanks stripped.

Prints the symbols that exist on one side only and those whose bodies differ; exit status 0 when there are none.
--asm-a / --asm-b take assembly that was compiled already (about a minute per compile otherwise).
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_hazard_lint as L  # noqa: E402

_LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI)\d+")
_TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def _norm(line):
    line = line.split(";", 1)[0].split("//", 1)[0].rstrip()
    return _LABEL.sub(lambda m: "." + m.group(1) + "N", line)


def symbols(asm_text):
    """{symbol: normalised text of its function body and, for a kernel, its .amdhsa_kernel block}"""
    out, name, block = {}, None, None
    for raw in asm_text.splitlines():
        m = _TYPE.match(raw)
        k = _KERNEL.match(raw)
        if m:
            name, block = m.group(1), "body"
            out.setdefault(name, [])
        elif k:
            name, block = k.group(1), "desc"
            out.setdefault(name, []).append(".amdhsa_kernel")
            continue
        if name is None:
            continue
        line = _norm(raw)
        if line:
            out[name].append(line)
        if (block == "body" and raw.lstrip().startswith(".Lfunc_end")) or (block == "desc" and ".end_amdhsa_kernel" in raw):
            name = None
    return {k: "\n".join(v) for k, v in out.items()}


def compare(asm_a, asm_b):
    a, b = symbols(open(asm_a).read()), symbols(open(asm_b).read())
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
    return len(a), len(b), only_a, only_b, differ


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--unit", default="sq_dense.hip")
    ap.add_argument("--asm-a")
    ap.add_argument("--asm-b")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm = []
        for tag, tree, given in (("a", args.tree_a, args.asm_a), ("b", args.tree_b, args.asm_b)):
            if given:
                asm.append(given)
                continue
            csrc = os.path.join(tree, "smqtk_indexing_amd", "csrc")
            asm.append(L.compile_to_asm(os.path.join(csrc, args.unit), os.path.join(tmp, tag + ".s"), csrc=csrc))
        na, nb, only_a, only_b, differ = compare(*asm)
    print("%s: %d symbols in %s, %d in %s" % (args.unit, na, args.tree_a, nb, args.tree_b))
    for title, names in (("only in " + args.tree_a, only_a), ("only in " + args.tree_b, only_b), ("bodies differ", differ)):
        print("%s: %d" % (title, len(names)))
        for s in names:
            print("   " + s)
    same = not (only_a or only_b or differ)
    print("RESULT: " + ("every symbol equal" if same else "DEVICE CODE DIFFERS"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

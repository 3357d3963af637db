#!/usr/bin/env python3
"""Instruction identity of the kernels two builds share.

    python tools/isa_identity.py OLD_DIR NEW_DIR [--drop REGEX=REPL ...]

OLD_DIR and NEW_DIR hold device assembly of the same translation units
(hipcc <Makefile flags> --cuda-device-only -S X.hip -o DIR/X.s).  Kernels are
matched by demangled name; --drop rewrites OLD names first (template arguments
the new build no longer has).  A kernel's body is the text between its label
and its .Lfunc_end (the kernel descriptor included), comments stripped, local
labels renumbered, the kernel's own symbol replaced and section directives
dropped (a template's kernel lives in a COMDAT section).  Prints one
line per kernel: identical or the differing lines, and VGPRs, spills,
occupancy and LDS of both builds as the assembler recorded them."""
import difflib
import os
import re
import subprocess
import sys


def kernels(path):
    """{demangled name: (body lines, resources)} of one .s file"""
    text = open(path).read().splitlines()
    names = [ln.split()[1] for ln in text if ln.strip().startswith(".amdhsa_kernel")]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True).stdout.splitlines()
    out = {}
    for sym, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = d.replace("(anonymous namespace)::", "").replace("tmh::", "")
        d = re.sub(r"\(.*", "", d)
        i = next(k for k in range(len(text)) if text[k].startswith(sym + ":"))
        j = next(k for k in range(i, len(text)) if text[k].startswith(".Lfunc_end"))
        body, labels = [], {}
        for ln in text[i + 1:j]:
            ln = ln.split(";")[0].rstrip().replace(sym, "KERNEL")
            if ln.strip() and not ln.strip().startswith((".section", ".text")):
                body.append(ln)
        for ln in body:  # local labels in order of definition
            m = re.match(r"(\.LBB\d+_\d+):", ln)
            if m:
                labels[m.group(1)] = ".L%d" % len(labels)
        body = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.get(m.group(0), m.group(0)), ln)
                for ln in body]
        res = {}
        for ln in text[j:j + 60]:
            m = re.match(r"; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", ln)
            if m:
                res[m.group(1)] = int(m.group(2))
        out[d] = (body, res)
    return out


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    drops = [a.split("=", 1) for a in sys.argv[4:]] if len(sys.argv) > 3 else []
    for f in sorted(os.listdir(new_dir)):
        if not f.endswith(".s"):
            continue
        old, new = kernels(os.path.join(old_dir, f)), kernels(os.path.join(new_dir, f))
        canon = {}
        for name in old:
            c = name
            for pat, repl in drops:
                c = re.sub(pat, repl, c)
            canon.setdefault(c, []).append(name)
        print("== %s: %d kernels before, %d after" % (f, len(old), len(new)))
        for name in sorted(new):
            was = [n for n in canon.get(name, [])]
            if len(was) != 1:
                print("%-64s %s" % (name[:64], "NEW" if not was else "AMBIGUOUS %s" % was))
                continue
            (b0, r0), (b1, r1) = old[was[0]], new[name]
            diff = [d for d in difflib.unified_diff(b0, b1, lineterm="", n=0)
                    if d[0] in "+-" and not d.startswith(("+++", "---"))]
            rs = " ".join("%s %s" % (k, r1.get(k)) if r0.get(k) == r1.get(k)
                          else "%s %s->%s" % (k, r0.get(k), r1.get(k))
                          for k in ("NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize"))
            print("%-64s %5d insts %s | %s" % (
                name[:64], len(b1), "identical" if not diff else "%d LINES DIFFER" % len(diff), rs))
            for d in diff:
                print("      " + d)
        gone = sorted(n for c, ns in canon.items() if c not in new for n in ns)
        for n in gone:
            print("%-64s removed" % n[:64])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per-kernel textual comparison of two device-side assemblies of one source file, for changes that must not move the device code:

    hipcc <build.py's hip_flags()> --offload-device-only -S -Rpass-analysis=kernel-resource-usage -x hip device.hip -o X.s 2> X.remarks
    python scripts/kernel_asm_diff.py parent.s new.s [parent.remarks new.remarks]

A kernel is everything from its `.globl` line to the next one (instructions, kernel descriptor, the compiler's resource comments). The
order of the kernels in the file may differ, so the number of the function inside local labels (.LBB<n>_<m>, .Lfunc_end<n>, ..., and
BB<n>_<m> in the compiler's comments) is dropped before the comparison, and with it the padding in front of a comment, which depends on
the label's width; nothing else is. The remarks are compared as the figures of each kernel, without their source lines.
One line per kernel; exit status 1 if anything differs."""
import re
import sys

LABEL = re.compile(r"(?:\.L|\b)(BB|func_begin|func_end|tmp|JTI|CPI|_unnamed_)(\d+)(?=_|\b)")       # (block names in comments have no .L)


def kernels(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m or line.lstrip().startswith((".amdgpu_metadata", ".ident", ".p2alignl")):       # (.p2alignl: the file's trailer behind the last kernel)
            if name:
                out[name] = buf
            name, buf = (m.group(1) if m else None), []
        if name:
            buf.append(re.sub(r"[ \t]+;", " ;", LABEL.sub(lambda x: ".L" + x.group(1), line)))
    if name:
        out[name] = buf
    for buf in out.values():      # the lines that open the next kernel's section in front of its .globl are not this kernel's
        while buf and re.match(r"\s*\.(section\s+\.text|text|protected|weak|hidden|p2align)\b", buf[-1]):
            buf.pop()
    return out


def remarks(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            name = m.group(1).split(":", 1)[1].strip()
            out[name] = []
        elif name:
            out[name].append(m.group(1))
    return out


def main(argv):
    a, b = kernels(argv[1]), kernels(argv[2])
    ra, rb = (remarks(argv[3]), remarks(argv[4])) if len(argv) > 4 else ({}, {})
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name.startswith("__hip_cuid_"):      # (the compilation unit's id: a hash of the source file, no kernel)
            continue
        if name not in a or name not in b:
            verdict = "ONLY IN " + (argv[1] if name in a else argv[2])
        else:
            verdict = "same text" if a[name] == b[name] else "TEXT DIFFERS"
            if ra or rb:
                verdict += ", same figures" if ra.get(name) == rb.get(name) and name in ra else ", FIGURES DIFFER"
        bad += verdict != "same text" and verdict != "same text, same figures"
        fig = ra.get(name) or []
        pick = {k.strip(): v.strip() for k, v in (f.split(":", 1) for f in fig)}
        print("%-24s %6d lines  %s  %s" % (verdict, len(a.get(name) or b.get(name)), name,
                                           " ".join("%s=%s" % (k, pick[k]) for k in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]") if k in pick)))
    print("%d kernels in %s, %d in %s, %d differ" % (len(a), argv[1], len(b), argv[2], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

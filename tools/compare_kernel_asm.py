#!/usr/bin/env python3
"""Compare the kernels of two assembly listings of one translation unit (hipcc ... --offload-device-only -S), as a
refactor's check that device code did not change:

    python tools/compare_kernel_asm.py parent.s change.s

A plain text comparison that knows nothing about particular instructions.  Per kernel (by mangled name) it compares the
body between the kernel's label and the end of the function, the kernel descriptor (.amdhsa_kernel ... .end_amdhsa_kernel)
and, from the metadata, .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size.  Block labels
and function numbers (.LBB12_3, .Lfunc_end12, numbered temporaries) depend on a kernel's place in the file and are
renumbered; comments that name the source file's lines are dropped.  Exit status 1 if a kernel of the first file is missing
from the second or differs."""
import re
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def normalise(lines):
    out = []
    for line in lines:
        line = re.sub(r"\s*;.*$", "", line).rstrip()           # comments
        line = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI|LCPI)\d+", r".\1N", line)
        if line.strip():
            out.append(line)
    return out


def kernels(path):
    text = open(path).read().split("\n")
    found = {}
    names = [m.group(1) for line in text for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", line)] if m]
    for name in names:
        begin = next(i for i, line in enumerate(text) if line.startswith(name + ":"))
        end = next(i for i in range(begin, len(text)) if text[i].startswith(".Lfunc_end"))
        d0 = next(i for i, line in enumerate(text) if line.strip() == ".amdhsa_kernel " + name)
        d1 = next(i for i in range(d0, len(text)) if text[i].strip() == ".end_amdhsa_kernel")
        found[name] = {"body": normalise(text[begin + 1:end]), "descriptor": normalise(text[d0:d1])}
    # metadata: one YAML list item per kernel, its keys in alphabetical order
    meta = "\n".join(text[text.index("amdhsa.kernels:"):])
    for item in re.split(r"\n  - (?=\.agpr_count)", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", item).group(1)
        for f in FIELDS:
            found[name][f] = re.search(r"\n    %s:\s+(\S+)" % re.escape(f), item).group(1)
    return found


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    bad = 0
    for name in sorted(ka):
        if name not in kb:
            print("MISSING  ", name)
            bad += 1
            continue
        diff = [k for k in ka[name] if ka[name][k] != kb[name][k]]
        print("%-9s %s  (%d lines, vgpr %s sgpr %s lds %s scratch %s)%s" % (
            "DIFFERS" if diff else "same", name, len(ka[name]["body"]), *[ka[name][f] for f in FIELDS],
            "  <- " + ", ".join(diff) if diff else ""))
        bad += bool(diff)
    for name in sorted(set(kb) - set(ka)):
        print("NEW      ", name)
    print("%d kernels in %s, %d in %s, %d missing or different" % (len(ka), a, len(kb), b, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

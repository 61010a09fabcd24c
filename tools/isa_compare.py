#!/usr/bin/env python3
"""Compare the device code of two builds, kernel symbol by kernel symbol.

    tools/isa_compare.py PARENT_DIR BRANCH_DIR

Each directory holds one <file>.s per source of the Makefile's SRCS, written by
    hipcc <the Makefile's CXXFLAGS and per-file flags> --cuda-device-only -S <file>.hip -o DIR/<file>.s
Per kernel symbol the instruction stream (comments dropped, local labels renumbered in order of appearance, the kernel's
own name masked) and the .amdhsa_kernel descriptor are compared.  Prints per-file counts, and registers / LDS / scratch of
every symbol that differs; no instruction text.  Exit status 1 when anything differs.
"""
import os
import re
import subprocess
import sys


def kernels(path):
    """{symbol: (instruction stream, descriptor lines)} of one assembly file."""
    lines = open(path).read().split("\n")
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        desc = [l.strip().replace(name, "@K") for l in lines[i + 1:end]]
        start = max(j for j in range(i) if lines[j].startswith(name + ":"))
        labels = {}
        body = []
        for l in lines[start + 1:i]:
            l = l.split(";")[0].strip()
            if not l or l.startswith((".section", ".p2align")):
                continue
            l = re.sub(r"\.L\w+", lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), l)
            body.append(l.replace(name, "@K"))
        out[name] = (body, desc)
    return out


def field(desc, key):
    for l in desc:
        if l.startswith(".amdhsa_" + key + " "):
            return l.split()[-1]
    return "?"


def resources(k):
    body, desc = k
    insts = sum(1 for l in body if not l.startswith(".") and not l.endswith(":"))
    return ("vgpr %s accum_offset %s sgpr %s lds %s scratch %s insts %d" %
            (field(desc, "next_free_vgpr"), field(desc, "accum_offset"), field(desc, "next_free_sgpr"),
             field(desc, "group_segment_fixed_size"), field(desc, "private_segment_fixed_size"), insts))


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, r))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(parent, branch):
    files = sorted(f for f in os.listdir(parent) if f.endswith(".s"))
    assert files == sorted(f for f in os.listdir(branch) if f.endswith(".s")), "the two directories hold different files"
    bad = 0
    total = 0
    for f in files:
        kp, kb = kernels(os.path.join(parent, f)), kernels(os.path.join(branch, f))
        print("== %s: %d kernel symbols in the parent, %d in the branch" % (f[:-2] + ".hip", len(kp), len(kb)))
        only = sorted(set(kp) ^ set(kb))
        pretty = demangle(only + sorted(n for n in set(kp) & set(kb) if kp[n] != kb[n]))
        print("   symbol sets equal" if not only else "   symbol sets DIFFER")
        for n in only:
            print("   only in the %s: %s" % ("parent" if n in kp else "branch", pretty[n]))
        common = sorted(set(kp) & set(kb))
        same = [n for n in common if kp[n] == kb[n]]
        print("   identical (instruction stream and kernel descriptor): %d of %d" % (len(same), len(common)))
        for n in common:
            if kp[n] != kb[n]:
                print("   DIFFERS %s\n      parent: %s\n      branch: %s" % (pretty[n], resources(kp[n]), resources(kb[n])))
        bad += len(only) + len(common) - len(same)
        total += len(common)
    print("\n%d files, %d kernel symbols in both builds, %d differ or are unmatched" % (len(files), total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

#!/usr/bin/env python3
"""Instruction-for-instruction comparison of kernels in two gfx950 assembly files.

usage: kernel_asm_diff.py <old.s> <new.s> <kernel name substring>...

The .s files come from compiling csrc/probe_api.hip with the flags of ops/build.py plus
``--save-temps`` (probe_api-hip-amdgcn-amd-amdhsa-gfx950.s). For every kernel whose mangled name
contains one of the substrings, the body from its label to its end label is compared after dropping
comments and the function number in local labels (.LBB<n>_<k>, which shifts when kernels are added
or removed around it). Prints one line per kernel and exits 1 if any body differs or is missing.
"""
import difflib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name and re.match(r"^\.Lfunc_end\d+:", line):
            out[name], name = body, None
        elif name:
            text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            if text:
                body.append(text)
    return out


def main():
    old, new, wanted = kernels(sys.argv[1]), kernels(sys.argv[2]), sys.argv[3:]
    names = sorted(n for n in old if any(w in n for w in wanted))
    bad = not names
    for n in names:
        diff = list(difflib.unified_diff(old[n], new.get(n, []), lineterm="", n=0))
        bad |= bool(diff)
        print(f"{'DIFFERS' if diff else 'identical'} {len(old[n])} instructions {n}")
        if diff:
            print("\n".join(diff[:20]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the device code of two `hipcc --cuda-device-only -S` outputs function by function.

usage: tools/isa_diff.py A.s B.s

A host-side refactor must leave every kernel's text as it was. Functions may come out in another
order, and a function's local labels (.LBB<f>_<n>, .Ltmp<n>, .LJTI<f>_<n>, .Lfunc_end<f>) carry
the function's ordinal in the file; those numbers are rewritten to the function-relative order of
first appearance before the texts are compared. The assembler comments (from ';' to the end of a
line: the compiler's loop annotations name the same block numbers, and their column moves with a
label's width) are dropped. Nothing else is. Exit status 1 on any difference.
"""
import re
import sys

LOCAL = re.compile(r"\.L(?:BB|JTI|tmp|func_end|func_begin)[0-9_]+")


def functions(path):
    """{symbol: body text from its label to its .Lfunc_end}, {kernel symbols}"""
    out, kernels, name, body = {}, set(), None, []
    for line in open(path):
        m = re.match(r"([A-Za-z_$][\w$.]*):\s*(;.*)?$", line)
        if name is None and m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if k:
            kernels.add(k.group(1))
        if name is not None:
            body.append(line.split(";", 1)[0].rstrip() + "\n")
            if re.match(r"\.Lfunc_end\d+:", line):
                ids = {}
                text = LOCAL.sub(lambda x: ids.setdefault(x.group(0), f".L{len(ids)}"), "".join(body))
                out[name] = text
                name = None
    return out, kernels


def main():
    (fa, ka), (fb, kb) = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    if ka != kb:
        bad += 1
        print("kernel sets differ: only in A", sorted(ka - kb), "only in B", sorted(kb - ka))
    if set(fa) != set(fb):
        bad += 1
        print("function sets differ:", sorted(set(fa) ^ set(fb)))
    diff = [n for n in fa if n in fb and fa[n] != fb[n]]
    for n in diff:
        print("differs:", n)
    bad += len(diff)
    print(f"{len(ka)} kernels, {len(fa)} functions in A; {len(kb)} kernels, {len(fb)} functions "
          f"in B; {len(diff)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the device assembly of selected kernels between two builds, unit by unit.

    hipcc <Makefile's HIPFLAGS and DEVFLAGS> -I../include -Icsrc --cuda-device-only -S csrc/solve_X.hip -o DIR/solve_X.s
    tools/kernel_asm_diff.py DIR_A DIR_B [--match solve_kernel]

For every .s file present in both directories, the body of each function whose mangled name contains
the pattern (default: solve_kernel -- the solve and resume instantiations) is compared line by line.
Local labels carry the function's ordinal in its translation unit (.LBB<n>_<m>), which shifts when a
unit gains a kernel; they are renumbered per function before the comparison.  Exit status 1 when a
body differs or a kernel exists on one side only."""
import argparse
import os
import re
import sys


def functions(path, pat):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None and pat in m.group(1):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = line.split(";")[0].rstrip()  # (comments carry source line numbers)
            if s.strip() and not s.lstrip().startswith((".loc", ".file", ".cfi")):
                body.append(re.sub(r"\.L(BB|tmp|func_begin)\d+", r".L\1", s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--match", default="solve_kernel")
    args = ap.parse_args()
    bad = 0
    for f in sorted(os.listdir(args.a)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(args.b, f)):
            continue
        fa, fb = functions(os.path.join(args.a, f), args.match), functions(os.path.join(args.b, f), args.match)
        for k in sorted(set(fa) | set(fb)):
            if k not in fa or k not in fb:
                print(f"{f}: {k}: on one side only")
                bad += 1
            elif fa[k] != fb[k]:
                n = sum(x != y for x, y in zip(fa[k], fb[k])) + abs(len(fa[k]) - len(fb[k]))
                print(f"{f}: {k}: {n} differing lines")
                bad += 1
        print(f"{f}: {len(fa)} kernels, {sum(len(v) for v in fa.values())} instructions and labels compared")
    print("identical" if bad == 0 else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

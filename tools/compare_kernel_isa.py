#!/usr/bin/env python3
"""Are the kernels of OLD.s, instruction for instruction, the kernels of NEW.s [NEW2.s ...]?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only x.hip -o x.s
    python tools/compare_kernel_isa.py old/x.s new/x.s new/y.s

Every kernel of OLD must appear exactly once across the NEW files with the same body (`_Z...:` to `.Lfunc_end`; comments,
blank lines and directives dropped, `.LBB<n>_` labels renumbered).  For refactors that move or re-spell device code.
"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].strip()
        m = re.match(r"(_Z\w+):$", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name and line and (not line.startswith(".") or line.startswith(".LBB")):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main(old, *new):
    found, bad = {}, 0
    for path in new:
        for k, body in kernels(path).items():
            found.setdefault(k, []).append((path, body))
    for k, body in kernels(old).items():
        hits = found.get(k, [])
        same = len(hits) == 1 and hits[0][1] == body
        bad += not same
        print(f"{'same' if same else 'DIFFERENT' if len(hits) == 1 else f'found {len(hits)} times'}  {len(body):5d} lines  {k}")
    print(f"{bad} of {len(kernels(old))} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))

#!/usr/bin/env python3
"""Diff function bodies by name between two sets of gfx950 device assembly.

    tools/diff_kernel_asm.py OLD_DIR NEW_DIR

Each directory holds *.s files (hipcc -S --offload-device-only with the Makefile's HIPFLAGS) and, optionally, *.remarks files
(the stderr of the same compile with -Rpass-analysis=kernel-resource-usage).  Functions are matched by symbol across all files
of a directory, so a kernel may move from one unit to another.  What depends only on a function's position in its file is
normalised: the function number in local labels (.LBB12_3 -> .LBB_3, .Lfunc_end12) and the order of functions.  Comments
are dropped.  Exit status 0: same symbols, same instructions, same resource usage."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp)\d+")


def functions(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        name, body = None, []
        for line in open(path):
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if re.match(r"\.Lfunc_end\d+:", line):
                assert name not in out, f"{name} defined twice in {d}"
                out[name] = body
                name = None
                continue
            text = line.split(";")[0].rstrip()
            if text.strip():
                body.append(LABEL.sub(lambda m: ".L" + m.group(1), text))
    return out


def resources(d):
    out, name = {}, None
    for path in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        for line in open(path):
            m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?:\[[^\]]*\])?):\s+(\S+) \[-Rpass-analysis", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = m.group(2)
                out[name] = {}
            else:
                out[name][m.group(1).strip()] = m.group(2)
    return out


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    bad = 0
    for what, old, new in (("instructions", functions(old_dir), functions(new_dir)),
                           ("resource usage", resources(old_dir), resources(new_dir))):
        for n in sorted(set(old) - set(new)):
            print(f"{what}: only in {old_dir}: {n}"); bad += 1
        for n in sorted(set(new) - set(old)):
            print(f"{what}: only in {new_dir}: {n}"); bad += 1
        same = 0
        for n in sorted(set(old) & set(new)):
            if old[n] == new[n]:
                same += 1
            else:
                print(f"{what} differ: {n}"); bad += 1
        print(f"{what}: {same} functions identical, {len(old)} in {old_dir}, {len(new)} in {new_dir}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the kernel launches of two runs, launch shape by launch shape (the host-side companion of kernel_diff.py).

    tools/launch_diff.py OLD_DIR NEW_DIR

OLD_DIR and NEW_DIR hold the `*kernel_trace.csv` files of `rocprofv3 --kernel-trace --output-format csv -d DIR -- <program>` runs of the same
program on two builds of the library (searched recursively: one file per traced process).  For every kernel whose name starts with `k_`, a launch
is the key (name without parameter list, grid x/y/z, workgroup x/y/z, LDS bytes); the two runs are compared as MULTISETS of such keys, not as
sequences -- launches of two streams interleave differently from run to run.  One line per key whose count differs, then a summary line; exit
status 1 on any difference.  The columns are found by name in the CSV header.  For refactors of the launchers: every shape must still reach the
same instantiation with the same grid, block and LDS size, which kernel_diff.py cannot show.  Needs no GPU itself.
"""
import collections
import csv
import glob
import os
import sys

LDS_COLUMNS = ("LDS_Block_Size", "Group_Segment_Size")  # (the name differs between rocprofv3 releases)


def short_name(d):
    """'void k<bf16, 2>(bf16 const*, int) [clone .kd]' -> 'k<bf16, 2>'"""
    d = d.strip()
    if d.startswith("void "):
        d = d[5:]
    depth = 0
    for i, ch in enumerate(d):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return d[:i]
    return d.split(" [")[0]


def launches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"launch_diff: no *kernel_trace.csv under {directory}")
    out = collections.Counter()
    for f in files:
        with open(f, newline="") as fh:
            rd = csv.DictReader(fh)
            cols = rd.fieldnames or []
            lds = next((c for c in LDS_COLUMNS if c in cols), None)
            need = ["Kernel_Name"] + [f"{w}_Size_{a}" for w in ("Grid", "Workgroup") for a in "XYZ"]
            missing = [c for c in need if c not in cols] + ([] if lds else ["/".join(LDS_COLUMNS)])
            if missing:
                sys.exit(f"launch_diff: {f}: no column {', '.join(missing)}")
            for r in rd:
                name = short_name(r["Kernel_Name"])
                if name.startswith("k_"):
                    out[(name,) + tuple(int(r[c]) for c in need[1:]) + (int(r[lds]),)] += 1
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = launches(argv[1]), launches(argv[2])
    differ = 0
    for key in sorted(set(old) | set(new)):
        if old[key] != new[key]:
            differ += 1
            name, gx, gy, gz, bx, by, bz, lds = key
            print(f"DIFF  {name}  grid=({gx}, {gy}, {gz}) block=({bx}, {by}, {bz}) lds={lds}: {old[key]} -> {new[key]} launches")
    print(f"launch_diff: {sum(old.values())} / {sum(new.values())} launches of k_* kernels, {len(set(old) | set(new))} distinct (kernel, grid, block, LDS) keys, "
          f"{differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

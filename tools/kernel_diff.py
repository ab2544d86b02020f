#!/usr/bin/env python3
"""Compare the device code of two versions of the kernels, kernel by kernel.

    tools/kernel_diff.py OLD NEW [--glob 'rec_*.hip'] [--map REGEX=REPL ...] [--keep DIR]

OLD and NEW are source trees (their ocrs_models_amd/csrc/<glob> is compiled to assembly with the flags of ocrs_models_amd/build.py plus
`-S --cuda-device-only`) or directories of such `.s` files.  A kernel is identified by its demangled name without the parameter list, e.g.
`k_dz_apply<bf16, 2, 2, false, 1024>`, whatever file it lives in; `--map` renames old kernels before they are matched (re.sub on that name):

    --map 'k_act_pool_fwd_t<=k_act_pool_fwd<'

Two kernels are the same when their instruction streams, their `.amdhsa_kernel` descriptors (in both: comments dropped, the local label prefix
`.LBB<n>_` and the kernel's own symbol normalised -- they move when a kernel changes files or names) and their .vgpr_count, .agpr_count,
.sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size from the metadata are equal; a kernel whose metadata lacks one of these
numbers, or that has no descriptor, is an error.  A name that occurs in more than one file of a side is matched within its file.  One line per kernel -- same / DIFF / old-only / new-only -- then a summary line; exit status 1 if any
kernel differs.  For refactors that move kernels between files: nothing that is only moved may change.
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def build_flags():
    sys.path.insert(0, ROOT)
    from ocrs_models_amd import build as b
    return b._hipcc(), list(b.FLAGS)


def compile_tree(tree, pattern, outdir):
    hipcc, flags = build_flags()
    srcs = sorted(glob.glob(os.path.join(tree, "ocrs_models_amd", "csrc", pattern)))
    if not srcs:
        sys.exit(f"kernel_diff: no {pattern} under {tree}/ocrs_models_amd/csrc")
    os.makedirs(outdir, exist_ok=True)

    def cc(src):
        out = os.path.join(outdir, os.path.splitext(os.path.basename(src))[0] + ".s")
        r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", src, "-o", out], capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"kernel_diff: hipcc failed for {src}:\n{r.stderr}")

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(cc, srcs))
    return outdir


def demangle(names):
    tool = next((t for t in (shutil.which("llvm-cxxfilt"), "/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt", shutil.which("c++filt"))
                 if t and os.path.exists(t)), None)
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: short_name(d) for n, d in zip(names, out)}


def short_name(d):
    """'void k<bf16, 2>(bf16 const*, int)' -> 'k<bf16, 2>'"""
    d, depth = d.replace("(anonymous namespace)", "{anonymous}"), 0
    for i, ch in enumerate(d):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            d = d[:i]
            break
    return d[5:] if d.startswith("void ") else d


def parse_metadata(path, lines):
    """{mangled kernel name: {resource: value}} from the .amdgpu_metadata block; a kernel entry runs from its `  - ` line to the next one"""
    res, cur, in_meta = {}, None, False

    def close():
        if cur is not None:
            missing = [k for k in ("name",) + RES_KEYS if k not in cur]
            if missing:
                sys.exit(f"kernel_diff: {path}: metadata entry {cur.get('name', '?')} lacks {', '.join(missing)}")
            res[cur["name"]] = {k: cur[k] for k in RES_KEYS}

    for ln in lines:
        if ln.strip() == ".amdgpu_metadata":
            in_meta = True
        elif ln.strip() == ".end_amdgpu_metadata":
            close()
            cur, in_meta = None, False
        elif in_meta:
            m = re.match(r"^(  - |    )\.(\w+):\s*(.*)$", ln)  # kernel-level keys only (arguments are indented deeper)
            if m:
                if m.group(1) == "  - ":
                    close()
                    cur = {}
                if cur is not None:
                    cur[m.group(2)] = m.group(3).strip()
    return res


def parse_asm(path):
    """{mangled kernel name: (normalised instruction lines, normalised .amdhsa_kernel descriptor lines, {resource: value})} of one .s file"""
    lines = open(path).read().split("\n")
    out = {}
    for name, r in parse_metadata(path, lines).items():
        def norm(ln):
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].rstrip()).replace(name, "@SELF")
            return ln.replace(name[2:], "@SELF") if name.startswith("_Z") else ln  # (function-local statics: _ZZ<encoding>E<variable>)

        a = next((i for i, ln in enumerate(lines) if ln.startswith(name + ":")), None)
        d0 = next((i for i, ln in enumerate(lines) if ln.split() == [".amdhsa_kernel", name]), None)
        if a is None or d0 is None:
            sys.exit(f"kernel_diff: {path}: no {'body' if a is None else 'kernel descriptor'} for {name}")
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        end = next(i for i in range(a + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [norm(lines[i]) for i in range(a + 1, end) if not d0 <= i <= d1]
        desc = [norm(lines[i]) for i in range(d0, d1 + 1)]
        out[name] = ([ln for ln in body if ln.strip()], [ln for ln in desc if ln.strip()], r)
    return out


def load(arg, pattern, keep, tag):
    if os.path.isdir(os.path.join(arg, "ocrs_models_amd", "csrc")):
        arg = compile_tree(arg, pattern, os.path.join(keep, tag))
    found = []  # (mangled name, file, parsed)
    for s in sorted(glob.glob(os.path.join(arg, "*.s"))):
        found += [(name, os.path.basename(s), v) for name, v in parse_asm(s).items()]
    if not found:
        sys.exit(f"kernel_diff: no kernels found in {arg}")
    dm = demangle(sorted({n for n, _, _ in found}))
    count = {}
    for n, _, _ in found:
        count[dm[n]] = count.get(dm[n], 0) + 1
    kernels = {}
    for n, f, v in found:  # the same name in two files (anonymous namespaces, file-local kernels): keyed by file as well
        key = dm[n] if count[dm[n]] == 1 else f"{dm[n]} [{os.path.splitext(f)[0]}]"
        if key in kernels:
            sys.exit(f"kernel_diff: {arg}: two kernels named {key}")
        kernels[key] = v + (f,)
    for name, c in sorted(count.items()):
        if c > 1:
            print(f"note      {tag}: {c} kernels named {name}, matched by file", file=sys.stderr)
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--glob", default="rec_*.hip", help="sources of a tree to compile (default: rec_*.hip)")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="rename old kernels (re.sub on the demangled name)")
    ap.add_argument("--keep", metavar="DIR", help="keep the compiled .s files in DIR/old and DIR/new")
    a = ap.parse_args()
    keep = a.keep or tempfile.mkdtemp(prefix="kernel_diff_")
    try:
        old, new = load(a.old, a.glob, keep, "old"), load(a.new, a.glob, keep, "new")
    finally:
        if not a.keep:
            shutil.rmtree(keep, ignore_errors=True)
    renamed = {}
    for name, v in old.items():
        to = name
        for m in a.map:
            pat, _, repl = m.partition("=")
            to = re.sub(pat, repl, to)
        renamed[to] = v + (name,)
    same = diff = 0
    for name in sorted(set(renamed) | set(new)):
        if name not in new:
            print(f"old-only  {renamed[name][4]}  ({renamed[name][3]})")
        elif name not in renamed:
            print(f"new-only  {name}  ({new[name][3]})")
        else:
            (ob, od, orr, of, oname), (nb, nd, nr, nf) = renamed[name], new[name]
            what = [f"{k} {orr[k]} -> {nr[k]}" for k in RES_KEYS if orr[k] != nr[k]]
            for label, x, y in (("instructions", ob, nb), ("descriptor", od, nd)):
                if x != y:
                    first = next((i for i, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
                    what.append(f"{label} differ from #{first} ({len(x)} -> {len(y)} lines)")
            where = f"{of} -> {nf}" if of != nf else nf
            was = f"  (was {oname})" if oname != name else ""
            if what:
                diff += 1
                print(f"DIFF      {name}  ({where}){was}: " + "; ".join(what))
            else:
                same += 1
                print(f"same      {name}  ({where}){was}")
    only_old, only_new = len(set(renamed) - set(new)), len(set(new) - set(renamed))
    print(f"kernel_diff: {same + diff} kernels on both sides, {same} identical, {diff} differ; {only_old} only in old, {only_new} only in new")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two source trees (a parent exported with `git archive` or `git worktree`,
and the working tree): which kernels' instruction streams are the same, which are not, which exist on one side only.

    python tools/isa_compare.py PARENT_TREE NEW_TREE [-D DEFINE ...]

Every .hip of build.py's PRODUCT_HIP (with -D LZF_ANALYSIS: and of ANALYSIS_HIP) is compiled in each tree with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S
the assembly is cut up per kernel symbol, and the kernels are matched BY SYMBOL ACROSS ALL FILES (a kernel may have moved to another
source).  Two kernels are `identical` when their instruction streams are the same text, line by line, once the labels of a kernel are
numbered in the order they are defined (branch targets and the labels of inline assembly carry counters of the whole file) and the
file's __hip_cuid_<hash> symbol is taken out.  Instructions are counted from that text; VGPRs, SGPRs, LDS and scratch are the
kernel's own metadata.  The last line is `kernels: N, differing: M` (M counts a difference in the stream or in any of the four
resources); the exit status is 1 when M > 0 or a kernel stands on one side only.

Compiles and compares text on the CPU: needs hipcc, no GPU.  profiles/capi_split.txt and profiles/seg_split.txt hold its tables.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def load_build(tree):
    """The tree's build.py (rust-lz-fear_amd/build.py) as a module: PRODUCT_HIP, ANALYSIS_HIP, CSRC, hipcc()."""
    for d in sorted(os.listdir(tree)):
        p = os.path.join(tree, d, "build.py")
        if os.path.isdir(os.path.join(tree, d, "csrc")) and os.path.exists(p):
            spec = importlib.util.spec_from_file_location("lzf_build_" + re.sub(r"\W", "_", os.path.abspath(tree)), p)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            return mod
    sys.exit(f"{tree}: no <package>/build.py beside a csrc/")


def compile_tree(tree, defines, tmp, tag):
    b = load_build(tree)
    srcs = list(b.PRODUCT_HIP) + (list(b.ANALYSIS_HIP) if "LZF_ANALYSIS" in defines else [])
    base = [b.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S",
            "-I", os.path.join(os.path.abspath(tree), "include")] + [f"-D{d}" for d in defines]

    def one(s):
        out = os.path.join(tmp, tag + "_" + s.replace("/", "_") + ".s")
        subprocess.check_call(base + [os.path.join(b.CSRC, s), "-o", out])
        return os.path.splitext(os.path.basename(s))[0], out

    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", 0)) or os.cpu_count() or 4) as ex:
        return list(ex.map(one, srcs))


def kernels_of(asm_path):
    """{symbol: (instruction lines, {metadata key: value})} of one assembly file."""
    lines = open(asm_path).read().splitlines()
    meta, cur = {}, {}
    md = lines[lines.index("\t.amdgpu_metadata"):] if "\t.amdgpu_metadata" in lines else []
    for ln in md:                                      # amdhsa.kernels: an entry per kernel opens with "  - ", its own keys stand four columns in
        m = re.match(r"(  - |    )(\.[a-z_]+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == ".symbol":
            meta[cur[".symbol"][:-3]] = cur
    out = {}
    for sym in meta:
        start = next((i for i, ln in enumerate(lines) if ln.startswith(sym + ":")), None)
        if start is None:
            continue
        body = []
        for ln in lines[start + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].rstrip()             # comments (and the ;#ASMSTART marks) are no instructions
            if ln.strip():
                body.append(ln.strip())
        labels = {}
        for ln in body:
            m = re.match(r"([.\w$]+):$", ln)
            if m:
                labels.setdefault(m.group(1), f"L{len(labels)}")
        pat = re.compile("|".join(r"(?<![.\w$])" + re.escape(k) + r"(?![\w$])" for k in sorted(labels, key=len, reverse=True))) if labels else None
        text = []
        for ln in body:
            if ln.startswith(".") and not ln.endswith(":"):
                continue                               # directives (.p2align, .loc ...)
            if pat:
                ln = pat.sub(lambda m: labels[m.group(0)], ln)
            text.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln))
        out[sym] = (text, {k: meta[sym].get(k, "?") for k in META_KEYS})
    return out


def demangle(syms):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            names = subprocess.run([tool], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
            break
        except (OSError, subprocess.CalledProcessError):
            names = list(syms)
    short = {}
    for s, n in zip(syms, names):
        n = re.sub(r"^void ", "", n)
        n = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", n) if n != s else n      # the parameter list
        short[s] = n.replace("lzf::", "").replace("(anonymous namespace)::", "")
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="DEFINE")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="isa_compare_")
    sides = []
    for tag, tree in (("parent", a.parent), ("new", a.new)):
        ks = {}
        for fname, path in compile_tree(tree, a.defines, tmp, tag):
            for sym, (text, meta) in kernels_of(path).items():
                ks[sym] = (fname, text, meta)
        sides.append(ks)
    old, new = sides
    both = [s for s in old if s in new]
    names = demangle(sorted(set(old) | set(new)))
    print(f"defines: {' '.join(a.defines) or '(none: the product build)'}")
    print(f"  {'file (parent -> new)':<46} {'kernel':<62} {'instructions':<16} {'VGPRs':<10} {'SGPRs':<10} {'LDS':<16} {'scratch':<8} result")
    differing = 0

    def pair(x, y):
        return f"{x} -> {y}"

    for s in sorted(both, key=lambda s: (old[s][0], names[s])):
        (fo, to, mo), (fn, tn, mn) = old[s], new[s]
        same = to == tn and mo == mn
        differing += 0 if same else 1
        lds, scr = (mo[k] if mo[k] == mn[k] else pair(mo[k], mn[k]) for k in META_KEYS[2:])
        print(f"  {(fo if fo == fn else pair(fo, fn)):<46} {names[s][:61]:<62} {pair(len([l for l in to if not l.endswith(':')]), len([l for l in tn if not l.endswith(':')])):<16} "
              f"{pair(mo[META_KEYS[0]], mn[META_KEYS[0]]):<10} {pair(mo[META_KEYS[1]], mn[META_KEYS[1]]):<10} {lds:<16} {scr:<8} {'identical' if same else 'differs'}")
    for tag, a_, b_ in (("parent only", old, new), ("new only", new, old)):
        for s in sorted(a_):
            if s not in b_:
                print(f"  {tag}: {names[s]}  ({a_[s][0]})")
    one_side = len(old) + len(new) - 2 * len(both)
    if differing or one_side:
        print(f"(the assembly of both sides is left in {tmp})")
    else:
        shutil.rmtree(tmp)
    print(f"kernels: {len(both)}, differing: {differing}" + (f", on one side only: {one_side}" if one_side else ""))
    return 1 if differing or one_side else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the gfx950 ISA of two source trees, symbol by symbol (CPU only).

    python scripts/isa_diff.py TREE_A TREE_B [--must-match REGEX] [--keep DIR]

Every .hip of build.py's SOURCES in each tree is compiled with build.py's ARCH,
FLAGS and include paths plus `--cuda-device-only -S`.  Each .s is cut into one
block per symbol (kernels and out-of-line device functions, `sym:` to its
.Lfunc_end) with the kernel's .amdhsa_kernel directive block (registers, LDS,
scratch) attached; what depends only on the position in the unit is
normalised.  Prints the symbols that are identical, different, and present in
one tree only; exits 1 if a symbol matching --must-match differs or is missing.
It compares text and nothing else.
"""
import argparse
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

NORMALISE = [(re.compile(r"\s*;.*$"), ""), (re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
             (re.compile(r"\.Ltmp\d+"), ".Ltmp"), (re.compile(r"__hip_cuid_\w+"), "__hip_cuid")]


def load_build(tree):
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(tree))), os.path.join(tree, "cuda-phdslam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(tree, out):
    b = load_build(tree)
    srcs = [s for s in b.SOURCES if s.endswith(".hip")]

    def one(src):
        dst = os.path.join(out, src[:-4] + ".s")
        r = subprocess.run([b.hipcc(), f"--offload-arch={b.ARCH}", *b.FLAGS, "-I" + os.path.join(b.REPO, "include"), "-I" + b.CSRC,
                            "--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", dst], capture_output=True, text=True)
        if r.returncode:  # (warnings of a good compile are not repeated here)
            sys.exit(f"{os.path.join(b.CSRC, src)}: hipcc failed\n{r.stderr}")
        return dst
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, srcs))


def norm(line):
    for rx, rep in NORMALISE:
        line = rx.sub(rep, line)
    return line.rstrip()


def symbols(paths):
    """{symbol: normalised text} over the units: code from `sym:` to .Lfunc_end, plus the .amdhsa_kernel block."""
    syms = {}
    for path in paths:
        cur, kd, funcs = None, None, set()
        for raw in open(path):
            line = norm(raw)
            t = re.match(r"^\s*\.type\s+(\w+),@function$", line)
            if t:
                funcs.add(t.group(1))
            m = re.match(r"^(\w+):$", line)
            if m and cur is None and kd is None and m.group(1) in funcs:
                cur = m.group(1)
                syms[cur] = []
            elif cur is not None:
                if line.startswith(".Lfunc_end"):
                    cur = None
                elif line:
                    syms[cur].append(line)
            elif line.strip().startswith(".amdhsa_kernel "):
                kd = line.split()[1]
                syms.setdefault(kd, []).append(".amdhsa_kernel")
            elif kd is not None:
                if line.strip() == ".end_amdhsa_kernel":
                    kd = None
                elif line:
                    syms[kd].append(line)
    return {k: "\n".join(v) for k, v in syms.items() if v}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--must-match", default=None, help="regex of symbols that must be present in both trees and identical")
    ap.add_argument("--keep", default=None, help="keep the .s files under DIR/a and DIR/b")
    a = ap.parse_args()
    top = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    got = []
    for tag, tree in (("a", a.tree_a), ("b", a.tree_b)):
        os.makedirs(os.path.join(top, tag), exist_ok=True)
        got.append(symbols(assemble(os.path.abspath(tree), os.path.join(top, tag))))
    sa, sb = got
    same = sorted(k for k in sa if k in sb and sa[k] == sb[k])
    diff = sorted(k for k in sa if k in sb and sa[k] != sb[k])
    only = sorted([k + " (first only)" for k in sa if k not in sb] + [k + " (second only)" for k in sb if k not in sa])
    for title, names in (("identical", same), ("different", diff), ("in one tree only", only)):
        print(f"== {title} ({len(names)})")
        for k in names:
            print("  " + k)
    bad = [k for k in diff + only if a.must_match and re.search(a.must_match, k)]
    if a.must_match and not any(re.search(a.must_match, k) for k in same + diff + only):
        bad.append("(no symbol matches --must-match)")
    if bad:
        print("MUST-MATCH FAILED: " + ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

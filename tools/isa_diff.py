#!/usr/bin/env python3
"""Does a change leave the device code alone?  Compiles every maf-yolo_amd/csrc/*.hip of two revisions to gfx950 assembly with the
library's own flags (-ffp-contract=off for the objects the Makefile builds that way) and counts the differing lines per file.  The
`__hip_cuid_<hash>` lines are left out: the hash follows the source text.  CPU only, no GPU is opened.

  python tools/isa_diff.py HEAD~1 HEAD          # two revisions
  python tools/isa_diff.py HEAD                 # a revision against the working tree
  python tools/isa_diff.py HEAD -j 8 --keep /tmp/isa bottleneck.hip head_tail.hip
  python tools/isa_diff.py HEAD --flags=-DMAF_KO=1 conv_mfma_f16.hip    # the `make ko KO=1` build of one file

Exit status 1 if any file differs or fails to compile.
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "maf-yolo_amd/csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]


def export(rev, dst):
    """csrc/ and include/ of `rev` (None: the working tree) under dst, laid out as in the repository."""
    if rev is None:
        shutil.copytree(os.path.join(ROOT, CSRC), os.path.join(dst, CSRC), ignore=shutil.ignore_patterns("build"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(dst, "include"))
        return
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)


def no_contract(csrc):
    """The sources whose Makefile rule carries -ffp-contract=off."""
    lines = open(os.path.join(csrc, "Makefile")).read().split("\n")
    out = set()
    for i, l in enumerate(lines):
        if "-ffp-contract=off" in l:
            j = i
            while j > 0 and lines[j].startswith("\t"):
                j -= 1
            out.update(m + ".hip" for m in re.findall(r"build/(\w+)\.o", lines[j].split(":")[0]))
    return out


def compile_one(csrc, name, extra):
    out = os.path.join(csrc, name[:-4] + ".s")
    r = subprocess.run([HIPCC] + FLAGS + extra + [name, "-o", out], cwd=csrc, capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


def differing_lines(a, b):
    fa, fb = a + ".flt", b + ".flt"
    for src, dst in ((a, fa), (b, fb)):
        with open(src) as f, open(dst, "w") as g:
            g.writelines(l for l in f if "__hip_cuid_" not in l)
    r = subprocess.run(["diff", fa, fb], capture_output=True, text=True)
    return sum(1 for l in r.stdout.split("\n") if l.startswith(("<", ">")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev_a")
    ap.add_argument("rev_b", nargs="?", default=None, help="default: the working tree")
    ap.add_argument("-j", "--jobs", type=int, default=16)
    ap.add_argument("--keep", metavar="DIR", help="leave the two trees and their .s files here")
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, e.g. --flags=-DMAF_BN_PROFILE (the `make prof` build)")
    ap.add_argument("files", nargs="*", help="only these csrc/*.hip (default: all)")
    a = ap.parse_intermixed_args()
    if a.rev_b is not None and a.rev_b.endswith(".hip"):       # `HEAD file.hip`: a revision against the working tree, some files
        a.files.insert(0, a.rev_b)
        a.rev_b = None
    jobs = max(1, min(a.jobs, 16))
    top = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(top, exist_ok=True)
    sides = []
    for tag, rev in (("a", a.rev_a), ("b", a.rev_b)):
        d = os.path.join(top, tag)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        export(rev, d)
        sides.append(os.path.join(d, CSRC))
    names = [sorted(n for n in os.listdir(s) if n.endswith(".hip") and (not a.files or n in a.files)) for s in sides]
    work = [(s, n, a.flags.split() + (["-ffp-contract=off"] if n in no_contract(s) else [])) for s, ns in zip(sides, names) for n in ns]
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        done = dict(zip(((s, n) for s, n, _ in work), ex.map(lambda w: compile_one(*w), work)))
    bad = 0
    print("%-28s %s" % ("file", "%s .. %s" % (a.rev_a, a.rev_b or "working tree")))
    for n in sorted(set(names[0]) | set(names[1])):
        if n not in names[0] or n not in names[1]:
            verdict = "only in %s" % (a.rev_a if n in names[0] else a.rev_b or "working tree")
        else:
            (sa, ea), (sb, eb) = done[(sides[0], n)], done[(sides[1], n)]
            if sa is None or sb is None:
                verdict = "does not compile: " + (ea if sa is None else eb).strip().split("\n")[0]
            else:
                d = differing_lines(sa, sb)
                verdict = "identical" if d == 0 else "%d differing lines" % d
        bad += verdict != "identical"
        print("%-28s %s" % (n, verdict))
    if not a.keep:
        shutil.rmtree(top, ignore_errors=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

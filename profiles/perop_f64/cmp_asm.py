#!/usr/bin/env python3
"""Device code of generic.hip and generic64.hip, parent tree against this one.

    cmp_asm.py PARENT_CSRC THIS_CSRC

Each file of each tree is compiled to gfx950 assembly with the Makefile's
flags (-S --cuda-device-only), cut into kernels, and every kernel of the
parent is looked up in this tree by its demangled name -- with the per-op
kernels' renaming applied (k_fir64< X > is k_fir< double, X >, k_fir< X > is
k_fir< float, X >, k_epilogue64< T, B > is k_epilogue64< T >). The instruction
streams are compared after symbol names and .LBB labels are normalised;
comments and directives are dropped."""
import re
import subprocess
import sys

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
         "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-S", "--cuda-device-only", "-o", "-"]


def kernels(csrc, name):
    asm = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [name], cwd=csrc,
                         check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".LBB")):
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"_Z\w+", "SYM", line)
        out[cur].append(line)
    names = subprocess.run(["c++filt"] + list(out),
                           check=True, capture_output=True,
                           text=True).stdout.split("\n")
    return {key(n): out[s] for s, n in zip(out, names)}


def key(n):
    n = n.replace("(anonymous namespace)::", "").replace("avirhip::", "")
    n = n.split("(")[0].replace("void ", "").replace(" ", "")
    m = re.match(r"(k_fir|k_gather|k_upf)(64)?<(?:(float|double),)?(\w+)>", n)
    if m:
        f = m.group(3) or ("double" if m.group(2) else "float")
        return "%s<%s,%s>" % (m.group(1), f, m.group(4))
    return re.sub(r"(k_epilogue64<\w+),\w+>", r"\1>", n)


def main():
    parent, this = sys.argv[1], sys.argv[2]
    old, new = {}, {}
    for f in ("generic.hip", "generic64.hip"):
        old.update(kernels(parent, f))
        new.update(kernels(this, f))
    bad = 0
    for k in sorted(old):
        if k not in new:
            res = "MISSING"
        elif old[k] == new[k]:
            res = "same"
        else:
            d = [i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b]
            res = "DIFFERS (%d -> %d, first at %s)" % (
                len(old[k]), len(new[k]), d[:1])
        bad += res != "same"
        print("%-60s %5d  %s" % (k, len(old[k]), res))
    print("kernels of the parent: %d, of this tree: %d, not the same: %d" %
          (len(old), len(new), bad))
    print("only in this tree:", sorted(set(new) - set(old)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

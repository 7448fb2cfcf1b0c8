#!/usr/bin/env python3
"""Runs one row of tests/gpass_route_cases.py once, whole frames only, and no
reference: the program to put behind `rocprofv3 --kernel-trace --stats --`
when the launch sequence of a route is to be recorded or compared between two
builds of the library (profiles/gpass_route/README.md).

  python tools/gpass_route_trace.py --row NAME [--lib PATH]
  python tools/gpass_route_trace.py --row NAME --check DIR [--out FILE]
  python tools/gpass_route_trace.py --list

--check reads the *kernel_trace.csv files rocprofv3 left under DIR, prints the
library's launches in start order (kernel, grid, workgroup, LDS as the profiler
reports it) and fails unless they are the kernels the row names, call by call.
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launches(d):
    """The library's launches of a trace, in start order."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"),
                       recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return ["%s grid=%s wg=%s lds=%s" % (
        r["Kernel_Name"].replace("void avirhip::", "").replace("avirhip::", ""),
        r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"])
        for r in rows if "avirhip::" in r["Kernel_Name"]]


def check(G, row, d, out):
    got = launches(d)
    want = [k for (c, env, images), ks in zip(G.row(row)[1], G.row(row)[2])
            for _ in images for k in ks]
    text = "== %s\n%s\n" % (row, "\n".join(got))
    if out:
        open(out, "a").write(text)
    print(text, end="")
    bad = len(got) != len(want) or any(
        not g.startswith(w) for g, w in zip(got, want))
    if bad:
        print("%s: expected %r" % (row, want))
    return int(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row")
    ap.add_argument("--lib", help="the library to load instead of the tree's")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--check", metavar="DIR")
    ap.add_argument("--out", help="append the launch list to this file")
    a = ap.parse_args()
    if a.lib:
        os.environ["AVIRHIP_LIB"] = os.path.abspath(a.lib)  # (read on import)
    from avir_amd import abi
    from tests import gpass_route_cases as G
    from tests import window_cases as W
    if a.list:
        print("\n".join(G.NAMES))
        return 0
    if a.check:
        return check(G, a.row, a.check, a.out)
    lib = abi.load()
    for (c, env, images) in G.row(a.row)[1]:
        with G.environment(env):
            obj, p = G.plan(c)
            for kind in images:
                src = G.to_device(G.flat(G.image(c, kind), W.pitch(c)))
                rcs, got = G.run_device(lib, p, c, src, [(0, c[4])])
                print("%s %s %s %s -> %r" % (a.row, W.case_id(c), env, kind, rcs),
                      flush=True)
                if rcs != [0]:
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

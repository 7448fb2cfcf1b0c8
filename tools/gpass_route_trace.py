#!/usr/bin/env python3
"""Runs one row of tests/gpass_route_cases.py once, whole frames only, and no
reference: the program to put behind `rocprofv3 --kernel-trace --stats --`
when the launch sequence of a route is to be recorded or compared between two
builds of the library (profiles/gpass_route/README.md).

  python tools/gpass_route_trace.py --row NAME [--lib PATH]
  python tools/gpass_route_trace.py --row NAME --check DIR [--out FILE]
  python tools/gpass_route_trace.py --list
  python tools/gpass_route_trace.py --far --row GROUP [--lib PATH]
  python tools/gpass_route_trace.py --far --row GROUP --check DIR [--out FILE]
  python tools/gpass_route_trace.py --far --list

--far: GROUP is a family group of tests/far_row_cases.py; every row of it runs
once on its forced path, whole frame, at its `under` level (`wrap` where the
memory cap drops that one), from the pitched device buffer of
tests/test_gpu_far_rows.py. --check then lists the launches row by row (a
line of dashes stands for the fill and copy kernels between two rows) and
fails unless every row launched a kernel of the library
(profiles/far_rows/README.md).

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


def launches(d, sep=False):
    """The library's launches of a trace, in start order; sep: one "--" line
    for every run of other kernels between them."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"),
                       recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        if "avirhip::" in r["Kernel_Name"]:
            out.append("%s grid=%s wg=%s lds=%s" % (
                r["Kernel_Name"].replace("void avirhip::", "").replace(
                    "avirhip::", ""),
                r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"]))
        elif sep and out and out[-1] != "--":
            out.append("--")
    return out


def far_level(F, r):
    lv = F.level(r, "under")
    return F.level(r, "wrap") if lv.dropped else lv


def far_check(F, group, d, out):
    """The launches of a --far run, row by row."""
    got = launches(d, sep=True)
    runs = [[]]
    for g in got:
        if g == "--":
            runs.append([])
        else:
            runs[-1].append(g)
    runs = [r for r in runs if r]
    rows = F.group(group)
    text = "== %s\n" % group
    for i, r in enumerate(rows):
        lv = far_level(F, r)
        text += "-- %s %s (%d rows, pitch %d, path %d variant %d)\n%s\n" % (
            r["name"], lv.name, lv.sh, lv.pitch, r["path"], r["variant"],
            "\n".join(runs[i]) if i < len(runs) else "(nothing)")
    if out:
        open(out, "a").write(text)
    print(text, end="")
    if len(runs) != len(rows):
        print("%s: %d runs of launches for %d rows" % (group, len(runs),
                                                      len(rows)))
    return int(len(runs) != len(rows))


def far_run(F, group):
    """Every row of the group once: forced path, whole frame."""
    import ctypes as C
    import torch
    from avir_amd import abi
    from tests import gpass_route_cases as G
    from tests import test_gpu_far_rows as T
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    for r in F.group(group):
        lv = far_level(F, r)
        img = T._image(r, lv.sh)
        isz, osz = F.TYPES[r["tin"]][2], F.TYPES[r["tout"]][2]
        row_b = r["sw"] * r["ch"] * isz
        nh = 2 * lv.sh if r["by"] == "rows" else r["nh"]
        drow_b = r["nw"] * r["ch"] * osz
        # (both buffers first: the fills are the separator in front of a row)
        dst = T._Pitched(nh, drow_b,
                         lv.pitch * osz if r["by"] == "dst" else drow_b)
        src = T._Pitched(lv.sh, row_b,
                         row_b if r["by"] == "dst" else lv.pitch * isz)
        with G.environment(r["env"]):
            obj, p = T._plan(r, lv, r["path"])
            if p is None:
                print("%s: set_path refused" % r["name"])
                return 1
            src.put(img)
            torch.cuda.synchronize()
            rc = lib.avirhip_resize_band(
                p, C.c_void_p(src.ptr()), abi.MEM_DEVICE,
                C.c_void_p(dst.ptr()), abi.MEM_DEVICE, 0, nh, None)
            torch.cuda.synchronize()
        print("%s %s -> %d (path %d)" % (
            r["name"], lv.name, rc, lib.avirhip_plan_get_path(p)), flush=True)
        if rc != 0:
            return 1
        del obj, p, src, dst
        torch.cuda.empty_cache()
    return 0


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
    ap.add_argument("--far", action="store_true",
                    help="--row names a family group of tests/far_row_cases.py")
    a = ap.parse_args()
    if a.lib:
        os.environ["AVIRHIP_LIB"] = os.path.abspath(a.lib)  # (read on import)
    from avir_amd import abi
    from tests import gpass_route_cases as G
    from tests import window_cases as W
    if a.far:
        from tests import far_row_cases as F
        if a.list:
            print("\n".join(F.GROUPS))
            return 0
        if a.check:
            return far_check(F, a.row, a.check, a.out)
        return far_run(F, a.row)
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

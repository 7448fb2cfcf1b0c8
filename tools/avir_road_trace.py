#!/usr/bin/env python3
"""Runs every row of tests/avir_road_cases.py (--cases lanc:
tests/lanc_road_cases.py) once on one build of the library and writes, per row and call (the whole frame, then each band): the tags of the
call's AVIRHIP_VERBOSE lines in order, its return code, the device bytes the
plan holds after it (avirhip_plan_device_bytes) and a hash of the destination's
bytes. No reference is computed. Two builds are compared by running this once
per build -- each in a process of its own, the library named by AVIRHIP_LIB as
tools/ab_libs.sh names it -- and taking a `diff` of the two files
(profiles/avir_road/, profiles/lanc_road/).

  python tools/avir_road_trace.py [--cases avir|lanc] --lib PATH --out FILE
                                  [--row NAME ...]
"""
import argparse
import hashlib
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAG = re.compile(r"^(k_\w+|pack pass|output stage):", re.M)


class stderr_lines(object):
    """`with stderr_lines() as s:` -- what the process wrote to file descriptor
    2 meanwhile, in s.text."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.keep = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()
        return False


def trace_row(lib, R, r, out):
    src = R.source(r)
    keep, sptr = R.device_source(r, src)
    paths = [r["path"]] + ([0] if r["rc"] != 0 else [])
    for path in paths:
        with R.environment(dict(r["env"], AVIRHIP_VERBOSE="1")):
            obj, p = R.plan(r, path)
            nh = r["geom"][3]
            for (a, b) in [(0, nh)] + (R.bands(r) if path == r["path"] else []):
                with stderr_lines() as s:
                    rcs, got, clean = R.run(lib, p, r, sptr, [(a, b)])
                out.write("%s path %d rows %d:%d tags %r rc %d bytes %d "
                          "guards %s md5 %s\n" % (
                              r["name"], path, a, b, TAG.findall(s.text),
                              rcs[0], lib.avirhip_plan_device_bytes(p),
                              "clean" if clean else "WRITTEN",
                              hashlib.md5(got.tobytes()).hexdigest()))
                if rcs[0] != 0:
                    out.write("%s path %d error %r\n" % (
                        r["name"], path, lib.avirhip_last_error()))
            del obj, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="the library to load instead of the tree's")
    ap.add_argument("--out", required=True)
    ap.add_argument("--row", action="append")
    ap.add_argument("--cases", choices=("avir", "lanc"), default="avir")
    a = ap.parse_args()
    if a.lib:
        os.environ["AVIRHIP_LIB"] = os.path.abspath(a.lib)  # (read on import)
    from avir_amd import abi
    import importlib
    R = importlib.import_module("tests.%s_road_cases" % a.cases)
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    with open(a.out, "w") as out:
        for name in a.row or R.NAMES:
            try:
                trace_row(lib, R, R.row(name), out)
            except Exception as e:  # (a row the build cannot plan: recorded)
                out.write("%s failed: %s: %s\n" % (name, type(e).__name__, e))
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
